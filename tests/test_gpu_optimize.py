"""GPU: pre-training on the device -- tbnn_optimize (Adam / AMSGrad on the target log-probability; include/tbnn.h) on every kernel
family, and the Python surface over it (Chain / ChainGroup.optimize, network.pretrain, BNN_functions.trainBasic*).

Every handle asserts its kernel family; every optimiser call is repeated from the same start and must give the same bits.  The shapes are
ahead-of-time instantiations or those of tests/jit_shapes.json: nothing new is compiled here.

Bands.
  * Step arithmetic: with the device's own total gradient g and the moments before the step as inputs, the recursion evaluated in fp64 must
    give the device's m, v, vhat to 4 fp32 ulps of their magnitude (two roundings each, fused or not; for m, whose two terms cancel where the
    gradient has turned, the magnitude is that of the larger term: a rounding is an ulp of what was rounded) and the device's new theta to 1e-5 lr
    (a handful of fp32 roundings, the sqrt and the divide; a wrong bias correction, a misplaced epsilon or swapped betas moves the step by
    per cents).  theta itself is an fp32 number: adding the step rounds it by up to half an ulp of theta, 1.2e-7 for |theta| < 2 and 2.4e-7
    below 8 -- the states here stay below 8 (asserted) -- so these tests step at lr = 0.05, where 1e-5 lr = 5e-7 holds that rounding too;
    at lr = 1e-3 the band would be a twelfth of one ulp of theta and no fp32 state could meet it.
  * g against the fp64 oracle: the project's per-tensor band, 1e-4 of the tensor's largest entry (floor 1e-3), as tests/test_gpu_poisson.py.
  * Free run: 8 x the gap between the restatement's own fp32 arm and fp64 on the same run (tests/optim_ref.py computes it on the CPU, never
    from the kernel's output): two independent fp32 evaluations, times 4 for another summation order -- the rule of tests/test_gpu_poisson.py.
  * Hand-over, blocks, chain groups, repeats: bit for bit."""
import numpy as np
import pytest

import optim_ref as R
import tbnn_oracle as o
from tensor_checks import layers_of, tensor_errs

pytestmark = pytest.mark.gpu

FUSED = {"fast3": "", "mid": "fast3,fast,tall,wide", "tall": "fast3,fast,mid,wide", "wide": "fast3,fast,mid,tall"}
STEP_LR = R.F32(0.05)

# name -> (dims, rows, hidden activation, prior, likelihood, family)
CASES = {
    "fast3": ([6, 24, 24, 1], 1501, o.ACT_TANH, o.PRIOR_GAUSSIAN, o.LIK_GAUSSIAN, "fast3"),
    "fast3_deep": ([5, 49, 49, 49, 1], 3001, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, "fast3"),
    "mid": ([20, 100, 48, 2], 1000, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, "mid"),
    "tall": ([100, 64, 32, 1], 1205, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, "tall"),
    "wide": ([10, 200, 256, 1], 700, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, "wide"),
    "layered": ([7, 17, 33, 2], 777, o.ACT_TANH, o.PRIOR_GAUSSIAN, o.LIK_GAUSSIAN, "layered"),
    "generic": ([5, 16, 16, 4], 517, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, "generic"),
    "traj": ([1, 10, 10, 1], 500, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, "aot"),        # P = 141: one k_optim block; trajectory-eligible
}
assert all(CASES[k][:2] == R.FREE_RUN[k][:2] and CASES[k][3] == R.FREE_RUN[k][2] for k in R.FREE_RUN)


def problem(name):
    if name in R.FREE_RUN:
        return R.free_run(name)[0]
    dims, n, act, prior, lik, _fam = CASES[name]
    return R.problem(dims, n, prior, act, lik)


def make(native, monkeypatch, spec, fam, chains=0, **kw):
    """a Chain (chains = 0) or a ChainGroup of the family, its kernel name asserted"""
    def new(**k2):
        if chains:
            return native.ChainGroup(layers_of(spec), chains, likelihood=spec.likelihood, fixed_sd=spec.fixed_sd, **k2, **kw)
        return native.Chain(layers_of(spec), likelihood=spec.likelihood, fixed_sd=spec.fixed_sd, **k2, **kw)
    if fam in FUSED:
        monkeypatch.setenv("TBNN_JIT_SKIP", FUSED[fam])
        ch = new(jit=True)
        assert ch.kernel_name.startswith(f"jit-{fam}<"), ch.kernel_name
    elif fam == "aot":
        ch = new(jit=False)
        assert ch.kernel_name.startswith("fast3<"), ch.kernel_name
    elif fam == "layered":
        monkeypatch.setenv("TBNN_TALL", "0")
        monkeypatch.setenv("TBNN_REGISTERED", "0")
        ch = new(jit=False)
        assert ch.kernel_name.startswith("layered<"), ch.kernel_name
    else:
        ch = new(kernel=native.KERNEL_GENERIC)
        assert ch.kernel_name.startswith("generic"), ch.kernel_name
    return ch


def staged(native, monkeypatch, name, w=None):
    spec, X, Y, theta0, eta = problem(name)
    ch = make(native, monkeypatch, spec, CASES[name][5])
    ch.set_data(X, Y)
    if w is not None:
        ch.set_row_weights(w)
    ch.set_state(theta0)
    ch.set_hypers(eta)
    return ch, spec, X, Y, theta0, eta


def same(a, b):
    """two optimize() results agree bit for bit (the timing aside)"""
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a if k != "device_us")


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------- 1. step arithmetic, per family
@pytest.mark.parametrize("name", list(CASES))
def test_step_arithmetic(native, monkeypatch, name):
    ch, spec, X, Y, theta0, eta = staged(native, monkeypatch, name)
    P = spec.n_params
    th, m, v, vh = theta0.copy(), np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32)
    recs = []
    for t in range(1, 6):
        out = ch.optimize(1, lr=STEP_LR, check_every=1, keep="last", reset=(t == 1))
        st, new = ch.optim_state(), ch.get_state()
        recs.append((out, st, new))
        assert st["t"] == t and out["n_checks"] == 2 and out["diverged"] == 0 and np.all(np.isfinite(out["trace"]))
        assert np.abs(new).max() < 8.0                                    # (the rounding of theta the band allows for: see the docstring)
        g = st["g"].astype(np.float64)
        th64, m64, v64, vh64 = R.adam_step(th, g, m, v, vh, t, STEP_LR, dtype=np.float64)
        # (m's two terms cancel where the gradient has turned: its roundings are ulps of the larger term, not of the difference)
        m_mag = np.maximum(np.abs(m64), np.maximum(np.abs(R.B1 * m.astype(np.float64)), np.abs((1.0 - R.B1) * g)))
        for k, ref, mag in (("m", m64, m_mag), ("v", v64, v64), ("vhat", vh64, vh64)):
            err = np.abs(st[k].astype(np.float64) - ref)
            assert np.all(err <= 4 * ulp32(mag)), (name, t, k, float((err / ulp32(mag)).max()))
        es = np.abs(new.astype(np.float64) - th64).max()
        print(f"[optimize] {name} step {t}: theta err {es / STEP_LR:.2e} lr, |theta| max {np.abs(new).max():.2f}")
        assert es <= 1e-5 * STEP_LR, (name, t, es / STEP_LR)
        g64 = o.target_log_prob_and_grad(spec, th, eta, X, Y, np.float64)[1]
        eg = tensor_errs(spec, st["g"], g64, 1e-3)
        assert max(eg) <= 1e-4, (name, t, eg)
        th, m, v, vh = new, st["m"], st["v"], st["vhat"]
    # the same five calls from the same start: the same bits
    ch.set_state(theta0)
    for t in range(1, 6):
        out = ch.optimize(1, lr=STEP_LR, check_every=1, keep="last", reset=(t == 1))
        st, new = ch.optim_state(), ch.get_state()
        assert same(out, recs[t - 1][0]) and np.array_equal(new, recs[t - 1][2])
        assert all(np.array_equal(st[k], recs[t - 1][1][k]) for k in ("m", "v", "vhat", "g"))
    ch.close()


def test_both_slab_loops_at_100k_rows(native, monkeypatch):
    """fast3 at 100 k rows: more than 8 x UPD_GROUPS slabs, so the unrolled loop of upd_column_partial and its remainder loop both run"""
    dims, _n, act, prior, lik, fam = CASES["fast3"]
    spec, X, Y, theta0, eta = R.problem(dims, 100_003, prior, act, lik)
    ch = make(native, monkeypatch, spec, fam)
    ch.set_data(X, Y); ch.set_state(theta0); ch.set_hypers(eta)
    out = ch.optimize(1, lr=STEP_LR, check_every=1, keep="last")
    st, new = ch.optim_state(), ch.get_state()
    ch.set_state(theta0)
    assert same(ch.optimize(1, lr=STEP_LR, check_every=1, keep="last"), out) and np.array_equal(ch.get_state(), new)
    ch.close()
    lp64, g64 = o.target_log_prob_and_grad(spec, theta0, eta, X, Y, np.float64)
    assert abs(out["trace"][0] - lp64) <= 4e-6 * abs(lp64)
    assert max(tensor_errs(spec, st["g"], g64, 1e-3)) <= 1e-4
    th64 = R.adam_step(theta0, st["g"].astype(np.float64), 0 * g64, 0 * g64, 0 * g64, 1, STEP_LR)[0]
    assert np.abs(new.astype(np.float64) - th64).max() <= 1e-5 * STEP_LR


# ---------------------------------------------------------------- 2. free run against fp64
@pytest.mark.parametrize("name", list(R.FREE_RUN))
def test_free_run_against_fp64(native, monkeypatch, name):
    _pb, (tr64, th64), (tr32, th32) = R.free_run(name)
    gap_tr, gap_th = R.free_gaps(tr32, th32, tr64, th64)
    ch, spec, X, Y, theta0, eta = staged(native, monkeypatch, name)
    out = ch.optimize(R.FREE_STEPS, lr=R.LR, check_every=1, keep="last")
    th = ch.get_state()
    ch.set_state(theta0)
    assert same(ch.optimize(R.FREE_STEPS, lr=R.LR, check_every=1, keep="last"), out) and np.array_equal(ch.get_state(), th)
    ch.close()
    assert out["n_checks"] == R.FREE_STEPS + 1 and out["diverged"] == 0 and out["steps_done"] == R.FREE_STEPS
    assert out["obj_first"] == out["trace"][0] and out["obj_last"] == out["trace"][-1] and out["obj_best"] == out["trace"].max()
    assert out["best_step"] == int(np.argmax(out["trace"]))
    e_tr, e_th = R.free_gaps(out["trace"], th, tr64, th64)
    print(f"[optimize] {name}: trace err {e_tr:.3e} (band 8 x {gap_tr:.3e}), theta err {e_th:.3e} lr (band 8 x {gap_th:.3e} lr)")
    assert e_tr <= 8 * gap_tr and e_th <= 8 * gap_th, (name, e_tr, gap_tr, e_th, gap_th)


# ---------------------------------------------------------------- 3. hand-over to the sampler
def strip(rec):
    return {k: v for k, v in rec.items() if k not in ("device_us", "fwdbwd_us")}


@pytest.mark.parametrize("name", ["fast3", "traj", "layered", "generic"])
def test_hand_over_to_the_sampler(native, monkeypatch, name):
    """optimize, then a weight and a hyper transition == the same two on a fresh handle given the state: no stale image, cached gradient
    or data term, no touched random stream"""
    ch, spec, X, Y, theta0, eta = staged(native, monkeypatch, name)
    ch.hmc_step(1e-4, 3)                                      # caches, images and the epoch counter in use before the optimiser runs
    ch.optimize(12, lr=R.LR, check_every=5, keep="best")
    theta1, eta1 = ch.get_state(), ch.get_hypers()
    a = [strip(ch.hmc_step(2e-4, 4)), strip(ch.hyper_step(1e-3, 5)), ch.get_state(), ch.get_hypers(), ch.last_transition_path]
    ch.close()
    fresh = make(native, monkeypatch, spec, CASES[name][5])
    fresh.set_data(X, Y); fresh.set_state(theta1); fresh.set_hypers(eta1); fresh.set_epoch(1)
    b = [strip(fresh.hmc_step(2e-4, 4)), strip(fresh.hyper_step(1e-3, 5)), fresh.get_state(), fresh.get_hypers(), fresh.last_transition_path]
    fresh.close()
    assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4], (a[:2], b[:2])
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    if name == "traj":
        assert a[4] == "trajectory"


# ---------------------------------------------------------------- 4. blocks
@pytest.mark.parametrize("name", ["fast3", "layered"])
def test_blocks_equal_one_call(native, monkeypatch, name):
    ch, spec, X, Y, theta0, eta = staged(native, monkeypatch, name)
    one = ch.optimize(40, lr=R.LR, check_every=10, keep="last")
    th_one, st_one = ch.get_state(), ch.optim_state()
    ch.set_state(theta0)
    parts = [ch.optimize(10, lr=R.LR, check_every=10, keep="last", reset=(b == 0)) for b in range(4)]
    th_four, st_four = ch.get_state(), ch.optim_state()
    ch.close()
    assert np.array_equal(th_one, th_four) and st_one["t"] == st_four["t"] == 40
    assert all(np.array_equal(st_one[k], st_four[k]) for k in ("m", "v", "vhat", "g"))
    assert np.array_equal(one["trace"], np.concatenate([parts[0]["trace"]] + [p["trace"][1:] for p in parts[1:]]))
    assert all(parts[b]["trace"][0] == parts[b - 1]["trace"][1] for b in range(1, 4))
    assert parts[-1]["obj_best"] == one["obj_best"] and parts[-1]["best_step"] == one["best_step"]


# ---------------------------------------------------------------- 5. chain groups
@pytest.mark.parametrize("name", ["fast3", "layered"])
def test_group_equals_solo_chains(native, monkeypatch, name):
    spec, X, Y, theta0, eta = problem(name)
    rng = np.random.default_rng(3)
    starts = np.stack([theta0, theta0 + 0.05 * rng.standard_normal(theta0.size).astype(np.float32), 0.5 * theta0]).astype(np.float32)
    grp = make(native, monkeypatch, spec, CASES[name][5], chains=3)
    grp.set_data(X, Y); grp.set_state(starts); grp.set_hypers(eta)
    outs = grp.optimize(20, lr=R.LR, check_every=5, keep="best")
    th, st = grp.get_state(), grp.optim_state()
    grp.set_state(starts)
    again = grp.optimize(20, lr=R.LR, check_every=5, keep="best")
    assert all(same(x, y) for x, y in zip(outs, again)) and np.array_equal(grp.get_state(), th)
    grp.close()
    for c in range(3):
        ch = make(native, monkeypatch, spec, CASES[name][5])
        ch.set_data(X, Y); ch.set_state(starts[c]); ch.set_hypers(eta)
        solo = ch.optimize(20, lr=R.LR, check_every=5, keep="best")
        s1 = ch.optim_state()
        assert same(solo, outs[c]), (c, solo, outs[c])
        assert np.array_equal(ch.get_state(), th[c]) and all(np.array_equal(s1[k], st[k][c]) for k in ("m", "v", "vhat", "g"))
        ch.close()


# ---------------------------------------------------------------- 6. divergence is contained
def poisson_problem():
    spec = o.make_spec([1, 16, 16, 1], o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_POISSON, o.ACT_NONE)
    x = np.linspace(-2.0, 2.0, 500)
    X = x.reshape(-1, 1).astype(np.float32)
    Y = np.random.default_rng(11).poisson(np.exp(1.0 + np.sin(2.0 * x))).astype(np.float32).reshape(-1, 1)
    theta0 = o.synth_problem([1, 16, 16, 1], 8, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN)[3]
    return spec, X, Y, theta0, o.default_hypers(spec)[:spec.n_hypers]


def test_divergence_is_contained(native, monkeypatch):
    """arithmetic overflow, no device fault: at lr = 1e3 the first step throws the log-rates out of exp's fp32 range (the oracle: -inf after
    step 1, NaN after it, in both precisions).  Checked at every step, so the chain freezes with finite weights."""
    spec, X, Y, theta0, eta = poisson_problem()
    ref = R.run(spec, theta0, eta, X, Y, 2, lr=R.F32(1e3), dtype=np.float64)[0]
    assert np.isfinite(ref[0]) and ref[1] == -np.inf and not np.isfinite(ref[2])
    ch = make(native, monkeypatch, spec, "layered")
    ch.set_data(X, Y); ch.set_state(theta0); ch.set_hypers(eta)
    ok = ch.optimize(10, lr=R.F32(1e-2), check_every=1, keep="last")
    assert ok["diverged"] == 0 and np.all(np.isfinite(ok["trace"])) and np.all(np.isfinite(ch.get_state()))
    ch.set_state(theta0)
    bad = ch.optimize(10, lr=R.F32(1e3), check_every=1, keep="last")
    assert bad["diverged"] == 1 and bad["best_step"] == 0 and bad["steps_done"] == 1
    assert np.isfinite(bad["trace"][0]) and not np.any(np.isfinite(bad["trace"][1:])) and bad["obj_best"] == bad["trace"][0]
    assert np.array_equal(ch.get_state(), theta0)
    # the handle goes on: a transition from the start state matches the oracle
    p0 = np.random.default_rng(0).standard_normal(spec.n_params).astype(np.float32)
    out = ch.hmc_step(1e-4, 3, p0=p0, log_u=float(np.log(0.5)))
    want = o.weight_step(spec, theta0, eta, X, Y, 1e-4, 3, p0, np.log(0.5), np.float64)
    assert abs(out["logp_new"] - want.logp_new) <= 4e-6 * abs(want.logp_new) and bool(out["accepted"]) == want.accepted
    ch.close()
    # in a group the chains beside the diverged one are what they are without it
    starts = np.stack([theta0, 0.5 * theta0, 0.25 * theta0]).astype(np.float32)
    runs = []
    for lr_mid in (R.F32(1e-2), None):
        grp = make(native, monkeypatch, spec, "layered", chains=3)
        grp.set_data(X, Y); grp.set_state(starts); grp.set_hypers(eta)
        if lr_mid is None:                  # chain 1 is thrown far out first: a start whose first check is already not finite
            far = starts.copy(); far[1] = 1e30
            grp.set_state(far)
        runs.append((grp.optimize(8, lr=R.F32(1e-2), check_every=1, keep="last"), grp.get_state()))
        grp.close()
    (a, tha), (b, thb) = runs
    assert [r["diverged"] for r in a] == [0, 0, 0] and [r["diverged"] for r in b] == [0, 1, 0]
    assert b[1]["steps_done"] == 0 and np.array_equal(thb[1], np.full(spec.n_params, 1e30, np.float32))
    for c in (0, 2):
        assert same(a[c], b[c]) and np.array_equal(tha[c], thb[c])


# ---------------------------------------------------------------- 7. objectives and weights
LIK_CASES = {
    "bernoulli": ([5, 16, 16, 1], 600, o.LIK_BERNOULLI, o.ACT_SIGMOID),
    "categorical": ([5, 16, 16, 4], 517, o.LIK_CATEGORICAL, o.ACT_NONE),
}


def lik_problem(kind):
    dims, n, lik, final = LIK_CASES[kind]
    if lik == o.LIK_BERNOULLI:
        spec, X, Y, theta, eta = o.synth_problem(dims, n, o.ACT_TANH, o.PRIOR_CAUCHY, lik)
    else:
        _s, X, Yr, theta, _e = o.synth_problem(dims, n, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN)
        spec = o.make_spec(dims, o.ACT_TANH, o.PRIOR_CAUCHY, lik, final)
        Y = np.eye(dims[-1], dtype=np.float32)[np.argmax(Yr, axis=1)]
        eta = o.default_hypers(spec)
    return spec, X, Y, theta, np.asarray(eta[:spec.n_hypers], np.float32)


def check_run(out, th, g, spec, theta0, eta, X, Y, steps, w=None, objective="posterior"):
    """a short run against the restatement in fp64: the trace to the project's 4e-6 value band, the last gradient to its per-tensor band,
    theta to 8 x the restatement's own fp32 gap"""
    tr64, th64, gs = R.run(spec, theta0, eta, X, Y, steps, dtype=np.float64, w=w, objective=objective)
    _t32, th32, _g = R.run(spec, theta0, eta, X, Y, steps, dtype=np.float32, w=w, objective=objective)
    assert np.all(np.abs(out["trace"] - tr64) <= 4e-6 * np.maximum(np.abs(tr64), 1.0)), (out["trace"], tr64)
    assert max(tensor_errs(spec, g, gs[-1], 1e-3)) <= 1e-4
    gap = np.abs(th32.astype(np.float64) - th64).max()
    assert np.abs(th.astype(np.float64) - th64).max() <= 8 * gap, (np.abs(th - th64).max(), gap)


def test_likelihood_objective_leaves_the_prior_out(native, monkeypatch):
    ch, spec, X, Y, theta0, eta = staged(native, monkeypatch, "fast3")
    out = ch.optimize(6, lr=R.LR, check_every=1, keep="last", objective="likelihood")
    th, st = ch.get_state(), ch.optim_state()
    _lp, _g, stat = ch.logp_grad(theta0, eta)
    ch.close()
    check_run(out, th, st["g"], spec, theta0, eta, X, Y, 6, objective="likelihood")
    lp, _ = o.target_log_prob_and_grad(spec, theta0, eta, X, Y, np.float64)
    assert abs(out["trace"][0] - lp) > 10 * 4e-6 * abs(lp)                  # (not the posterior: the priors are ten value bands away)
    # the data term as tbnn_logp_grad's statistic gives it: sum (y - f)^2 of the Gaussian likelihood
    s = float(eta[-1]) ** 2
    nel = X.shape[0] * spec.layers[-1].out_dim
    data = -0.5 * (2.0 * nel * np.log(s) + stat / (s * s) + nel * np.log(2.0 * np.pi))
    assert abs(out["trace"][0] - data) <= 4e-6 * abs(data)


def test_row_weights_enter_as_in_the_sampler(native, monkeypatch):
    spec, X, Y, theta0, eta = problem("layered")
    w = np.random.default_rng(7).uniform(0.0, 2.0, X.shape[0]).astype(np.float32)
    w[::9] = 0.0
    ch, *_ = staged(native, monkeypatch, "layered", w=w)
    assert "weighted" in ch.kernel_name
    out = ch.optimize(6, lr=R.LR, check_every=1, keep="last")
    th, st = ch.get_state(), ch.optim_state()
    ch.close()
    check_run(out, th, st["g"], spec, theta0, eta, X, Y, 6, w=w)


@pytest.mark.parametrize("kind", list(LIK_CASES))
def test_other_likelihoods(native, monkeypatch, kind):
    spec, X, Y, theta0, eta = lik_problem(kind)
    ch = make(native, monkeypatch, spec, "layered")
    ch.set_data(X, Y); ch.set_state(theta0); ch.set_hypers(eta)
    out = ch.optimize(6, lr=R.LR, check_every=1, keep="last")
    th, st = ch.get_state(), ch.optim_state()
    ch.set_state(theta0)
    assert same(ch.optimize(6, lr=R.LR, check_every=1, keep="last"), out) and np.array_equal(ch.get_state(), th)
    ch.close()
    check_run(out, th, st["g"], spec, theta0, eta, X, Y, 6)


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_handle_alone(native, monkeypatch):
    spec, X, Y, theta0, eta = problem("fast3")
    ch = make(native, monkeypatch, spec, "fast3")
    ch.set_state(theta0); ch.set_hypers(eta)
    with pytest.raises(native.TbnnError, match="set_data"):
        ch.optimize(1)
    with pytest.raises(native.TbnnError, match="tbnn_optimize has not been called"):
        ch.optim_state()
    ch.set_data(X, Y)
    ch.optimize(3, lr=R.LR, check_every=1, keep="last")
    before = (ch.get_state(), ch.optim_state(), ch.kernel_name)
    import ctypes as C
    cfg = native.OptimCfg(1e-3, 0.9, 0.999, 1e-8, 1, 0, 1, 1)
    outs = (native.OptimOut * 1)()
    assert native.lib.tbnn_optimize(ch._h, None, 1, 1, outs, None) < 0 and "null" in native.lib.tbnn_last_error().decode()
    assert native.lib.tbnn_optimize(ch._h, C.byref(cfg), 1, 1, None, None) < 0 and "null" in native.lib.tbnn_last_error().decode()
    bad = [dict(steps=-1), dict(check_every=0), dict(lr=0.0), dict(lr=-1.0), dict(lr=float("nan")), dict(lr=float("inf")), dict(epsilon=0.0),
           dict(epsilon=float("nan")), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(objective=7)]
    for kw in bad:
        kw = dict(dict(steps=1), **kw)
        with pytest.raises(native.TbnnError):
            ch.optimize(kw.pop("steps"), **kw)
    with pytest.raises(ValueError):
        ch.optimize(1, objective="evidence")
    with pytest.raises(ValueError):
        ch.optimize(1, keep="first")
    comm = native.Comm(ch, 1, 0, native.comm_unique_id())
    ch.set_row_shard(comm, X.shape[0])
    with pytest.raises(native.TbnnError, match="row-sharded"):
        ch.optimize(1)
    ch.set_row_shard(None)
    comm.close()
    after = (ch.get_state(), ch.optim_state(), ch.kernel_name)
    assert np.array_equal(before[0], after[0]) and before[2] == after[2] and before[1]["t"] == after[1]["t"] == 3
    assert all(np.array_equal(before[1][k], after[1][k]) for k in ("m", "v", "vhat", "g"))
    # and it still optimises: the run continues where it stood
    out = ch.optimize(2, lr=R.LR, check_every=1, keep="last", reset=False)
    assert out["diverged"] == 0 and ch.optim_state()["t"] == 5
    ch.close()


# ---------------------------------------------------------------- 9. the Python surface
def regression_net(n=400, nv=150):
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.network import network
    rng = np.random.default_rng(21)
    x = rng.uniform(-2, 2, n + nv)
    y = np.sin(2 * x) + 0.1 * rng.standard_normal(n + nv)
    net = network(np.float32, 1, x[:n].reshape(-1, 1), y[:n].reshape(-1, 1), x[n:].reshape(-1, 1), y[n:].reshape(-1, 1))
    dims = [1, 16, 16, 1]
    for i in range(3):
        net.add(DenseLayer(dims[i], dims[i + 1], seed=10 * i))
        if i < 2:
            net.add(Tanh())
    return net


def test_network_pretrain(native, monkeypatch):
    from tensorbnn_amd.likelihood import GaussianLikelihood
    monkeypatch.setenv("TBNN_REGISTERED", "0")               # (whatever libraries earlier modules registered: the layered family)
    net = regression_net()
    lik = GaussianLikelihood(sd=0.1)
    hypers0 = [h.copy() for h in net.hyperStates]
    hist = net.pretrain(lik, cycles=2, epochs=200, learningRate=0.01, patience=10, checkEvery=10, verbose=False)
    assert net._chain.kernel_name.startswith("layered<")
    mons = [b["monitor"] for b in hist["blocks"]]
    assert hist["monitor"] == "validation" and hist["best"] > hist["start"] and hist["best"] == max(mons)
    assert hist["blocks"][0]["lr"] == 0.01 and hist["steps"] == hist["blocks"][-1]["step"]
    assert len(net.hyperStates) == len(hypers0) and all(np.array_equal(a, b) for a, b in zip(net.hyperStates, hypers0))
    theta = net._theta()
    ch = net._chain
    assert np.array_equal(ch.get_state(), theta)
    assert ch.ensemble_loglik(theta[None, :], which=1, sd=0.1)[0][0] == hist["best"]
    # train() afterwards starts from them
    net.setupMCMC(stepSizeStart=1e-4, leapfrogStart=3, burnin=2, adapt=False)
    lp, _g, _s = ch.logp_grad(theta, np.concatenate(hypers0 + [np.float32([0.1 ** 0.5])]))
    recs = net.train(1, 1, lik, adjustHypers=False, verbose=False)
    assert recs[0]["main"]["logp_old"] == lp
    # patience 1 stops early; without validation rows the training objective is the monitor
    early = regression_net()
    h2 = early.pretrain(lik, cycles=3, epochs=500, learningRate=0.3, patience=1, checkEvery=5, verbose=False)
    assert h2["stopped_early"] and h2["steps"] < 1500
    early._chain.close(); net._chain.close()
    from tensorbnn_amd.network import network
    noval = regression_net()
    nv = network(np.float32, 1, noval.trainX, noval.trainY, np.zeros((0, 1), np.float32), np.zeros((0, 1), np.float32))
    for layer in noval.layers:
        nv.add(layer)
    h3 = nv.pretrain(lik, cycles=1, epochs=50, verbose=False)
    assert h3["monitor"] == "training" and h3["best"] > h3["start"] and h3["best"] == max(b["objective"] for b in h3["blocks"])
    nv._chain.close()


def test_train_basic_helpers(native, monkeypatch, tmp_path):
    import tensorbnn_amd
    monkeypatch.setenv("TBNN_REGISTERED", "0")
    rng = np.random.default_rng(5)
    X = rng.standard_normal((600, 3)).astype(np.float32)
    yr = (np.sin(X[:, :1]) + 0.5 * X[:, 1:2] * X[:, 2:3]).astype(np.float32)
    w, b, act = tensorbnn_amd.trainBasicRegression(2, 3, 1, 12, 2, 150, 0, X[:450], yr[:450], X[450:], yr[450:], str(tmp_path / "reg"))
    assert [x.shape for x in w] == [(12, 3), (12, 12), (1, 12)] and [x.shape for x in b] == [(12, 1), (12, 1), (1, 1)] and act == []
    saved = np.load(str(tmp_path / "reg.npz"))
    assert np.array_equal(saved["weights1"], w[1]) and np.array_equal(saved["biases2"], b[2])

    def mlp(Xv, w, b, last=lambda z: z):
        a = Xv.T.astype(np.float64)
        for i, (W, B) in enumerate(zip(w, b)):
            a = W.astype(np.float64) @ a + B
            a = np.maximum(a, 0) if i < len(w) - 1 else last(a)
        return a.T
    from tensorbnn_amd.BNN_functions import _glorot
    w0 = [_glorot(i, *d) for i, d in enumerate([(3, 12), (12, 12), (12, 1)])]
    b0 = [np.zeros((x.shape[0], 1)) for x in w0]
    mse = lambda ws, bs: float(np.mean((mlp(X[450:], ws, bs) - yr[450:]) ** 2))
    assert mse(w, b) < mse(w0, b0), (mse(w, b), mse(w0, b0))
    yc = (yr > np.median(yr)).astype(np.float32)
    w, b, act = tensorbnn_amd.trainBasicClassification(2, 3, 1, 12, 2, 150, 0, X[:450], yc[:450], X[450:], yc[450:], str(tmp_path / "cls"))
    assert [x.shape for x in w] == [(12, 3), (12, 12), (1, 12)] and act == []
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))

    def bce(ws, bs):
        p = np.clip(mlp(X[450:], ws, bs, sig), 1e-8, 1 - 1e-7)
        return float(-np.mean(yc[450:] * np.log(p) + (1 - yc[450:]) * np.log1p(-p)))
    assert bce(w, b) < bce(w0, b0), (bce(w, b), bce(w0, b0))
