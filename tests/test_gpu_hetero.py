"""GPU: HeteroscedasticGaussianLikelihood (TBNN_LIK_HETERO_GAUSSIAN) -- a 2-output network predicts the mean f and the log-sd g of each
row, log p = -1/2 log(2 pi) - gc - 1/2 (y - f)^2 exp(-2 gc), gc = g clipped to +-log(1e8), ONE term per row -- on every kernel family that
takes a 2-output network: the narrow fast3 and fast kernels and their one-launch trajectory kernel, mid, tall and wide (the VALU last
layer), each likelihood path of the layered family (k_lay_tail, k_lay_last, k_lay_lik) and the generic kernel.  Against the oracle in fp64
(the cases are tests/hetero_ref.py's): the value with its constant, the gradient per tensor, the forward outputs, an injected weight
transition with both decisions (log u placed on either side of the reference's log accept ratio, two bands away), a hyper transition, every
launch repeated bit for bit.  Then: the clip, row weights, refusals, target padding, the device metrics, trainChains against solo runs,
pre-training, a row-sharded chain on the stub collective library, and an end-to-end fit on data whose noise grows 10x over the inputs
against the fixed-sd Gaussian fit.

Bands: the project's, as tests/test_gpu_negbin.py has them -- value 4e-6 relative, gradient 1e-4 of each tensor's largest entry (floor
1e-3), log accept ratio 2e-2 + 1e-4 |lar| + 4e-7 |logp|.  tests/test_hetero_host.py (CPU arithmetic only) shows that the kernel's own
formula in fp32 stays inside HALF of them at every case here, so no case has a band of its own.

The clip (test_clip): with the last bias of output 1 at +-25 every row's g lies beyond +-log(1e8) = +-18.42; the value is finite and the
reference's, and dL/dg is 0 on every row, so the data term's part of that bias' gradient is exactly 0 and what tbnn_logp_grad returns there
is the prior's own gradient (to fp32 rounding: 4 ulp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hetero_ref as hr
import optim_ref as R
import tbnn_oracle as o
from tensor_checks import layers_of, tensor_errs
from test_gpu_freerun import SEED

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FUSED = {"fast3": "", "fast": "fast3", "mid": "fast3,fast,tall,wide", "tall": "fast3,fast,mid,wide", "wide": "fast3,fast,mid,tall"}
CASES = {k: v for k, v in hr.CASES.items() if v[4] != "traj"}
NET = [1, 16, 16, 2]                                              # the network(...) of the trainChains and end-to-end tests (tanh)
LIK = o.LIK_HETERO_GAUSSIAN
LAY_KERNEL = {"lay_last": "last", "lay_separate": "lik", "lay_tail": "tail"}


def lay_kernel(dims, n, env):
    """which likelihood kernel the layered family runs for `dims` over n rows: lay_plan_shape / lay_plan_rows of csrc/kernels_layered.hpp
    restated (the kernel name carries the dims alone) -- "tail": k_lay_tail, "last": k_lay_last, "lik": k_lay_lik"""
    cdiv = lambda a, b: (a + b - 1) // b
    nl = len(dims) - 1
    TK = [cdiv(dims[l] + 1, 16) for l in range(nl)]
    TM = [cdiv(dims[l + 1], 16) for l in range(nl)]
    TO = [TK[l + 1] if l + 1 < nl else TM[l] for l in range(nl)]
    l0 = nl
    while l0 >= 1 and TK[l0 - 1] <= 4 and TO[l0 - 1] <= 4 and TM[l0 - 1] <= 4:
        l0 -= 1
    if env.get("TBNN_LAY_TAIL") == "0":
        l0 = nl
    last_ok = l0 == nl and nl >= 2 and TM[nl - 1] == 1 and TK[nl - 1] <= 8 and TM[nl - 2] <= 8 and env.get("TBNN_LAY_LAST") != "0"
    small = cdiv(n, 16) < 4 * 512                                     # (PSTAT_CAP workgroups of four waves)
    tail = l0 < nl and small
    return "tail" if tail else "last" if (last_ok and small) else "lik"


def job(spec, lik=LIK, skip="", weighted=False):
    j = {"layers": [list(l) for l in layers_of(spec)], "likelihood": lik, "skip": skip, "flags": ""}
    if weighted:
        j["weighted"] = True
    return j


def jit_jobs():
    """the run-time instantiations this module asks for (jit.prebuild's job format)"""
    jobs = []
    for dims, _n, act, prior, fam, _env in hr.CASES.values():
        if fam in FUSED:
            jobs.append(job(o.make_spec(dims, act, prior, LIK, o.ACT_NONE), skip=FUSED[fam]))
        elif fam == "traj":
            jobs.append(job(o.make_spec(dims, act, prior, LIK, o.ACT_NONE)))
    jobs.append(job(o.make_spec(*[hr.CASES["fast3"][i] for i in (0, 2, 3)], LIK, o.ACT_NONE), weighted=True))
    jobs.append(job(o.make_spec(NET, o.ACT_TANH, o.PRIOR_CAUCHY, LIK, o.ACT_NONE)))
    # the fixed-sd fit of the end-to-end test (1-16-16-1) and the predictors' forward chains (fixed-sd Gaussian handles)
    jobs.append(job(o.make_spec([1, 16, 16, 1], o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_FIXED_GAUSSIAN, o.ACT_NONE), lik=o.LIK_FIXED_GAUSSIAN))
    jobs.append(job(o.make_spec(NET, o.ACT_TANH, o.PRIOR_CAUCHY, LIK, o.ACT_NONE), lik=o.LIK_FIXED_GAUSSIAN))
    return [j for i, j in enumerate(jobs) if j not in jobs[:i]]


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """compile this module's run-time shapes side by side before any test touches the GPU (cached: a second run compiles nothing)"""
    from tensorbnn_amd import jit
    jobs = jit_jobs()
    assert len(jobs) <= 16
    assert jit.prebuild(jobs, processes=min(16, len(jobs))) == len(jobs)


def gaps(spec, lp, g, lp64, g64):
    """(value error / max(|lp64|, 1), per tensor: gradient error / max(|g64|_inf, 1e-3))"""
    return abs(lp - lp64) / max(abs(lp64), 1.0), tensor_errs(spec, g, g64, 1e-3)


def check_value_gradient(tag, lp, g, spec, ref64):
    ev, eg = gaps(spec, lp, g, *ref64)
    print(f"[hetero] {tag}: logp {lp:.9g} (fp64 {ref64[0]:.9g}) err {ev:.3e} of band 4e-6; gradient err max {max(eg):.3e} of band 1e-4")
    assert np.isfinite(lp) and np.all(np.isfinite(g))
    assert ev <= 4e-6, (tag, lp, ref64[0])
    assert max(eg) <= 1e-4, (tag, eg)


def make_chain(native, monkeypatch, name, spec, **kw):
    fam, env = hr.CASES[name][4], hr.CASES[name][5]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(likelihood=LIK, **kw)
    if fam in FUSED:
        monkeypatch.setenv("TBNN_JIT_SKIP", FUSED[fam])
        ch = native.Chain(layers_of(spec), jit=True, **kw)
        assert ch.kernel_name.startswith(f"jit-{fam}<") and ",hetero-gaussian;" in ch.kernel_name, ch.kernel_name
    elif fam == "layered":
        monkeypatch.setenv("TBNN_TALL", "0")
        monkeypatch.setenv("TBNN_REGISTERED", "0")
        ch = native.Chain(layers_of(spec), jit=False, **kw)
        assert ch.kernel_name.startswith("layered<"), ch.kernel_name
    else:
        ch = native.Chain(layers_of(spec), kernel=native.KERNEL_GENERIC, **kw)
        assert ch.kernel_name == "generic", ch.kernel_name
    assert ch.H == 4 * len(spec.layers)
    return ch


@pytest.mark.parametrize("name", list(CASES))
def test_value_gradient_forward(native, monkeypatch, name):
    spec, X, Y, theta, eta = hr.problem(name)
    ch = make_chain(native, monkeypatch, name, spec)
    if name in LAY_KERNEL:
        assert lay_kernel(hr.CASES[name][0], X.shape[0], hr.CASES[name][5]) == LAY_KERNEL[name]
    ch.set_data(X, Y)
    lp, g, st = ch.logp_grad(theta, eta)
    for _ in range(2):
        lp2, g2, st2 = ch.logp_grad(theta, eta)
        assert lp2 == lp and st2 == st and np.array_equal(g, g2)
    m = min(500, X.shape[0])
    f = ch.forward(X[:m], theta)
    assert np.array_equal(f, ch.forward(X[:m], theta))
    # [n, 2] targets are taken as they are, and column 1 is not read: any value there, the same bits
    Y2 = np.stack([Y, np.full_like(Y, 1e30)], axis=1)
    ch.set_data(X, Y2)
    lp3, g3, st3 = ch.logp_grad(theta, eta)
    assert lp3 == lp and st3 == st and np.array_equal(g, g3)
    ch.close()
    check_value_gradient(name, lp, g, spec, hr.ref64(name))
    # stat is the data term with its constant (as Poisson's), and logp minus it the priors
    f64 = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    data64 = float(o.log_likelihood(spec, eta, f64, Y, np.float64))
    assert abs(st - data64) <= 4e-6 * abs(data64), (st, data64)
    prior = float(hr.ref64(name)[0] - data64)
    assert abs((lp - st) - prior) <= 4e-6 * max(abs(lp), 1.0)
    assert f.shape == (2, m)
    assert np.abs(f - f64[:, :m]).max() <= 1e-4 * max(1.0, np.abs(f64).max())


@pytest.mark.parametrize("name", list(CASES))
def test_transitions(native, monkeypatch, name):
    spec, X, Y, theta, eta = hr.problem(name)
    rng = np.random.default_rng(4)
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    ch = make_chain(native, monkeypatch, name, spec, seed=SEED, chain_id=2)
    ch.set_data(X, Y)
    lp64 = hr.ref64(name)[0]
    eps = hr.step_size(name)
    ref = o.weight_step(spec, theta, eta, X, Y, eps, 4, p0, -1e30, np.float64)
    tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
    # log u on either side of the reference's log accept ratio, two bands away: the kernel's rounding cannot flip the decision
    for log_u, accept in ((ref.log_accept_ratio - 2 * tol, True), (ref.log_accept_ratio + 2 * tol, False)):
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hmc_step(eps, 4, p0=p0, log_u=log_u)
        print(f"[hetero] {name}: lar {out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g}, band {tol:.3g}), logp {lp64:.6g}")
        assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= tol
        assert bool(out["accepted"]) == accept
        assert abs(out["logp_old"] - lp64) <= 4e-6 * max(abs(lp64), 1.0)
        assert abs(out["logp_new"] - ref.logp_new) <= 4e-6 * max(abs(ref.logp_new), 1.0)
        want = ref.theta_proposed if accept else theta
        assert np.abs(ch.get_state() - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
        again = ch.set_state(theta) or ch.hmc_step(eps, 4, p0=p0, log_u=log_u)
        assert again["log_accept_ratio"] == out["log_accept_ratio"] and again["logp_new"] == out["logp_new"]
    # the hyper transition: the layer priors only (no likelihood hyper, no data term)
    ph = rng.standard_normal(spec.n_hypers).astype(np.float32)
    ch.set_state(theta); ch.set_hypers(eta)
    ch.logp_grad(theta, eta)
    out = ch.hyper_step(1e-4, 9, p0=ph, log_u=-1e30)
    ref = o.hyper_step(spec, eta, theta, X, Y, 1e-4, 9, ph, -1e30, np.float64)
    assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= 2e-2 + 1e-3 * abs(ref.log_accept_ratio)
    assert np.allclose(ch.get_hypers(), ref.theta, rtol=1e-4, atol=1e-5)
    # after the accepted hyper transition the cached gradient is refreshed for the new priors: the next weight step starts from it
    eta2 = ch.get_hypers()
    lp_new, g_new, _ = ch.logp_grad(theta, eta2)
    check_value_gradient(name + " after the hyper step", lp_new, g_new, spec, o.target_log_prob_and_grad(spec, theta, eta2, X, Y, np.float64))
    ch.close()


def test_trajectory_kernel(native, monkeypatch):
    """a small narrow problem takes the one-launch trajectory kernel; the traced run of the same transition (per-step kernels) agrees with
    fp64 step by step"""
    spec, X, Y, theta, eta = hr.problem("traj")
    monkeypatch.setenv("TBNN_TRAJ", "1")
    monkeypatch.setenv("TBNN_JIT_SKIP", "")
    ch = native.Chain(layers_of(spec), likelihood=LIK, jit=True, seed=SEED)
    assert ch.kernel_name.startswith("jit-fast3<") and ",hetero-gaussian;" in ch.kernel_name, ch.kernel_name
    ch.set_data(X, Y)
    lp, g, _ = ch.logp_grad(theta, eta)
    check_value_gradient("traj", lp, g, spec, hr.ref64("traj"))
    p0 = np.random.default_rng(5).standard_normal(spec.n_params).astype(np.float32)
    lp64 = hr.ref64("traj")[0]
    eps = hr.step_size("traj")
    for L in (1, 9):
        ref = o.weight_step(spec, theta, eta, X, Y, eps, L, p0, -1e30, np.float64)
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hmc_step(eps, L, p0=p0, log_u=-1e30)
        assert ch.last_transition_path == "trajectory"
        tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
        print(f"[hetero] trajectory L={L}: lar {out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g})")
        assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= tol
        assert bool(out["accepted"]) == ref.accepted
        assert abs(out["logp_new"] - ref.logp_new) <= 4e-6 * max(abs(ref.logp_new), 1.0)
        np.testing.assert_allclose(ch.get_state(), ref.theta, rtol=2e-5, atol=2e-6)
        ch.set_state(theta); ch.set_hypers(eta)
        again = ch.hmc_step(eps, L, p0=p0, log_u=-1e30)
        assert again["log_accept_ratio"] == out["log_accept_ratio"] and ch.last_transition_path == "trajectory"
        ch.set_state(theta); ch.set_hypers(eta)
        rej = ch.hmc_step(eps, L, p0=p0, log_u=ref.log_accept_ratio + 2 * tol)           # the other decision
        assert rej["accepted"] == 0 and np.array_equal(ch.get_state(), theta)
        ch.set_state(theta); ch.set_hypers(eta)
        traced = ch.hmc_step(eps, L, p0=p0, log_u=-1e30, trace=True)
        assert ch.last_transition_path == "per-step"
        tr, tr64 = np.asarray(traced["trace_logp"]), np.asarray(ref.trace_logp)
        assert tr.shape == tr64.shape and np.max(np.abs(tr - tr64) / np.maximum(np.abs(tr64), 1.0)) <= 4e-6
        assert abs(traced["log_accept_ratio"] - ref.log_accept_ratio) <= tol
    ch.close()


@pytest.mark.parametrize("name", hr.CLIP_CASES)
@pytest.mark.parametrize("bias", [25.0, -25.0])
def test_clip(native, monkeypatch, name, bias):
    """g beyond +-log(1e8) on every row: the value is the reference's and finite; the data term adds exactly nothing to the gradient of
    the bias that moved g there, so the entry returned is the prior's own gradient"""
    spec, X, Y, theta, eta = hr.problem(name)
    j = hr.last_bias_index(spec, 1)
    th = theta.copy()
    th[j] = bias
    g64_out = o.forward(spec, th.astype(np.float64), X.astype(np.float64), np.float64)[1]
    assert np.all(np.abs(g64_out) > o.LOG_CLIP + 0.5)
    ref = o.target_log_prob_and_grad(spec, th, eta, X, Y, np.float64)
    ch = make_chain(native, monkeypatch, name, spec)
    ch.set_data(X, Y)
    lp, g, _st = ch.logp_grad(th, eta)
    ch.close()
    check_value_gradient(f"{name} clip {bias:+g}", lp, g, spec, ref)
    pg = o.prior_grad(spec.layers[-1], eta[-4:].astype(np.float64), *o.unflatten(spec, th.astype(np.float64))[-1], np.float64)[1][1, 0]
    assert ref[1][j] == pg                                                # (the reference: no data part either)
    print(f"[hetero] {name} clip {bias:+g}: gradient of the bias {g[j]:.9g}, the prior's own {pg:.9g}")
    assert abs(float(g[j]) - pg) <= 4 * np.spacing(np.float32(abs(pg))), (g[j], pg)


@pytest.mark.parametrize("name", ["fast3", "lay_last"])
def test_row_weights(native, monkeypatch, name):
    spec, X, Y, theta, eta = hr.problem(name)
    n = min(600, X.shape[0])
    X, Y = X[:n], Y[:n]
    w = np.random.default_rng(21).integers(0, 4, n).astype(np.float32)
    vg = lambda Xs, Ys, ws=None: o.target_log_prob_and_grad(spec, theta, eta, Xs, Ys, np.float64, ws)
    ch = make_chain(native, monkeypatch, name, spec)
    ch.set_data(X, Y)
    plain = ch.logp_grad(theta, eta)
    # a weight of 1 everywhere: the unweighted bits
    ch.set_row_weights(np.ones(n, np.float32))
    if hr.CASES[name][4] in FUSED:
        assert ",hetero-gaussian,weighted;" in ch.kernel_name, ch.kernel_name
    ones = ch.logp_grad(theta, eta)
    assert ones[0] == plain[0] and ones[2] == plain[2] and np.array_equal(ones[1], plain[1])
    check_value_gradient(name + " weight 1", ones[0], ones[1], spec, vg(X, Y))
    # integer weights: the rows duplicated
    ch.set_row_weights(w)
    lp, g, st = ch.logp_grad(theta, eta)
    check_value_gradient(name + " weighted", lp, g, spec, vg(X, Y, w))
    idx = np.repeat(np.arange(n), w.astype(int))
    ch.set_row_weights(None)
    ch.set_data(X[idx], Y[idx])
    dup = ch.logp_grad(theta, eta)
    check_value_gradient(name + " duplicated", dup[0], dup[1], spec, vg(X[idx], Y[idx]))
    ev, eg = gaps(spec, lp, g, dup[0], dup[1].astype(np.float64))
    print(f"[hetero] {name}: weights vs duplicated rows: value {ev:.3e}, gradient {max(eg):.3e}")
    assert ev <= 4e-6 and max(eg) <= 1e-4, (ev, eg)
    # clearing the weights brings the unweighted bits back
    ch.set_data(X, Y); ch.set_row_weights(w); ch.set_row_weights(None)
    back = ch.logp_grad(theta, eta)
    assert back[0] == plain[0] and np.array_equal(back[1], plain[1])
    ch.close()


def test_refusals_padding_and_metrics(native, monkeypatch):
    spec, X, Y, theta, eta = hr.problem("generic")
    layers = layers_of(spec)
    for d_out in (1, 3):
        bad = layers[:-1] + [(layers[-1][0], d_out) + layers[-1][2:]]
        with pytest.raises(native.TbnnError, match="needs exactly 2 outputs: mean and log-sd"):
            native.Chain(bad, likelihood=LIK, kernel=native.KERNEL_GENERIC)
        with pytest.raises(native.TbnnError, match="needs exactly 2 outputs: mean and log-sd"):
            native.ChainGroup(bad, 2, likelihood=LIK, kernel=native.KERNEL_GENERIC)
    with pytest.raises(native.TbnnError, match="no activation"):
        native.Chain(layers[:-1] + [layers[-1][:2] + (native.ACT_TANH,) + layers[-1][3:]], likelihood=LIK, kernel=native.KERNEL_GENERIC)
    for unknown in (4, 6, 7, 9, 11):
        with pytest.raises(native.TbnnError, match="unknown likelihood"):
            native.Chain(layers, likelihood=unknown, kernel=native.KERNEL_GENERIC)
    # fixed_sd and lik_df are not read
    ch = native.Chain(layers, likelihood=LIK, kernel=native.KERNEL_GENERIC, fixed_sd=0.0, lik_df=float("nan"))
    n = X.shape[0]
    ch.set_data(X, Y)
    a = ch.logp_grad(theta, eta)
    ch.set_data(X, Y.reshape(n, 1))
    b = ch.logp_grad(theta, eta)
    ch.set_data(X, np.stack([Y, -Y], axis=1))
    c = ch.logp_grad(theta, eta)
    assert a[0] == b[0] == c[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])
    check_value_gradient("generic, padded targets", a[0], a[1], spec, hr.ref64("generic"))
    # tbnn_metrics: output 0 against target column 0 alone (the log-sd does not enter the squared error)
    ch.set_validation(X[:100], Y[:100])
    f = ch.forward(X, theta).astype(np.float64)
    for which, rows in ((0, n), (1, 100)):
        mse = ch.metrics(which, theta)[0]
        want = float(np.mean((f[0, :rows] - Y[:rows].astype(np.float64)) ** 2))
        assert abs(mse - want) <= 1e-5 * want, (which, mse, want)
    # the ensemble log-likelihood on a 1-output handle is refused
    one = native.Chain(layers[:-1] + [(layers[-1][0], 1) + layers[-1][2:]], likelihood=o.LIK_FIXED_GAUSSIAN, fixed_sd=1.0, kernel=native.KERNEL_GENERIC)
    th1 = np.zeros((2, one.P), np.float32)
    with pytest.raises(native.TbnnError, match="needs exactly 2 outputs"):
        one.ensemble_loglik(th1, Y=Y[:64].reshape(-1, 1), X=X[:64], likelihood=LIK)
    with pytest.raises(native.TbnnError, match="needs exactly 2 outputs"):
        one.ensemble_loo(th1, Y=Y[:64].reshape(-1, 1), X=X[:64], likelihood=LIK)
    one.close()
    ch.close()


# ---------------------------------------------------------------------------------------------------------------------- pre-training
def test_pretraining_against_the_restatement(native, monkeypatch):
    """Chain.optimize for a few steps against the Adam / AMSGrad restatement of tests/optim_ref.py driven by the oracle's gradient: the
    checked objectives to the value band, the last step's gradient to the gradient band, theta to 8 x the restatement's own fp32 gap"""
    name, steps = "fast3_two_outputs", 6
    spec, X, Y, theta0, eta = hr.problem(name)

    def run(dtype):
        dt = dtype
        theta = np.asarray(theta0, dtype=dt)
        m = v = vhat = np.zeros_like(theta)
        trace, g = [], None
        for i in range(steps):
            lp, g = o.target_log_prob_and_grad(spec, theta, eta, X, Y, dt)
            trace.append(float(lp))
            theta, m, v, vhat = R.adam_step(theta, g, m, v, vhat, i + 1, R.LR, dtype=dt)
        trace.append(float(o.target_log_prob_and_grad(spec, theta, eta, X, Y, dt)[0]))
        return np.asarray(trace), theta, g

    ch = make_chain(native, monkeypatch, name, spec)
    ch.set_data(X, Y); ch.set_state(theta0); ch.set_hypers(eta)
    out = ch.optimize(steps, lr=R.LR, check_every=1, keep="last")
    th, st = ch.get_state(), ch.optim_state()
    ch.set_state(theta0)
    again = ch.optimize(steps, lr=R.LR, check_every=1, keep="last")
    assert np.array_equal(again["trace"], out["trace"]) and np.array_equal(ch.get_state(), th)
    ch.close()
    tr64, th64, g64 = run(np.float64)
    _tr32, th32, _g32 = run(np.float32)
    print(f"[hetero] optimize: trace {out['trace'][0]:.6f} -> {out['trace'][-1]:.6f} (fp64 {tr64[0]:.6f} -> {tr64[-1]:.6f})")
    assert out["steps_done"] == steps and out["diverged"] == 0 and tr64[-1] > tr64[0]
    assert np.all(np.abs(out["trace"] - tr64) <= 4e-6 * np.maximum(np.abs(tr64), 1.0)), (out["trace"], tr64)
    assert max(tensor_errs(spec, st["g"], g64, 1e-3)) <= 1e-4
    gap = np.abs(th32.astype(np.float64) - th64).max()
    assert np.abs(th.astype(np.float64) - th64).max() <= 8 * gap, (np.abs(th - th64).max(), gap)


# ---------------------------------------------------------------------------------------------------------------------- row-sharded chain
def test_row_shard_two_ranks(tmp_path, native, monkeypatch):
    """world 2 on the stub collective library (tests/stubccl/worker_hetero.py: two fresh child processes, each under its own time limit):
    the statistic is all-reduced and the constant counts n_total rows, so the sharded chain takes the unsharded chain's decisions and
    reaches its state, within the sharding band of tests/test_gpu_multirank.py"""
    from conftest import wait_gpu_quiet
    from test_gpu_multirank import build_stub
    sys.path.insert(0, os.path.join(HERE, "stubccl"))
    import worker_hetero as ws
    wait_gpu_quiet()
    env = dict(os.environ, TBNN_RCCL_LIB=build_stub(), TBNN_JIT="0", TBNN_PREBUILD_JIT="0")
    idfile = str(tmp_path / "shard.id")
    procs = []
    for rk in range(2):
        out = str(tmp_path / f"shard_{rk}.npz")
        procs.append((out, subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "stubccl", "worker_hetero.py"), str(rk), "2", idfile, out],
                                            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    ranks = []
    for out, p in procs:
        try:
            log, _ = p.communicate(timeout=330)
        except subprocess.TimeoutExpired:
            for _, q in procs:
                q.kill()
            raise
        assert p.returncode == 0, log[-3000:]
        ranks.append(np.load(out))
    for name in ws.SHAPES:
        spec, X, Y, theta, eta = ws.problem(name)
        ref = ws.chain_of(name, spec)
        ref.set_data(X, Y); ref.set_state(theta); ref.set_hypers(eta)
        lp0, g0, st0 = ref.logp_grad(theta, eta)
        p0 = np.random.default_rng(5).standard_normal(spec.n_params).astype(np.float32)
        outs = [ref.hmc_step(1e-5, 4, p0=p0, log_u=-1e30, trace=True), ref.hmc_step(1e-5, 3)]
        th_ref = ref.get_state()
        n = X.shape[0]
        rows = [tuple(rk[name + "_rows"]) for rk in ranks]
        assert rows[0][0] == 0 and rows[0][1] == rows[1][0] and rows[1][1] == n, rows
        for rk in ranks:
            assert str(rk[name + "_kernel"]) == ref.kernel_name
            assert abs(float(rk[name + "_lp"]) - lp0) <= 1e-7 * abs(lp0) + 1e-6
            assert abs(float(rk[name + "_st"]) - st0) <= 1e-9 * abs(st0)
            np.testing.assert_allclose(rk[name + "_g"], g0, rtol=0, atol=4e-6 * np.abs(g0).max())
            np.testing.assert_allclose(rk[name + "_trace"], outs[0]["trace_logp"], rtol=1e-7, atol=1e-5)
            for k in range(2):
                assert abs(rk[name + "_lar"][k] - outs[k]["log_accept_ratio"]) <= 2e-3 + 1e-5 * abs(outs[k]["log_accept_ratio"])
                assert rk[name + "_acc"][k] == outs[k]["accepted"]
            np.testing.assert_allclose(rk[name + "_theta"], th_ref, rtol=0, atol=2e-6 * max(1.0, np.abs(th_ref).max()))
        np.testing.assert_array_equal(ranks[0][name + "_theta"], ranks[1][name + "_theta"])       # every rank took the same decisions
        np.testing.assert_array_equal(ranks[0][name + "_g"], ranks[1][name + "_g"])
        assert float(ranks[0][name + "_lp"]) == float(ranks[1][name + "_lp"])
        check_value_gradient("shard " + name, float(ranks[0][name + "_lp"]), ranks[0][name + "_g"], spec,
                             o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64))
        ref.close()


# ---------------------------------------------------------------------------------------------------------------------- network / train
def noise_sd(x):
    """the noise sd rises 10x from the left end of the inputs to the right end: 0.05 at x = -2, 0.5 at x = 2"""
    return 0.05 * 10.0 ** ((x + 2.0) / 4.0)


def hetero_data(n, seed):
    """x ~ U(-2, 2), y = sin(1.5 x) + N(0, noise_sd(x)^2)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, 1)).astype(np.float32)
    x = X[:, 0].astype(np.float64)
    return X, (np.sin(1.5 * x) + noise_sd(x) * rng.standard_normal(n)).astype(np.float32)


def make_net(X, Y, Xv, Yv, d_out=2, chain_id=0, **kw):
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.network import network
    net = network(np.float32, 1, X, Y, Xv, Yv, chain_id=chain_id, **kw)
    net.add(DenseLayer(1, 16, seed=1000)); net.add(Tanh())
    net.add(DenseLayer(16, 16, seed=2000)); net.add(Tanh())
    net.add(DenseLayer(16, d_out, seed=3000))
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    return net


def test_train_chains_equal_solo_runs(tmp_path, monkeypatch, native):
    from tensorbnn_amd.likelihood import HeteroscedasticGaussianLikelihood
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, Y = hetero_data(400, 1)
    Xv, Yv = hetero_data(200, 2)
    C, EPOCHS = 2, 14
    grp_net = make_net(X, Y, Xv, Yv)
    rec = grp_net.trainChains(C, EPOCHS, 4, HeteroscedasticGaussianLikelihood(), adjustHypers=True, folderName="multi", networksPerFile=2)
    assert len(rec) == EPOCHS and all(len(rc["main"]) == C for rc in rec)
    for c in range(C):
        net = make_net(X, Y, Xv, Yv, chain_id=c)
        solo = net.train(EPOCHS, 4, HeteroscedasticGaussianLikelihood(), adjustHypers=True, folderName="solo%d" % c, networksPerFile=2, verbose=False)
        assert net._chain.kernel_name.startswith("jit-fast3<") and "hetero-gaussian" in net._chain.kernel_name, net._chain.kernel_name
        for rg, rs in zip(rec, solo):
            assert rg["eps"][c] == rs["eps"] and rg["L"][c] == rs["L"]
            for k in ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new", "sjd"):
                # (the same bits: while the step size adapts a proposal may run out of the fp32 range -- r^2 u = inf, a NaN log-probability,
                # rejected -- in the group as in the solo run)
                a, b = rg["main"][c][k], rs["main"][k]
                assert a == b or (a != a and b != b), (c, rg["iter"], k, a, b)
            assert rg["hyper"][c]["log_accept_ratio"] == rs["hyper"]["log_accept_ratio"]
            assert rg["hyper_step_size"][c] == rs["hyper_step_size"]


def test_fit_on_heteroscedastic_data(tmp_path, monkeypatch, native):
    """[1, 16, 16, 2] on 400 rows of y = sin(1.5 x) + noise whose sd rises 10x from left to right, pretrain then train under
    HeteroscedasticGaussianLikelihood; beside it [1, 16, 16, 1] under FixedGaussianLikelihood(sd = the data's overall noise sd) on the same
    rows, trained the same way.  Asserted: the posterior-mean exp(g) over the left third of the inputs is below that over the right third,
    and on 300 held-out rows predictor.compareLoo favours the new model by more than 2 se_diff.  Printed: elpd_diff, se_diff and the coverage
    of each fit's 90 % predictive interval per third of the input range (README.md records them)."""
    from tensorbnn_amd.likelihood import FixedGaussianLikelihood, HeteroscedasticGaussianLikelihood
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, Y = hetero_data(400, 1)
    Xv, Yv = hetero_data(200, 2)
    Xh, Yh = hetero_data(300, 3)
    sd_all = float(np.sqrt(np.mean(noise_sd(X[:, 0].astype(np.float64)) ** 2)))
    loos = {}
    for tag, lik, d_out in (("hetero", HeteroscedasticGaussianLikelihood(), 2), ("fixed", FixedGaussianLikelihood(sd=sd_all), 1)):
        net = make_net(X, Y, Xv, Yv, d_out=d_out)
        hist = net.pretrain(lik, cycles=2, epochs=400, learningRate=0.01, verbose=False)
        net.train(70, 4, lik, folderName=tag, networksPerFile=1, verbose=False)
        assert ("hetero-gaussian" in net._chain.kernel_name) == (tag == "hetero"), net._chain.kernel_name
        p = predictor(str(tmp_path / tag) + "/", likelihood=lik)
        loos[tag] = p.loo(Xh, Yh)
        assert np.isfinite(loos[tag]["elpd_loo"])
        lower, _median, upper = p.predictiveInterval(Xh, level=0.9)
        assert lower.shape == upper.shape == (1, len(Xh)) and np.all(lower < upper)
        xh, yh = Xh[:, 0], Yh.astype(np.float64)
        inside = (yh >= lower[0]) & (yh <= upper[0])
        thirds = [float(inside[(xh >= a) & (xh < b)].mean()) for a, b in ((-2.0, -2.0 / 3.0), (-2.0 / 3.0, 2.0 / 3.0), (2.0 / 3.0, 2.01))]
        print(f"[hetero] {tag} fit: {p.numNetworks} networks after {hist['steps']} pre-training steps; elpd_loo {loos[tag]['elpd_loo']:.1f} "
              f"(se {loos[tag]['se']:.1f}) on {len(Xh)} held-out rows; 90 % predictive interval covers {float(inside.mean()):.3f} "
              f"(left / middle / right third of the inputs: {thirds[0]:.3f} / {thirds[1]:.3f} / {thirds[2]:.3f})")
        if tag == "hetero":
            f = np.asarray(p.predict(Xh), dtype=np.float64)                                    # [networks, 2, rows]
            s = np.exp(f[:, 1, :]).mean(axis=0)
            x = Xh[:, 0]
            left, right = float(s[x < -2.0 / 3.0].mean()), float(s[x > 2.0 / 3.0].mean())
            print(f"[hetero] posterior-mean exp(g): left third {left:.3f}, right third {right:.3f} "
                  f"(the data's: {noise_sd(-4.0 / 3.0):.3f}, {noise_sd(4.0 / 3.0):.3f})")
            assert left < right
    cmp_ = predictor.compareLoo(loos["hetero"], loos["fixed"])
    print(f"[hetero] compareLoo(hetero, fixed): elpd_diff {cmp_['elpd_diff']:.1f}, se_diff {cmp_['se_diff']:.1f}")
    assert cmp_["elpd_diff"] > 2.0 * cmp_["se_diff"]
