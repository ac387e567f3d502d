"""GPU: NegativeBinomialLikelihood (TBNN_LIK_NEG_BINOMIAL) -- over-dispersed counts with log link and a fixed dispersion r,
log p = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y log p + r log q per (row, output), p = sigmoid(f - log r) -- on every kernel family:
the narrow fast3 and fast kernels and their one-launch trajectory kernel, mid, tall and wide (the VALU last layer of one or two outputs and
the MFMA output tile of 3 .. 16), each likelihood path of the layered family (k_lay_tail, k_lay_last, k_lay_lik) and the generic kernel.
Against the oracle in fp64 (the cases are tests/negbin_ref.py's): the value with its constant, the gradient per tensor, the forward
outputs, an injected weight transition with both decisions (log u placed on either side of the reference's log accept ratio, two bands
away), a hyper transition, every launch repeated bit for bit.  Then: row weights, the Poisson limit, refusals, trainChains against solo
runs, pre-training, the ensemble reductions, a row-sharded chain on the stub collective library, and an end-to-end fit on over-dispersed
counts against the Poisson fit.

Bands: the project's -- value 4e-6 relative, gradient 1e-4 of each tensor's largest entry (floor 1e-3), log accept ratio
2e-2 + 1e-4 |lar| + 4e-7 |logp|.  tests/test_negbin_host.py (CPU arithmetic only) shows that the kernel's own formula in fp32 stays inside
them at every case here (value gaps to 1.2e-7, gradient gaps to 1.0e-6), so no case has a band of its own.  Targets: counts drawn from the
model around log-rates 1.5 + 1.2 z; r is spread over {0.5, 2.5, 30, 1e4}, the fast3 case at r = 0.5 with counts up to 22,075.

The Poisson limit (test_poisson_limit): at r = 1e6 the negative-binomial delta is the Poisson delta y - mu times r / (r + mu) -- it differs
by (y - mu) mu / (r + mu).  Rows whose rate at the state is above 20 are left out, so mu / r <= 2e-5 of each row's own delta: inside the
1e-4 gradient band.  On the CPU, fp64 definitions against each other on the test's rows (rates to 18.0): 1.46e-5 of the largest delta
(printed); on an MI355X the two handles' gradients differ by 7.5e-5 of a tensor's largest entry at the most.

End-to-end fit (test_fit_on_overdispersed_counts), measured on an MI355X: see NOTES.md."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import negbin_ref as nb
import optim_ref as R
import tbnn_oracle as o
from tensor_checks import layers_of, tensor_errs
from test_gpu_freerun import SEED

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FUSED = {"fast3": "", "fast": "fast3", "mid": "fast3,fast,tall,wide", "tall": "fast3,fast,mid,wide", "wide": "fast3,fast,mid,tall"}
CASES = {k: v for k, v in nb.CASES.items() if v[4] != "traj"}
NET = [1, 16, 16, 1]                                              # the network(...) of the trainChains and end-to-end tests (tanh)
LIK = o.LIK_NEG_BINOMIAL
LIMIT_DIMS = [5, 50, 50, 50, 1]


def job(spec, lik=LIK, skip="", weighted=False):
    j = {"layers": [list(l) for l in layers_of(spec)], "likelihood": lik, "skip": skip, "flags": ""}
    if weighted:
        j["weighted"] = True
    return j


def jit_jobs():
    """the run-time instantiations this module asks for (jit.prebuild's job format): 14 libraries"""
    jobs = []
    for dims, _n, act, prior, fam, _env, _r in nb.CASES.values():
        if fam in FUSED:
            jobs.append(job(o.make_spec(dims, act, prior, LIK, o.ACT_NONE), skip=FUSED[fam]))
        elif fam == "traj":
            jobs.append(job(o.make_spec(dims, act, prior, LIK, o.ACT_NONE)))
    jobs.append(job(o.make_spec(LIMIT_DIMS, o.ACT_RELU, o.PRIOR_CAUCHY, LIK, o.ACT_NONE), weighted=True))
    jobs.append(job(o.make_spec(LIMIT_DIMS, o.ACT_RELU, o.PRIOR_CAUCHY, LIK, o.ACT_NONE), lik=o.LIK_POISSON))          # the Poisson limit's other side
    jobs.append(job(o.make_spec(NET, o.ACT_TANH, o.PRIOR_CAUCHY, LIK, o.ACT_NONE)))
    # the Poisson fit of the end-to-end test and the predictors' forward chains (fixed-sd Gaussian handles)
    jobs.append(job(o.make_spec(NET, o.ACT_TANH, o.PRIOR_CAUCHY, LIK, o.ACT_NONE), lik=o.LIK_POISSON))
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
    print(f"[negbin] {tag}: logp {lp:.9g} (fp64 {ref64[0]:.9g}) err {ev:.3e} of band 4e-6; gradient err max {max(eg):.3e} of band 1e-4")
    assert np.isfinite(lp) and np.all(np.isfinite(g))
    assert ev <= 4e-6, (tag, lp, ref64[0])
    assert max(eg) <= 1e-4, (tag, eg)


def make_chain(native, monkeypatch, name, spec, **kw):
    fam, env = nb.CASES[name][4], nb.CASES[name][5]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(likelihood=LIK, lik_df=spec.lik_df, **kw)
    if fam in FUSED:
        monkeypatch.setenv("TBNN_JIT_SKIP", FUSED[fam])
        ch = native.Chain(layers_of(spec), jit=True, **kw)
        assert ch.kernel_name.startswith(f"jit-{fam}<") and ",neg-binomial;" in ch.kernel_name, ch.kernel_name
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
    spec, X, Y, theta, eta = nb.problem(name)
    ch = make_chain(native, monkeypatch, name, spec)
    ch.set_data(X, Y)
    lp, g, st = ch.logp_grad(theta, eta)
    for _ in range(2):
        lp2, g2, st2 = ch.logp_grad(theta, eta)
        assert lp2 == lp and st2 == st and np.array_equal(g, g2)
    m = min(500, X.shape[0])
    f = ch.forward(X[:m], theta)
    assert np.array_equal(f, ch.forward(X[:m], theta))
    ch.close()
    check_value_gradient(name, lp, g, spec, nb.ref64(name))
    # stat is the data term with its constant (as Poisson's): sum (y log p + r log q) - C, and logp minus it the priors
    f64 = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    data64 = float(o.log_likelihood(spec, eta, f64, Y, np.float64))
    assert abs(st - data64) <= 4e-6 * abs(data64), (st, data64)
    prior = float(nb.ref64(name)[0] - data64)
    assert abs((lp - st) - prior) <= 4e-6 * max(abs(lp), 1.0)
    assert f.shape == (spec.layers[-1].out_dim, m)
    assert np.abs(f - f64[:, :m]).max() <= 1e-4 * max(1.0, np.abs(f64).max())


@pytest.mark.parametrize("name", list(CASES))
def test_transitions(native, monkeypatch, name):
    spec, X, Y, theta, eta = nb.problem(name)
    rng = np.random.default_rng(4)
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    ch = make_chain(native, monkeypatch, name, spec, seed=SEED, chain_id=2)
    ch.set_data(X, Y)
    lp64 = nb.ref64(name)[0]
    eps = nb.step_size(name)
    ref = o.weight_step(spec, theta, eta, X, Y, eps, 4, p0, -1e30, np.float64)
    tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
    # log u on either side of the reference's log accept ratio, two bands away: the kernel's rounding cannot flip the decision
    for log_u, accept in ((ref.log_accept_ratio - 2 * tol, True), (ref.log_accept_ratio + 2 * tol, False)):
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hmc_step(eps, 4, p0=p0, log_u=log_u)
        print(f"[negbin] {name}: lar {out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g}, band {tol:.3g}), logp {lp64:.6g}")
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
    spec, X, Y, theta, eta = nb.problem("traj")
    r = spec.lik_df
    monkeypatch.setenv("TBNN_TRAJ", "1")
    monkeypatch.setenv("TBNN_JIT_SKIP", "")
    ch = native.Chain(layers_of(spec), likelihood=LIK, lik_df=r, jit=True, seed=SEED)
    assert ch.kernel_name.startswith("jit-fast3<") and ",neg-binomial;" in ch.kernel_name, ch.kernel_name
    ch.set_data(X, Y)
    lp, g, _ = ch.logp_grad(theta, eta)
    check_value_gradient("traj", lp, g, spec, nb.ref64("traj"))
    p0 = np.random.default_rng(5).standard_normal(spec.n_params).astype(np.float32)
    lp64 = nb.ref64("traj")[0]
    eps = nb.step_size("traj")
    for L in (1, 9):
        ref = o.weight_step(spec, theta, eta, X, Y, eps, L, p0, -1e30, np.float64)
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hmc_step(eps, L, p0=p0, log_u=-1e30)
        assert ch.last_transition_path == "trajectory"
        tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
        print(f"[negbin] trajectory L={L}: lar {out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g})")
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


@pytest.mark.parametrize("name", ["fast3", "lay_last"])
def test_row_weights(native, monkeypatch, name):
    spec, X, Y, theta, eta = nb.problem(name)
    n = min(600, X.shape[0])
    X, Y = X[:n], Y[:n]
    w = np.random.default_rng(21).integers(0, 4, n).astype(np.float32)
    vg = lambda Xs, Ys, ws=None: o.target_log_prob_and_grad(spec, theta, eta, Xs, Ys, np.float64, ws)
    ch = make_chain(native, monkeypatch, name, spec)
    ch.set_data(X, Y)
    plain = ch.logp_grad(theta, eta)
    # a weight of 1 everywhere: the unweighted bits
    ch.set_row_weights(np.ones(n, np.float32))
    if nb.CASES[name][4] in FUSED:
        assert ",neg-binomial,weighted;" in ch.kernel_name, ch.kernel_name
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
    print(f"[negbin] {name}: weights vs duplicated rows: value {ev:.3e}, gradient {max(eg):.3e}")
    assert ev <= 4e-6 and max(eg) <= 1e-4, (ev, eg)
    # clearing the weights brings the unweighted bits back
    ch.set_data(X, Y); ch.set_row_weights(w); ch.set_row_weights(None)
    back = ch.logp_grad(theta, eta)
    assert back[0] == plain[0] and np.array_equal(back[1], plain[1])
    ch.close()


def test_poisson_limit(native, monkeypatch):
    """r = 1e6 on rows whose rate at the state is <= 20: the gradient is the Poisson handle's within the gradient band -- no reference
    involved (the module docstring derives the 2e-5 that separates the two definitions there)"""
    dims, n, act, prior = LIMIT_DIMS, 3001, o.ACT_RELU, o.PRIOR_CAUCHY
    spec, X, _Y, theta, eta = nb.problem_of(dims, n, act, prior, 1e6)
    f = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)[0]
    keep = f <= math.log(20.0)
    X, f = X[keep], f[keep]
    assert 1000 <= X.shape[0] < n and X.shape[0] % 16 != 0
    Y = np.random.default_rng(3).poisson(np.exp(f)).astype(np.float32).reshape(-1, 1)
    _t, d_nb = o.negbin_elementwise(f[None], Y, 1e6, np.float64)
    d_po = Y[:, 0].astype(np.float64) - np.exp(f)
    print(f"[negbin] Poisson limit at r = 1e6, rates <= {np.exp(f).max():.2f}: the two fp64 definitions' deltas differ by "
          f"{np.abs(d_nb[0] - d_po).max() / np.abs(d_po).max():.2e} of the largest delta")
    monkeypatch.setenv("TBNN_JIT_SKIP", "")
    pch = native.Chain(layers_of(spec), likelihood=o.LIK_POISSON, jit=True)
    assert pch.kernel_name.startswith("jit-fast3<") and ",poisson;" in pch.kernel_name, pch.kernel_name
    pch.set_data(X, Y)
    _plp, pg, _ = pch.logp_grad(theta, eta)
    ch = native.Chain(layers_of(spec), likelihood=LIK, lik_df=1e6, jit=True)
    assert ch.kernel_name.startswith("jit-fast3<") and ",neg-binomial;" in ch.kernel_name, ch.kernel_name
    ch.set_data(X, Y)
    _lp, g, _ = ch.logp_grad(theta, eta)
    assert np.array_equal(pch.logp_grad(theta, eta)[1], pg)              # the Poisson chain unchanged beside it
    pch.close(); ch.close()
    eg = tensor_errs(spec, g, pg.astype(np.float64), 1e-3)
    print(f"[negbin] Poisson limit at r = 1e6: gradient against the Poisson handle's, worst tensor {max(eg):.3e}")
    assert max(eg) <= 1e-4, eg


def test_refusals(native, monkeypatch):
    spec, X, Y, theta, eta = nb.problem("generic")
    r = spec.lik_df
    layers = layers_of(spec)
    for df in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(native.TbnnError, match="lik_df"):
            native.Chain(layers, likelihood=LIK, lik_df=df, kernel=native.KERNEL_GENERIC)
        with pytest.raises(native.TbnnError, match="lik_df"):
            native.ChainGroup(layers, 2, likelihood=LIK, lik_df=df, kernel=native.KERNEL_GENERIC)
    with pytest.raises(native.TbnnError, match="no activation"):
        native.Chain(layers[:-1] + [layers[-1][:2] + (native.ACT_SIGMOID,) + layers[-1][3:]], likelihood=LIK, lik_df=3.0, kernel=native.KERNEL_GENERIC)
    for unknown in (4, 6, 7, 9):
        with pytest.raises(native.TbnnError, match="unknown likelihood"):
            native.Chain(layers, likelihood=unknown, lik_df=3.0, kernel=native.KERNEL_GENERIC)
    thetas = (theta[None] + 0.01 * np.random.default_rng(1).standard_normal((4, spec.n_params))).astype(np.float32)
    # a negative-binomial handle: targets that are not counts are refused and the handle keeps its rows; r is the descriptor's, the setter
    # is refused; Student-t's predictive distribution is still not built
    ch = native.Chain(layers, likelihood=LIK, lik_df=r, kernel=native.KERNEL_GENERIC)
    ch.set_data(X, Y)
    before = ch.logp_grad(theta, eta)
    for bad in (-1.0, float("nan"), float("inf")):
        Yb = Y.copy()
        Yb[7, 1] = bad
        with pytest.raises(native.TbnnError, match="negative-binomial likelihood takes counts"):
            ch.set_data(X, Yb)
    after = ch.logp_grad(theta, eta)
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    with pytest.raises(native.TbnnError):
        ch.set_row_weights(-np.ones(X.shape[0], np.float32))
    assert ch.logp_grad(theta, eta)[0] == before[0]
    with pytest.raises(native.TbnnError, match="descriptor"):
        ch.set_lik_df(5.0)
    with pytest.raises(native.TbnnError, match="not built"):
        ch.ensemble_predictive(thetas, probs=[0.5], X=X[:64], likelihood=8)
    with pytest.raises(native.TbnnError, match="posterior-mean probability"):
        ch.ensemble_predictive(thetas, probs=[0.5], X=X[:64], likelihood=o.LIK_BERNOULLI)
    Yh = Y[:64] + 0.5                                                   # non-integers are allowed
    per_net, rows = ch.ensemble_loglik(thetas, Y=Yh, X=X[:64])
    assert np.all(np.isfinite(per_net)) and np.all(np.isfinite(rows))
    ch.close()
    # a handle of another likelihood: judging under the negative binomial needs the setter first, and the setter a finite r > 0
    gch = native.Chain(layers, likelihood=o.LIK_FIXED_GAUSSIAN, fixed_sd=1.0, kernel=native.KERNEL_GENERIC)
    with pytest.raises(native.TbnnError, match="tbnn_set_lik_df"):
        gch.ensemble_loglik(thetas, Y=Y[:64], X=X[:64], likelihood=LIK)
    with pytest.raises(native.TbnnError, match="tbnn_set_lik_df"):
        gch.ensemble_loo(thetas, Y=Y[:64], X=X[:64], likelihood=LIK)
    with pytest.raises(native.TbnnError, match="tbnn_set_lik_df"):
        gch.ensemble_predictive(thetas, probs=[0.5], X=X[:64], likelihood=LIK)
    for df in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(native.TbnnError, match="finite and > 0"):
            gch.set_lik_df(df)
    gch.set_lik_df(r)
    per_net, rows = gch.ensemble_loglik(thetas, Y=Y[:64], X=X[:64], likelihood=LIK)
    assert np.all(np.isfinite(per_net)) and np.all(np.isfinite(rows))
    gch.close()


# ---------------------------------------------------------------------------------------------------------------------- pre-training
def test_pretraining_against_the_restatement(native, monkeypatch):
    """Chain.optimize for a few steps against the Adam / AMSGrad restatement of tests/optim_ref.py driven by the oracle's gradient: the
    checked objectives to the value band, the last step's gradient to the gradient band, theta to 8 x the restatement's own fp32 gap"""
    name, steps = "fast3_two_outputs", 6
    spec, X, Y, theta0, eta = nb.problem(name)

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
    print(f"[negbin] optimize: trace {out['trace'][0]:.6f} -> {out['trace'][-1]:.6f} (fp64 {tr64[0]:.6f} -> {tr64[-1]:.6f})")
    assert out["steps_done"] == steps and out["diverged"] == 0 and tr64[-1] > tr64[0]
    assert np.all(np.abs(out["trace"] - tr64) <= 4e-6 * np.maximum(np.abs(tr64), 1.0)), (out["trace"], tr64)
    assert max(tensor_errs(spec, st["g"], g64, 1e-3)) <= 1e-4
    gap = np.abs(th32.astype(np.float64) - th64).max()
    assert np.abs(th.astype(np.float64) - th64).max() <= 8 * gap, (np.abs(th - th64).max(), gap)


# ---------------------------------------------------------------------------------------------------------------------- ensemble reductions
def term_magnitudes(f, Y, r):
    """per (output, row): the sum of the magnitudes that enter one term of the log mass -- the three lgamma values and the two products"""
    f = np.asarray(f, dtype=np.float64)
    y = np.asarray(Y, dtype=np.float64).reshape(f.shape[1], -1).T
    lg = np.vectorize(math.lgamma, otypes=[np.float64])
    t, _d = o.negbin_elementwise(f, Y, r, np.float64)
    return np.abs(lg(y + r)) + abs(math.lgamma(r)) + np.abs(lg(y + 1.0)) + np.abs(t)


def test_ensemble_loglik_and_loo(native, monkeypatch):
    """tbnn_ensemble_loglik and tbnn_ensemble_loo under TBNN_LIK_NEG_BINOMIAL, 16 networks over 517 rows of four outputs, on a
    negative-binomial handle (r from its descriptor) and on a fixed-sd Gaussian handle (r from tbnn_set_lik_df).  The matrix of row
    log-likelihoods against the definition in fp64 from the device's own fp32 predictions: both sides evaluate an fp64 expression of the
    same terms, so the band is rounding alone -- 16 ulp64 of every magnitude that enters a term (the three lgamma values, up to 8e4 each at
    r = 1e4, and the two products), summed over the row's outputs.  LOO, WAIC and lppd against tests/psis_ref.py fed with the device's
    matrix, by the rule and bound of tests/test_gpu_loo.py; per_net and lppd_rows of tbnn_ensemble_loglik against the same matrix."""
    from psis_ref import psis_ref
    from test_gpu_ensemble import U, logsumexp_rows
    from test_gpu_loo import TOL
    spec, X, Y, theta, eta = nb.problem("generic")
    r = spec.lik_df
    m, n, d_out = 16, X.shape[0], spec.layers[-1].out_dim
    assert (n, d_out) == (517, 4) and r == 1e4
    rng = np.random.default_rng(31)
    thetas = (theta[None] + 0.02 * rng.standard_normal((m, spec.n_params))).astype(np.float32)
    layers = layers_of(spec)
    handles = {"negbin": (native.Chain(layers, likelihood=LIK, lik_df=r, kernel=native.KERNEL_GENERIC), r),
               "gaussian": (native.Chain(layers, likelihood=o.LIK_FIXED_GAUSSIAN, fixed_sd=0.3, kernel=native.KERNEL_GENERIC), 2.5)}
    handles["gaussian"][0].set_lik_df(2.5)
    for tag, (ch, disp) in handles.items():
        f = ch.forward_many(thetas, X=X).astype(np.float64)                          # [m, d_out, n]
        rr = float(np.float32(disp))
        l = np.stack([o.negbin_terms(f[i], Y, rr).sum(axis=0) for i in range(m)])                 # [m, n]
        mag = np.stack([term_magnitudes(f[i], Y, rr).sum(axis=0) for i in range(m)])
        got = ch.ensemble_loo(thetas, Y=Y, X=X, likelihood=LIK, pointwise=True)
        again = ch.ensemble_loo(thetas, Y=Y, X=X, likelihood=LIK, pointwise=True)
        for key in got:
            assert np.array_equal(got[key], again[key], equal_nan=True), key
        pw = got["pointwise"]
        e, tol = np.abs(pw - l), 16 * U * mag
        print(f"[negbin] ensemble on a {tag} handle: matrix against the fp64 definition, err max {e.max():.3e}, worst err/tol {np.max(e / tol):.3f}")
        assert pw.shape == (m, n) and np.all(np.isfinite(pw)) and np.all(e <= tol)
        ref = psis_ref(pw, 1.0)
        for key in ("elpd_loo", "pareto_k", "lppd", "p_waic"):
            g_, w_ = got[key], ref[key]
            assert np.array_equal(np.isposinf(g_), np.isposinf(w_)) and np.array_equal(np.isnan(g_), np.isnan(w_)), key
            fin = np.isfinite(w_)
            d = np.abs(g_[fin] - w_[fin]) / (np.abs(w_[fin]) if key in ("elpd_loo", "lppd") else 1.0)
            print(f"[negbin] ensemble on a {tag} handle: {key} diff {d.max(initial=0.0):.3e} (bound {TOL:.3e})")
            assert d.max(initial=0.0) <= TOL, (tag, key)
        for wts in (None, (rng.random(m) * (rng.random(m) > 0.2)).astype(np.float32)):
            per_net, rows = ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=LIK, weights=wts)
            assert np.all(np.abs(per_net - pw.sum(axis=1)) <= n * U * np.abs(pw).sum(axis=1))
            ww = np.ones(m) if wts is None else wts.astype(np.float64)
            want = logsumexp_rows(pw, ww) - math.log(ww.sum())
            assert np.all(np.abs(rows - want) <= (m + 8) * U + 4 * U * np.abs(want))
            if wts is None:
                assert np.array_equal(rows.view(np.uint64), got["lppd"].view(np.uint64))
        ch.close()


# ---------------------------------------------------------------------------------------------------------------------- row-sharded chain
def test_row_shard_two_ranks(tmp_path, native, monkeypatch):
    """world 2 on the stub collective library (tests/stubccl/worker_negbin.py: two fresh child processes, each under its own time limit):
    the statistic is all-reduced, every rank taking the constant of its own rows off first, so the sharded chain takes the unsharded
    chain's decisions and reaches its state, within the sharding band of tests/test_gpu_multirank.py"""
    from conftest import wait_gpu_quiet
    from test_gpu_multirank import build_stub
    sys.path.insert(0, os.path.join(HERE, "stubccl"))
    import worker_negbin as ws
    wait_gpu_quiet()
    env = dict(os.environ, TBNN_RCCL_LIB=build_stub(), TBNN_JIT="0", TBNN_PREBUILD_JIT="0")
    idfile = str(tmp_path / "shard.id")
    procs = []
    for rk in range(2):
        out = str(tmp_path / f"shard_{rk}.npz")
        procs.append((out, subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "stubccl", "worker_negbin.py"), str(rk), "2", idfile, out],
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
DISP = 1.5


def log_rate(x):
    """a smooth log-rate: rates from 5 to 50"""
    return math.log(5.0) + math.log(10.0) * (0.5 + 0.5 * np.sin(1.5 * x))


def overdispersed(n, seed):
    """x ~ U(-2, 2), y negative binomial of dispersion 1.5 around exp(log_rate(x)) (a gamma-Poisson mixture): variance mu + mu^2 / 1.5, up to
    34 times the Poisson variance"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, 1)).astype(np.float32)
    mu = np.exp(log_rate(X.astype(np.float64)))
    return X, rng.poisson(rng.gamma(DISP, mu / DISP)).astype(np.float32)


def make_net(X, Y, Xv, Yv, chain_id=0, **kw):
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.network import network
    net = network(np.float32, 1, X, Y, Xv, Yv, chain_id=chain_id, **kw)
    net.add(DenseLayer(1, 16, seed=1000)); net.add(Tanh())
    net.add(DenseLayer(16, 16, seed=2000)); net.add(Tanh())
    net.add(DenseLayer(16, 1, seed=3000))
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    return net


def test_train_chains_equal_solo_runs(tmp_path, monkeypatch, native):
    from tensorbnn_amd.likelihood import NegativeBinomialLikelihood
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, Y = overdispersed(400, 1)
    Xv, Yv = overdispersed(200, 2)
    C, EPOCHS = 3, 14
    lik = lambda: NegativeBinomialLikelihood(dispersion=DISP)
    grp_net = make_net(X, Y, Xv, Yv)
    rec = grp_net.trainChains(C, EPOCHS, 4, lik(), adjustHypers=True, folderName="multi", networksPerFile=2)
    assert len(rec) == EPOCHS and all(len(rc["main"]) == C for rc in rec)
    for c in range(C):
        net = make_net(X, Y, Xv, Yv, chain_id=c)
        solo = net.train(EPOCHS, 4, lik(), adjustHypers=True, folderName="solo%d" % c, networksPerFile=2, verbose=False)
        assert net._chain.kernel_name.startswith("jit-fast3<") and "neg-binomial" in net._chain.kernel_name, net._chain.kernel_name
        for rg, rs in zip(rec, solo):
            assert rg["eps"][c] == rs["eps"] and rg["L"][c] == rs["L"]
            for k in ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new", "sjd"):
                assert rg["main"][c][k] == rs["main"][k], (c, rg["iter"], k)
            assert rg["hyper"][c]["log_accept_ratio"] == rs["hyper"]["log_accept_ratio"]
            assert rg["hyper_step_size"][c] == rs["hyper_step_size"]


def test_fit_on_overdispersed_counts(tmp_path, monkeypatch, native):
    """[1, 16, 16, 1] on 400 rows of counts drawn from a negative binomial of dispersion 1.5 around a smooth log-rate (rates 5 .. 50),
    pretrain then train, once under PoissonLikelihood and once under NegativeBinomialLikelihood(dispersion=1.5), trained the same way.  On
    300 held-out rows predictor.compareLoo favours the negative binomial by more than 2 se_diff, and the coverage of the 90 % predictive
    interval (predictor.predictiveInterval) is closer to 0.9 under it than under Poisson, whose intervals are far too narrow.  Only the
    orderings are asserted; the figures are printed (NOTES.md records them)."""
    from tensorbnn_amd.likelihood import NegativeBinomialLikelihood, PoissonLikelihood
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, Y = overdispersed(400, 1)
    Xv, Yv = overdispersed(200, 2)
    Xh, Yh = overdispersed(300, 3)
    fits = {}
    for tag, lik in (("negbin", NegativeBinomialLikelihood(dispersion=DISP)), ("poisson", PoissonLikelihood())):
        net = make_net(X, Y, Xv, Yv)
        hist = net.pretrain(lik, cycles=2, epochs=400, learningRate=0.01, verbose=False)
        net.train(70, 4, lik, folderName=tag, networksPerFile=1, verbose=False)
        assert ("neg-binomial" if tag == "negbin" else "poisson") in net._chain.kernel_name, net._chain.kernel_name
        p = predictor(str(tmp_path / tag) + "/", likelihood=lik)
        loo = p.loo(Xh, Yh)
        waic = p.waic(Xh, Yh)
        lower, median, upper = p.predictiveInterval(Xh, level=0.9)
        below, at = p.predictiveCDF(Xh, Yh)
        yh = Yh[:, 0].astype(np.float64)
        cover = float(np.mean((yh >= lower[0]) & (yh <= upper[0])))
        mean, tot = p.predictMoments(Xh, countVariance=True)
        assert np.all(np.isfinite(lower)) and np.all(lower <= median) and np.all(median <= upper) and np.all(lower == np.floor(lower))
        assert np.all((below >= 0) & (below <= at) & (at <= 1)) and np.all(tot >= mean) and np.isfinite(loo["elpd_loo"]) and np.isfinite(waic["elpd_waic"])
        fits[tag] = (cover, loo)
        print(f"[negbin] {tag} fit: {p.numNetworks} networks after {hist['steps']} pre-training steps; on {len(Xh)} held-out rows: 90 % predictive "
              f"interval covers {cover:.3f}, mean width {float(np.mean(upper - lower)):.1f}, elpd_loo {loo['elpd_loo']:.1f} (se {loo['se']:.1f}), "
              f"elpd_waic {waic['elpd_waic']:.1f}, mean predictive sd {float(np.mean(np.sqrt(tot))):.2f}")
    cmp_ = predictor.compareLoo(fits["negbin"][1], fits["poisson"][1])
    print(f"[negbin] compareLoo(negbin, poisson): elpd_diff {cmp_['elpd_diff']:.1f}, se_diff {cmp_['se_diff']:.1f}; "
          f"coverage {fits['negbin'][0]:.3f} against {fits['poisson'][0]:.3f}")
    assert cmp_["elpd_diff"] > 2.0 * cmp_["se_diff"]
    assert abs(fits["negbin"][0] - 0.9) < abs(fits["poisson"][0] - 0.9)
