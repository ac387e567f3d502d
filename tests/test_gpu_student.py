"""GPU: StudentTLikelihood (TBNN_LIK_STUDENT_T) -- independent Student-t noise of fixed scale s and nu degrees of freedom,
log p = c(nu, s) - (nu + 1) / 2 log1p(r^2 / (nu s^2)) per (row, output) -- on every kernel family: the narrow fast3 and fast kernels and their
one-launch trajectory kernel, mid, tall and wide (the VALU last layer of one or two outputs and the MFMA output tile of 3 .. 16), each
likelihood path of the layered family (k_lay_tail, k_lay_last, k_lay_lik) and the generic kernel.  Against the oracle in fp64 (the cases are
tests/student_ref.py's): the value with its constant, the gradient per tensor, the forward outputs, an injected weight transition with
both decisions (log u placed on either side of the reference's log accept ratio, two bands away), a hyper transition, every launch repeated
bit for bit.  Then: row weights, the Gaussian limit, refusals, trainChains against solo runs, pre-training, the ensemble reductions, a
row-sharded chain on the stub collective library, and an end-to-end fit on contaminated data against the Gaussian fit.

Bands: the project's -- value 4e-6 relative, gradient 1e-4 of each tensor's largest entry (floor 1e-3), log accept ratio
2e-2 + 1e-4 |lar| + 4e-7 |logp|.  tests/test_student_host.py (CPU arithmetic only) shows that the kernel's own formula in fp32 stays inside them
at every case here (value gaps to 9.4e-8, gradient gaps to 1.8e-6), so no case has a band of its own.  Targets: the teacher's outputs plus
N(0, s^2), 5 % of the rows moved by 20 s .. 50 s, so that r^2 << nu s^2 and r^2 >> nu s^2 both occur in every tile (the host test asserts it);
nu is spread over {1, 2.5, 30, 1e4} and s over {0.1, 1}, the fast3 case at nu = 1e4.

The Gaussian limit (test_gaussian_limit) runs on CLEAN targets (no outliers): at nu = 1e6 the Student-t delta is the Gaussian's times
(1 + 1/nu) / (1 + r^2 / (nu s^2)), and |r| <= 6 s keeps that within 4e-5 of 1, inside the 1e-4 gradient band; with 50 s outliers the two
likelihoods differ by 2.5e-3 on exactly the rows that dominate the Gaussian gradient, by the definition and not by rounding.

End-to-end fit (test_fit_on_contaminated_data), measured on an MI355X: see NOTES.md."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import optim_ref as R
import student_ref as sr
import tbnn_oracle as o
from tensor_checks import layers_of, tensor_errs
from test_gpu_freerun import SEED

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FUSED = {"fast3": "", "fast": "fast3", "mid": "fast3,fast,tall,wide", "tall": "fast3,fast,mid,wide", "wide": "fast3,fast,mid,tall"}
CASES = {k: v for k, v in sr.CASES.items() if v[4] != "traj"}
NET = [1, 16, 16, 1]                                              # the network(...) of the trainChains and end-to-end tests (tanh)
LIK = o.LIK_STUDENT_T


def job(spec, lik=LIK, skip="", weighted=False):
    j = {"layers": [list(l) for l in layers_of(spec)], "likelihood": lik, "skip": skip, "flags": ""}
    if weighted:
        j["weighted"] = True
    return j


def jit_jobs():
    """the run-time instantiations this module asks for (jit.prebuild's job format): 12 libraries"""
    jobs = []
    for dims, _n, act, prior, fam, _env, _nu, _s in sr.CASES.values():
        if fam in FUSED:
            jobs.append(job(o.make_spec(dims, act, prior, LIK, o.ACT_NONE), skip=FUSED[fam]))
        elif fam == "traj":
            jobs.append(job(o.make_spec(dims, act, prior, LIK, o.ACT_NONE)))
    jobs.append(job(o.make_spec([5, 50, 50, 50, 1], o.ACT_RELU, o.PRIOR_CAUCHY, LIK, o.ACT_NONE), weighted=True))
    jobs.append(job(o.make_spec(NET, o.ACT_TANH, o.PRIOR_CAUCHY, LIK, o.ACT_NONE)))
    # the Gaussian fit of the end-to-end test and the predictors' forward chains (fixed-sd Gaussian handles)
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
    print(f"[student] {tag}: logp {lp:.9g} (fp64 {ref64[0]:.9g}) err {ev:.3e} of band 4e-6; gradient err max {max(eg):.3e} of band 1e-4")
    assert np.isfinite(lp) and np.all(np.isfinite(g))
    assert ev <= 4e-6, (tag, lp, ref64[0])
    assert max(eg) <= 1e-4, (tag, eg)


def make_chain(native, monkeypatch, name, spec, **kw):
    fam, env = sr.CASES[name][4], sr.CASES[name][5]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(likelihood=LIK, fixed_sd=spec.fixed_sd, lik_df=spec.lik_df, **kw)
    if fam in FUSED:
        monkeypatch.setenv("TBNN_JIT_SKIP", FUSED[fam])
        ch = native.Chain(layers_of(spec), jit=True, **kw)
        assert ch.kernel_name.startswith(f"jit-{fam}<") and ",student-t;" in ch.kernel_name, ch.kernel_name
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
    spec, X, Y, theta, eta = sr.problem(name)
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
    check_value_gradient(name, lp, g, spec, sr.ref64(name))
    # stat is sum log1p(r^2 / (nu s^2)): the data term is rows d_out c(nu, s) - (nu + 1) / 2 stat, and logp minus it the priors
    f64 = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    nu = spec.lik_df
    stat64 = o.data_statistic(spec, eta, f64, Y, np.float64)
    assert abs(st - stat64) <= 4e-6 * abs(stat64), (st, stat64)
    data = X.shape[0] * spec.layers[-1].out_dim * o.student_const(nu, o.student_scale(spec)) - 0.5 * (nu + 1.0) * st
    prior = float(sr.ref64(name)[0] - o.log_likelihood(spec, eta, f64, Y, np.float64))
    assert abs((lp - data) - prior) <= 4e-6 * max(abs(lp), 1.0)
    assert f.shape == (spec.layers[-1].out_dim, m)
    assert np.abs(f - f64[:, :m]).max() <= 1e-4 * max(1.0, np.abs(f64).max())


@pytest.mark.parametrize("name", list(CASES))
def test_transitions(native, monkeypatch, name):
    spec, X, Y, theta, eta = sr.problem(name)
    rng = np.random.default_rng(4)
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    ch = make_chain(native, monkeypatch, name, spec, seed=SEED, chain_id=2)
    ch.set_data(X, Y)
    lp64 = sr.ref64(name)[0]
    eps = sr.step_size(name)
    ref = o.weight_step(spec, theta, eta, X, Y, eps, 4, p0, -1e30, np.float64)
    tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
    # log u on either side of the reference's log accept ratio, two bands away: the kernel's rounding cannot flip the decision
    for log_u, accept in ((ref.log_accept_ratio - 2 * tol, True), (ref.log_accept_ratio + 2 * tol, False)):
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hmc_step(eps, 4, p0=p0, log_u=log_u)
        print(f"[student] {name}: lar {out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g}, band {tol:.3g}), logp {lp64:.6g}")
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
    spec, X, Y, theta, eta = sr.problem("traj")
    monkeypatch.setenv("TBNN_TRAJ", "1")
    monkeypatch.setenv("TBNN_JIT_SKIP", "")
    ch = native.Chain(layers_of(spec), likelihood=LIK, fixed_sd=spec.fixed_sd, lik_df=spec.lik_df, jit=True, seed=SEED)
    assert ch.kernel_name.startswith("jit-fast3<") and ",student-t;" in ch.kernel_name, ch.kernel_name
    ch.set_data(X, Y)
    lp, g, _ = ch.logp_grad(theta, eta)
    check_value_gradient("traj", lp, g, spec, sr.ref64("traj"))
    p0 = np.random.default_rng(5).standard_normal(spec.n_params).astype(np.float32)
    lp64 = sr.ref64("traj")[0]
    eps = sr.step_size("traj")
    for L in (1, 9):
        ref = o.weight_step(spec, theta, eta, X, Y, eps, L, p0, -1e30, np.float64)
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hmc_step(eps, L, p0=p0, log_u=-1e30)
        assert ch.last_transition_path == "trajectory"
        tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
        print(f"[student] trajectory L={L}: lar {out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g})")
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
    spec, X, Y, theta, eta = sr.problem(name)
    n = min(600, X.shape[0])
    X, Y = X[:n], Y[:n]
    w = np.random.default_rng(21).integers(0, 4, n).astype(np.float32)
    vg = lambda Xs, Ys, ws=None: o.target_log_prob_and_grad(spec, theta, eta, Xs, Ys, np.float64, ws)
    ch = make_chain(native, monkeypatch, name, spec)
    ch.set_data(X, Y)
    plain = ch.logp_grad(theta, eta)
    # a weight of 1 everywhere: the unweighted bits
    ch.set_row_weights(np.ones(n, np.float32))
    if sr.CASES[name][4] in FUSED:
        assert ",student-t,weighted;" in ch.kernel_name, ch.kernel_name
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
    print(f"[student] {name}: weights vs duplicated rows: value {ev:.3e}, gradient {max(eg):.3e}")
    assert ev <= 4e-6 and max(eg) <= 1e-4, (ev, eg)
    # clearing the weights brings the unweighted bits back
    ch.set_data(X, Y); ch.set_row_weights(w); ch.set_row_weights(None)
    back = ch.logp_grad(theta, eta)
    assert back[0] == plain[0] and np.array_equal(back[1], plain[1])
    ch.close()


def test_gaussian_limit(native, monkeypatch):
    """nu = 1e6 and the same s on clean targets: the data gradient is the fixed-sd Gaussian handle's (on its ahead-of-time table) within the
    gradient band -- no reference involved (the module docstring derives the 4e-5 that separates the two definitions there)"""
    dims, n, act, prior, s = [5, 50, 50, 50, 1], 3001, o.ACT_RELU, o.PRIOR_CAUCHY, 0.1
    spec, X, Y, theta, eta = sr.problem_of(dims, n, act, prior, 1e6, s, outliers=0.0)
    # clean: the targets sit within 6 s of THIS state's outputs
    f = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64).T
    Y = (f + s * np.clip(np.random.default_rng(3).standard_normal(f.shape), -6, 6)).astype(np.float32)
    gch = native.Chain(layers_of(spec), likelihood=o.LIK_FIXED_GAUSSIAN, fixed_sd=s, jit=True)
    assert gch.kernel_name.startswith("fast3<") and "student" not in gch.kernel_name, gch.kernel_name
    gch.set_data(X, Y)
    _glp, gg, _ = gch.logp_grad(theta, eta)
    monkeypatch.setenv("TBNN_JIT_SKIP", "")
    ch = native.Chain(layers_of(spec), likelihood=LIK, fixed_sd=s, lik_df=1e6, jit=True)
    assert ch.kernel_name.startswith("jit-fast3<") and ",student-t;" in ch.kernel_name, ch.kernel_name
    ch.set_data(X, Y)
    _lp, g, _ = ch.logp_grad(theta, eta)
    g2 = gch.logp_grad(theta, eta)[1]
    assert np.array_equal(g2, gg)                                        # the Gaussian chain unchanged beside it
    gch.close(); ch.close()
    eg = tensor_errs(spec, g, gg.astype(np.float64), 1e-3)
    print(f"[student] Gaussian limit at nu = 1e6: gradient against the fixed-sd Gaussian handle's, worst tensor {max(eg):.3e}")
    assert max(eg) <= 1e-4, eg


def test_refusals(native, monkeypatch):
    spec, X, Y, theta, eta = sr.problem("generic")
    nu = spec.lik_df
    layers = layers_of(spec)
    for df in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(native.TbnnError, match="lik_df"):
            native.Chain(layers, likelihood=LIK, fixed_sd=1.0, lik_df=df, kernel=native.KERNEL_GENERIC)
        with pytest.raises(native.TbnnError, match="lik_df"):
            native.ChainGroup(layers, 2, likelihood=LIK, fixed_sd=1.0, lik_df=df, kernel=native.KERNEL_GENERIC)
    with pytest.raises(native.TbnnError, match="fixed_sd"):
        native.Chain(layers, likelihood=LIK, fixed_sd=0.0, lik_df=3.0, kernel=native.KERNEL_GENERIC)
    for unknown in (4, 6, 7):
        with pytest.raises(native.TbnnError, match="unknown likelihood"):
            native.Chain(layers, likelihood=unknown, lik_df=3.0, kernel=native.KERNEL_GENERIC)
    thetas = (theta[None] + 0.01 * np.random.default_rng(1).standard_normal((4, spec.n_params))).astype(np.float32)
    # a Student-t handle: nu is the descriptor's, the setter is refused
    ch = native.Chain(layers, likelihood=LIK, fixed_sd=1.0, lik_df=nu, kernel=native.KERNEL_GENERIC)
    with pytest.raises(native.TbnnError, match="descriptor"):
        ch.set_lik_df(5.0)
    with pytest.raises(native.TbnnError, match="not built"):
        ch.ensemble_predictive(thetas, probs=[0.5], X=X[:64])
    with pytest.raises(native.TbnnError, match="not built"):
        ch.ensemble_predictive(thetas, Y=Y[:64], X=X[:64])
    ch.close()
    # a handle of another likelihood: judging under Student-t needs the setter first, and the setter a finite df > 0
    gch = native.Chain(layers, likelihood=o.LIK_FIXED_GAUSSIAN, fixed_sd=1.0, kernel=native.KERNEL_GENERIC)
    with pytest.raises(native.TbnnError, match="tbnn_set_lik_df"):
        gch.ensemble_loglik(thetas, Y=Y[:64], X=X[:64], likelihood=LIK)
    with pytest.raises(native.TbnnError, match="tbnn_set_lik_df"):
        gch.ensemble_loo(thetas, Y=Y[:64], X=X[:64], likelihood=LIK)
    for df in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(native.TbnnError, match="finite and > 0"):
            gch.set_lik_df(df)
    with pytest.raises(native.TbnnError, match="not built"):
        gch.ensemble_predictive(thetas, probs=[0.5], X=X[:64], likelihood=LIK)
    gch.set_lik_df(nu)
    per_net, rows = gch.ensemble_loglik(thetas, Y=Y[:64], X=X[:64], likelihood=LIK)
    assert np.all(np.isfinite(per_net)) and np.all(np.isfinite(rows))
    gch.close()


# ---------------------------------------------------------------------------------------------------------------------- pre-training
def test_pretraining_against_the_restatement(native, monkeypatch):
    """Chain.optimize for a few steps against the Adam / AMSGrad restatement of tests/optim_ref.py driven by the oracle's gradient: the
    checked objectives to the value band, the last step's gradient to the gradient band, theta to 8 x the restatement's own fp32 gap"""
    name, steps = "fast3_two_outputs", 6
    spec, X, Y, theta0, eta = sr.problem(name)

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
    print(f"[student] optimize: trace {out['trace'][0]:.6f} -> {out['trace'][-1]:.6f} (fp64 {tr64[0]:.6f} -> {tr64[-1]:.6f})")
    assert out["steps_done"] == steps and out["diverged"] == 0 and tr64[-1] > tr64[0]
    assert np.all(np.abs(out["trace"] - tr64) <= 4e-6 * np.maximum(np.abs(tr64), 1.0)), (out["trace"], tr64)
    assert max(tensor_errs(spec, st["g"], g64, 1e-3)) <= 1e-4
    gap = np.abs(th32.astype(np.float64) - th64).max()
    assert np.abs(th.astype(np.float64) - th64).max() <= 8 * gap, (np.abs(th - th64).max(), gap)


# ---------------------------------------------------------------------------------------------------------------------- ensemble reductions
def test_ensemble_loglik_and_loo(native, monkeypatch):
    """tbnn_ensemble_loglik and tbnn_ensemble_loo under TBNN_LIK_STUDENT_T, 16 networks over 517 rows of four outputs, on a Student-t handle
    (nu from its descriptor) and on a fixed-sd Gaussian handle (nu from tbnn_set_lik_df; per-network scales).  The matrix of row
    log-likelihoods against the definition in fp64 from the device's own fp32 predictions: both sides evaluate the same fp64 expression, so
    the band is rounding alone -- 16 ulp64 of every magnitude that enters a term (the constant, whose two lgamma are up to nu / 2 log nu
    each, and the scaled log1p), summed over the row's outputs.  LOO, WAIC and lppd against tests/psis_ref.py fed with the device's matrix,
    by the rule and bound of tests/test_gpu_loo.py; per_net and lppd_rows of tbnn_ensemble_loglik against the same matrix."""
    from psis_ref import psis_ref
    from test_gpu_ensemble import U, logsumexp_rows
    from test_gpu_loo import TOL
    spec, X, Y, theta, eta = sr.problem("generic")
    nu = spec.lik_df
    m, n, d_out = 16, X.shape[0], spec.layers[-1].out_dim
    assert (n, d_out) == (517, 4)
    rng = np.random.default_rng(31)
    thetas = (theta[None] + 0.02 * rng.standard_normal((m, spec.n_params))).astype(np.float32)
    sds = (0.6 + rng.random(m)).astype(np.float32)
    layers = layers_of(spec)
    handles = {"student": (native.Chain(layers, likelihood=LIK, fixed_sd=spec.fixed_sd, lik_df=nu, kernel=native.KERNEL_GENERIC), None, nu),
               "gaussian": (native.Chain(layers, likelihood=o.LIK_FIXED_GAUSSIAN, fixed_sd=0.3, kernel=native.KERNEL_GENERIC), sds, 30.0)}
    handles["gaussian"][0].set_lik_df(30.0)
    for tag, (ch, sd, df) in handles.items():
        f = ch.forward_many(thetas, X=X).astype(np.float64)                          # [m, d_out, n]
        s_i = np.full(m, o.student_scale(spec)) if sd is None else sd.astype(np.float64)
        l = np.stack([o.student_terms(f[i], Y, df, s_i[i]).sum(axis=0) for i in range(m)])                 # [m, n]
        mag = np.stack([(abs(o.student_const(df, s_i[i])) + 2 * abs(math.lgamma(0.5 * (df + 1.0))) + np.abs(o.student_terms(f[i], Y, df, s_i[i]))).sum(axis=0) for i in range(m)])
        got = ch.ensemble_loo(thetas, Y=Y, X=X, likelihood=LIK, sd=sd, pointwise=True)
        again = ch.ensemble_loo(thetas, Y=Y, X=X, likelihood=LIK, sd=sd, pointwise=True)
        for key in got:
            assert np.array_equal(got[key], again[key], equal_nan=True), key
        pw = got["pointwise"]
        e, tol = np.abs(pw - l), 16 * U * mag
        print(f"[student] ensemble on a {tag} handle: matrix against the fp64 definition, err max {e.max():.3e}, worst err/tol {np.max(e / tol):.3f}")
        assert pw.shape == (m, n) and np.all(np.isfinite(pw)) and np.all(e <= tol)
        ref = psis_ref(pw, 1.0)
        for key in ("elpd_loo", "pareto_k", "lppd", "p_waic"):
            g_, w_ = got[key], ref[key]
            assert np.array_equal(np.isposinf(g_), np.isposinf(w_)) and np.array_equal(np.isnan(g_), np.isnan(w_)), key
            fin = np.isfinite(w_)
            d = np.abs(g_[fin] - w_[fin]) / (np.abs(w_[fin]) if key in ("elpd_loo", "lppd") else 1.0)
            print(f"[student] ensemble on a {tag} handle: {key} diff {d.max(initial=0.0):.3e} (bound {TOL:.3e})")
            assert d.max(initial=0.0) <= TOL, (tag, key)
        for wts in (None, (rng.random(m) * (rng.random(m) > 0.2)).astype(np.float32)):
            per_net, rows = ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=LIK, sd=sd, weights=wts)
            assert np.all(np.abs(per_net - pw.sum(axis=1)) <= n * U * np.abs(pw).sum(axis=1))
            ww = np.ones(m) if wts is None else wts.astype(np.float64)
            want = logsumexp_rows(pw, ww) - math.log(ww.sum())
            assert np.all(np.abs(rows - want) <= (m + 8) * U + 4 * U * np.abs(want))
            if wts is None:
                assert np.array_equal(rows.view(np.uint64), got["lppd"].view(np.uint64))
        ch.close()


# ---------------------------------------------------------------------------------------------------------------------- row-sharded chain
def test_row_shard_two_ranks(tmp_path, native, monkeypatch):
    """world 2 on the stub collective library (tests/stubccl/worker_student.py: two fresh child processes, each under its own time limit):
    the statistic is all-reduced and the constant counts the GLOBAL rows, so the sharded chain takes the unsharded chain's decisions and
    reaches its state, within the sharding band of tests/test_gpu_multirank.py"""
    from conftest import wait_gpu_quiet
    from test_gpu_multirank import build_stub
    sys.path.insert(0, os.path.join(HERE, "stubccl"))
    import worker_student as ws
    wait_gpu_quiet()
    env = dict(os.environ, TBNN_RCCL_LIB=build_stub(), TBNN_JIT="0", TBNN_PREBUILD_JIT="0")
    idfile = str(tmp_path / "shard.id")
    procs = []
    for r in range(2):
        out = str(tmp_path / f"shard_{r}.npz")
        procs.append((out, subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "stubccl", "worker_student.py"), str(r), "2", idfile, out],
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
        rows = [tuple(r[name + "_rows"]) for r in ranks]
        assert rows[0][0] == 0 and rows[0][1] == rows[1][0] and rows[1][1] == n, rows
        for r in ranks:
            assert str(r[name + "_kernel"]) == ref.kernel_name
            assert abs(float(r[name + "_lp"]) - lp0) <= 1e-7 * abs(lp0) + 1e-6
            assert abs(float(r[name + "_st"]) - st0) <= 1e-9 * abs(st0)
            np.testing.assert_allclose(r[name + "_g"], g0, rtol=0, atol=4e-6 * np.abs(g0).max())
            np.testing.assert_allclose(r[name + "_trace"], outs[0]["trace_logp"], rtol=1e-7, atol=1e-5)
            for k in range(2):
                assert abs(r[name + "_lar"][k] - outs[k]["log_accept_ratio"]) <= 2e-3 + 1e-5 * abs(outs[k]["log_accept_ratio"])
                assert r[name + "_acc"][k] == outs[k]["accepted"]
            np.testing.assert_allclose(r[name + "_theta"], th_ref, rtol=0, atol=2e-6 * max(1.0, np.abs(th_ref).max()))
        np.testing.assert_array_equal(ranks[0][name + "_theta"], ranks[1][name + "_theta"])       # every rank took the same decisions
        np.testing.assert_array_equal(ranks[0][name + "_g"], ranks[1][name + "_g"])
        assert float(ranks[0][name + "_lp"]) == float(ranks[1][name + "_lp"])
        check_value_gradient("shard " + name, float(ranks[0][name + "_lp"]), ranks[0][name + "_g"], spec,
                             o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64))
        ref.close()


# ---------------------------------------------------------------------------------------------------------------------- network / train
S_NOISE, DF = 0.1, 4.0


def teacher(x):
    return np.sin(2.0 * x)


def contaminated(n, seed, frac=0.08):
    """x ~ U(-2, 2), y = sin 2x + N(0, 0.1^2); `frac` of the rows are gross outliers, moved UP by 20 s .. 50 s (2 .. 5): a one-sided
    contamination biases a Gaussian fit by about frac x 3.5 = 0.28, almost three noise scales"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, 1)).astype(np.float32)
    Y = teacher(X.astype(np.float64)) + S_NOISE * rng.standard_normal((n, 1))
    bad = rng.random(n) < frac
    Y[bad] += S_NOISE * rng.uniform(20.0, 50.0, (int(bad.sum()), 1))
    return X, Y.astype(np.float32), bad


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
    from tensorbnn_amd.likelihood import StudentTLikelihood
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, Y, _ = contaminated(400, 1)
    Xv, Yv, _ = contaminated(200, 2)
    C, EPOCHS = 3, 14
    lik = lambda: StudentTLikelihood(df=DF, sd=S_NOISE)
    grp_net = make_net(X, Y, Xv, Yv)
    rec = grp_net.trainChains(C, EPOCHS, 4, lik(), adjustHypers=True, folderName="multi", networksPerFile=2)
    assert len(rec) == EPOCHS and all(len(r["main"]) == C for r in rec)
    for c in range(C):
        net = make_net(X, Y, Xv, Yv, chain_id=c)
        solo = net.train(EPOCHS, 4, lik(), adjustHypers=True, folderName="solo%d" % c, networksPerFile=2, verbose=False)
        assert net._chain.kernel_name.startswith("jit-fast3<") and "student-t" in net._chain.kernel_name, net._chain.kernel_name
        for rg, rs in zip(rec, solo):
            assert rg["eps"][c] == rs["eps"] and rg["L"][c] == rs["L"]
            for k in ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new", "sjd"):
                assert rg["main"][c][k] == rs["main"][k], (c, rg["iter"], k)
            assert rg["hyper"][c]["log_accept_ratio"] == rs["hyper"]["log_accept_ratio"]
            assert rg["hyper_step_size"][c] == rs["hyper_step_size"]


def test_fit_on_contaminated_data(tmp_path, monkeypatch, native):
    """[1, 16, 16, 1] on 400 rows with 8 % gross outliers, pretrain then train, once under StudentTLikelihood(df=4, sd=0.1) and once under
    FixedGaussianLikelihood(sd=0.1), trained the same way.  On clean held-out rows the Student-t fit's posterior-mean prediction is closer
    (mean squared error) to the noiseless teacher; on held-out CONTAMINATED rows predictor.compareLoo favours the Student-t model.  Only the
    orderings are asserted; the figures are printed (NOTES.md records them)."""
    from tensorbnn_amd.likelihood import FixedGaussianLikelihood, StudentTLikelihood
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, Y, bad = contaminated(400, 1)
    Xv, Yv, _ = contaminated(200, 2)
    assert 20 <= bad.sum() <= 45
    Xc = np.linspace(-1.9, 1.9, 300, dtype=np.float32).reshape(-1, 1)          # clean held-out rows: judged against the noiseless teacher
    Xh, Yh, badh = contaminated(300, 3)                                        # contaminated held-out rows: judged by LOO
    fits = {}
    for tag, lik in (("student", StudentTLikelihood(df=DF, sd=S_NOISE)), ("gaussian", FixedGaussianLikelihood(sd=S_NOISE))):
        net = make_net(X, Y, Xv, Yv)
        hist = net.pretrain(lik, cycles=2, epochs=400, learningRate=0.01, verbose=False)
        net.train(70, 4, lik, folderName=tag, networksPerFile=1, verbose=False)
        if tag == "student":
            assert "student-t" in net._chain.kernel_name, net._chain.kernel_name
        p = predictor(str(tmp_path / tag) + "/", likelihood=lik)
        mean, _var = p.predictMoments(Xc)
        mse = float(np.mean((mean[0] - teacher(Xc[:, 0].astype(np.float64))) ** 2))
        loo = p.loo(Xh, Yh)
        waic = p.waic(Xh, Yh)
        per_net, per_row = p.logPredictiveDensity(Xh, Yh)
        assert per_net.shape == (p.numNetworks,) and np.all(np.isfinite(per_row)) and np.isfinite(loo["elpd_loo"]) and np.isfinite(waic["elpd_waic"])
        fits[tag] = (mse, loo, p.numNetworks, hist["steps"])
        print(f"[student] {tag} fit: {p.numNetworks} networks after {hist['steps']} pre-training steps, clean held-out MSE against the teacher {mse:.5f}, "
              f"elpd_loo on {len(Xh)} contaminated rows ({int(badh.sum())} outliers) {loo['elpd_loo']:.1f} (se {loo['se']:.1f}), elpd_waic {waic['elpd_waic']:.1f}")
    cmp_ = predictor.compareLoo(fits["student"][1], fits["gaussian"][1])
    print(f"[student] compareLoo(student, gaussian): elpd_diff {cmp_['elpd_diff']:.1f}, se_diff {cmp_['se_diff']:.1f}")
    assert fits["student"][0] < fits["gaussian"][0]
    assert cmp_["elpd_diff"] > 0
