"""GPU: WeibullLikelihood (TBNN_LIK_WEIBULL) -- times to an event with right-censored rows, the censoring flag in the SIGN of the target,
log link on the scale and a fixed shape k; with t = |y| and u = (t e^-f)^k an event gives log k + (k - 1) log t - k f - u and a censored
row -u, per (row, output) -- on every kernel family: the narrow fast3 and fast kernels and their one-launch trajectory kernel, mid, tall
and wide (the VALU last layer of one or two outputs and the MFMA output tile of 3 .. 16), each likelihood path of the layered family
(k_lay_tail, k_lay_last, k_lay_lik) and the generic kernel.  Against fp64 (the cases and the reference are tests/weibull_ref.py's: the
data term stated there, everything else the oracle's): the value with its constant, the gradient per tensor, the forward outputs, an
injected weight transition with both decisions (log u placed on either side of the reference's log accept ratio, two bands away), a hyper
transition, every launch repeated bit for bit.  Then: the trajectory kernel, row weights, scale equivariance, the exponential limit
against a TBNN_LIK_GAMMA chain and the oracle's Gamma, the sign cases, refusals, trainChains against solo runs, pre-training, a
row-sharded chain on the stub collective library, and an end-to-end fit with and without the censoring flags.

Bands: the project's -- value 4e-6 relative, gradient 1e-4 of each tensor's largest entry (floor 1e-3), log accept ratio
2e-2 + 1e-4 |lar| + 4e-7 |logp|.  tests/test_weibull_host.py (CPU arithmetic only) shows that the kernel's own formula in fp32 stays
inside them at every case here (value gaps to 2.6e-7, gradient gaps to 3.6e-6), so no case has a band of its own.
Targets: event and censoring times drawn from the model around the network's OWN untrained log-scales (f0 + 0.3 z: u is of order 1, the
log-posterior a few hundred to 4e4, so the relative bands are tight in absolute terms and the event-only parts of the term count; 55 -
78 % events per case), one all-event and one all-censored dataset; k is spread over {0.5, 1, 1.5, 3}.  The injected transition takes ten
times student_ref's step: the reference's log accept ratio is 6e-5 .. 14 and the proposal moves theta by 4e-3 .. 6e-2, which the state
checks (1e-5, 2e-6) resolve hundreds of times over; the tests assert that margin.

Scale equivariance (test_scale_equivariance), a check of the log link that needs no reference for the likelihood: t e^-f is unchanged by
Y -> c Y (signs kept) together with b_last += log c, so the data term's gradient stays (inside the gradient band: c Y and b + log c are
rounded to fp32) and the data term shifts by -(weighted number of event elements) log c: per event element (k - 1) log c - k log c, per
censored element nothing.  The priors see the moved bias: their part of the change, on the last bias alone, is taken off with the
oracle's prior gradient.

End-to-end fit (test_fit_knows_the_censoring), measured on an MI355X: see NOTES.md."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import optim_ref as R
import tbnn_oracle as o
import weibull_ref as wr
from tensor_checks import layers_of, tensor_errs, tensors
from test_gpu_freerun import SEED

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FUSED = {"fast3": "", "fast": "fast3", "mid": "fast3,fast,tall,wide", "tall": "fast3,fast,mid,wide", "wide": "fast3,fast,mid,tall"}
CASES = {k: v for k, v in wr.CASES.items() if v[4] != "traj"}
NET = [1, 16, 16, 1]                                              # the network(...) of the trainChains and end-to-end tests (tanh)
LIK = wr.LIK_WEIBULL


def job(spec, lik=LIK, skip="", weighted=False):
    j = {"layers": [list(l) for l in layers_of(spec)], "likelihood": lik, "skip": skip, "flags": ""}
    if weighted:
        j["weighted"] = True
    return j


def jit_jobs():
    """the run-time instantiations this module asks for (jit.prebuild's job format)"""
    jobs = []
    for dims, _n, act, prior, fam, _env, _k, _kind in wr.CASES.values():
        if fam in FUSED:
            jobs.append(job(wr.make_spec(dims, act, prior), skip=FUSED[fam]))
        elif fam == "traj":
            jobs.append(job(wr.make_spec(dims, act, prior)))
    c = wr.CASES["fast3"]
    jobs.append(job(wr.make_spec(c[0], c[2], c[3]), weighted=True))
    c = wr.CASES["mid10"]
    jobs.append(job(wr.make_spec(c[0], c[2], c[3]), skip=FUSED[c[4]], weighted=True))
    c = wr.CASES["fast3_two_outputs"]
    jobs.append(job(wr.make_spec(c[0], c[2], c[3]), lik=o.LIK_GAMMA))                            # the exponential limit's Gamma chain
    jobs.append(job(wr.make_spec(NET, o.ACT_TANH, o.PRIOR_CAUCHY)))
    jobs.append(job(wr.make_spec(NET, o.ACT_TANH, o.PRIOR_CAUCHY), lik=o.LIK_FIXED_GAUSSIAN))      # the predictors' forward chains
    return [j for i, j in enumerate(jobs) if j not in jobs[:i]]


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """compile this module's run-time shapes side by side before any test touches the GPU (cached: a second run compiles nothing); every
    one went through the checked compile: the MFMA hazard check is clean for each new instantiation"""
    from tensorbnn_amd import jit
    jobs = jit_jobs()
    assert len(jobs) <= 16
    assert jit.prebuild(jobs, processes=min(16, len(jobs))) == len(jobs)
    for j in jobs:
        os.environ["TBNN_JIT_SKIP"], before = j["skip"], os.environ.get("TBNN_JIT_SKIP")
        try:
            so = jit.build([tuple(l) for l in j["layers"]], j["likelihood"], weighted=bool(j.get("weighted")))
        finally:
            if before is None:
                del os.environ["TBNN_JIT_SKIP"]
            else:
                os.environ["TBNN_JIT_SKIP"] = before
        st = jit.lint_status(so)
        assert "listing checked" in st and "disassembly clean" in st, (j, st)


def gaps(spec, lp, g, lp64, g64):
    """(value error / max(|lp64|, 1), per tensor: gradient error / max(|g64|_inf, 1e-3))"""
    return abs(lp - lp64) / max(abs(lp64), 1.0), tensor_errs(spec, g, g64, 1e-3)


def check_value_gradient(tag, lp, g, spec, ref64):
    ev, eg = gaps(spec, lp, g, *ref64)
    print(f"[weibull] {tag}: logp {lp:.9g} (fp64 {ref64[0]:.9g}) err {ev:.3e} of band 4e-6; gradient err max {max(eg):.3e} of band 1e-4")
    assert np.isfinite(lp) and np.all(np.isfinite(g))
    assert ev <= 4e-6, (tag, lp, ref64[0])
    assert max(eg) <= 1e-4, (tag, eg)


def make_chain(native, monkeypatch, name, spec, k, lik=LIK, word=",weibull;", **kw):
    fam, env = wr.CASES[name][4], wr.CASES[name][5]
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    kw = dict(likelihood=lik, lik_df=k, **kw)
    if fam in FUSED:
        monkeypatch.setenv("TBNN_JIT_SKIP", FUSED[fam])
        ch = native.Chain(layers_of(spec), jit=True, **kw)
        assert ch.kernel_name.startswith(f"jit-{fam}<") and word in ch.kernel_name, ch.kernel_name
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
    spec, X, Y, theta, eta, k = wr.problem(name)
    ch = make_chain(native, monkeypatch, name, spec, k)
    ch.set_data(X, Y)
    lp, g, st = ch.logp_grad(theta, eta)
    for _ in range(2):
        lp2, g2, st2 = ch.logp_grad(theta, eta)
        assert lp2 == lp and st2 == st and np.array_equal(g, g2)
    m = min(500, X.shape[0])
    f = ch.forward(X[:m], theta)
    assert np.array_equal(f, ch.forward(X[:m], theta))
    ch.close()
    check_value_gradient(name, lp, g, spec, wr.ref64(name))
    # stat is the data term with its constant (as Poisson's and Gamma's): -sum (k d f + u) - C, and logp minus it the priors
    f64 = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    data64 = wr.data_log_prob(spec, k, f64, Y, np.float64)[0]
    assert abs(st - data64) <= 4e-6 * abs(data64), (st, data64)
    prior = float(wr.ref64(name)[0] - data64)
    assert abs((lp - st) - prior) <= 4e-6 * max(abs(lp), 1.0)
    assert f.shape == (spec.layers[-1].out_dim, m)
    assert np.abs(f - f64[:, :m]).max() <= 1e-4 * max(1.0, np.abs(f64).max())


@pytest.mark.parametrize("name", list(CASES))
def test_transitions(native, monkeypatch, name):
    spec, X, Y, theta, eta, k = wr.problem(name)
    rng = np.random.default_rng(4)
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    ch = make_chain(native, monkeypatch, name, spec, k, seed=SEED, chain_id=2)
    ch.set_data(X, Y)
    lp64 = wr.ref64(name)[0]
    eps = wr.step_size(name)
    ref = wr.weight_step(spec, k, theta, eta, X, Y, eps, 4, p0, -1e30, np.float64)
    tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
    # log u on either side of the reference's log accept ratio, two bands away: the kernel's rounding cannot flip the decision
    for log_u, accept in ((ref.log_accept_ratio - 2 * tol, True), (ref.log_accept_ratio + 2 * tol, False)):
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hmc_step(eps, 4, p0=p0, log_u=log_u)
        print(f"[weibull] {name}: lar {out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g}, band {tol:.3g}), logp {lp64:.6g}")
        assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= tol
        assert bool(out["accepted"]) == accept
        assert abs(out["logp_old"] - lp64) <= 4e-6 * max(abs(lp64), 1.0)
        assert abs(out["logp_new"] - ref.logp_new) <= 4e-6 * max(abs(ref.logp_new), 1.0)
        want = ref.theta_proposed if accept else theta
        assert np.abs(ch.get_state() - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
        # ... which tells the two decisions apart: the proposal is at least 100 tolerances away from the start
        assert np.abs(ref.theta_proposed - theta).max() >= max(wr.MIN_MOVE, 50 * 1e-5 * max(1.0, np.abs(want).max()))
        if not accept:
            assert np.array_equal(ch.get_state(), theta)
        again = ch.set_state(theta) or ch.hmc_step(eps, 4, p0=p0, log_u=log_u)
        assert again["log_accept_ratio"] == out["log_accept_ratio"] and again["logp_new"] == out["logp_new"]
    # the hyper transition: the layer priors only (no likelihood hyper, no data term)
    ph = rng.standard_normal(spec.n_hypers).astype(np.float32)
    ch.set_state(theta); ch.set_hypers(eta)
    ch.logp_grad(theta, eta)
    out = ch.hyper_step(1e-4, 9, p0=ph, log_u=-1e30)
    ref = wr.hyper_step(spec, eta, theta, X, Y, 1e-4, 9, ph, -1e30, np.float64)
    assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= 2e-2 + 1e-3 * abs(ref.log_accept_ratio)
    assert np.allclose(ch.get_hypers(), ref.theta, rtol=1e-4, atol=1e-5)
    # after the accepted hyper transition the cached gradient is refreshed for the new priors: the next weight step starts from it
    eta2 = ch.get_hypers()
    lp_new, g_new, _ = ch.logp_grad(theta, eta2)
    check_value_gradient(name + " after the hyper step", lp_new, g_new, spec, wr.target_log_prob_and_grad(spec, k, theta, eta2, X, Y, np.float64))
    ch.close()


def test_trajectory_kernel(native, monkeypatch):
    """a small narrow problem takes the one-launch trajectory kernel; the traced run of the same transition (per-step kernels) agrees with
    fp64 step by step"""
    spec, X, Y, theta, eta, k = wr.problem("traj")
    monkeypatch.setenv("TBNN_TRAJ", "1")
    monkeypatch.setenv("TBNN_JIT_SKIP", "")
    ch = native.Chain(layers_of(spec), likelihood=LIK, lik_df=k, jit=True, seed=SEED)
    assert ch.kernel_name.startswith("jit-fast3<") and ",weibull;" in ch.kernel_name, ch.kernel_name
    ch.set_data(X, Y)
    lp, g, _ = ch.logp_grad(theta, eta)
    check_value_gradient("traj", lp, g, spec, wr.ref64("traj"))
    p0 = np.random.default_rng(5).standard_normal(spec.n_params).astype(np.float32)
    lp64 = wr.ref64("traj")[0]
    eps = wr.step_size("traj")
    for L in (1, 9):
        ref = wr.weight_step(spec, k, theta, eta, X, Y, eps, L, p0, -1e30, np.float64)
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hmc_step(eps, L, p0=p0, log_u=-1e30)
        assert ch.last_transition_path == "trajectory"
        tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
        print(f"[weibull] trajectory L={L}: lar {out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g})")
        assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= tol
        assert bool(out["accepted"]) == ref.accepted
        assert abs(out["logp_new"] - ref.logp_new) <= 4e-6 * max(abs(ref.logp_new), 1.0)
        np.testing.assert_allclose(ch.get_state(), ref.theta, rtol=2e-5, atol=2e-6)
        assert ref.accepted and np.abs(ref.theta - theta).max() >= wr.MIN_MOVE                   # (a moved state: 500 x the atol)
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
        assert L == 1 or np.ptp(tr64) > 100 * 4e-6 * np.abs(tr64).max()                        # (no constant series)
        assert abs(traced["log_accept_ratio"] - ref.log_accept_ratio) <= tol
    ch.close()


@pytest.mark.parametrize("name", ["fast3", "mid10", "lay_last"])
def test_row_weights(native, monkeypatch, name):
    spec, X, Y, theta, eta, k = wr.problem(name)
    n = min(600, X.shape[0])
    X, Y = X[:n], Y[:n]
    w = np.random.default_rng(21).integers(0, 4, n).astype(np.float32)
    vg = lambda Xs, Ys, ws=None: wr.target_log_prob_and_grad(spec, k, theta, eta, Xs, Ys, np.float64, ws)
    ch = make_chain(native, monkeypatch, name, spec, k)
    ch.set_data(X, Y)
    plain = ch.logp_grad(theta, eta)
    # a weight of 1 everywhere: the unweighted bits
    ch.set_row_weights(np.ones(n, np.float32))
    if wr.CASES[name][4] in FUSED:
        assert ",weibull,weighted;" in ch.kernel_name, ch.kernel_name
    ones = ch.logp_grad(theta, eta)
    assert ones[0] == plain[0] and ones[2] == plain[2] and np.array_equal(ones[1], plain[1])
    check_value_gradient(name + " weight 1", ones[0], ones[1], spec, vg(X, Y))
    # integer weights: the rows duplicated; weight 0: the row removed
    ch.set_row_weights(w)
    lp, g, st = ch.logp_grad(theta, eta)
    check_value_gradient(name + " weighted", lp, g, spec, vg(X, Y, w))
    idx = np.repeat(np.arange(n), w.astype(int))
    assert (w == 0).any() and idx.size < w.sum() + 1
    ch.set_row_weights(None)
    ch.set_data(X[idx], Y[idx])
    dup = ch.logp_grad(theta, eta)
    check_value_gradient(name + " duplicated", dup[0], dup[1], spec, vg(X[idx], Y[idx]))
    ev, eg = gaps(spec, lp, g, dup[0], dup[1].astype(np.float64))
    print(f"[weibull] {name}: weights vs duplicated rows: value {ev:.3e}, gradient {max(eg):.3e}")
    assert ev <= 4e-6 and max(eg) <= 1e-4, (ev, eg)
    # clearing the weights brings the unweighted bits back
    ch.set_data(X, Y); ch.set_row_weights(w); ch.set_row_weights(None)
    back = ch.logp_grad(theta, eta)
    assert back[0] == plain[0] and np.array_equal(back[1], plain[1])
    ch.close()


@pytest.mark.parametrize("name", ["fast3_two_outputs", "lay_last"])
def test_scale_equivariance(native, monkeypatch, name):
    """Y -> c Y (signs kept) with b_last += log c: the data term's gradient stays inside the gradient band and the data term moves by
    -(weighted number of event elements) log c inside the value band (the module docstring); the likelihood's reference is not involved.
    Unweighted and under row weights."""
    spec, X, Y, theta, eta, k = wr.problem(name)
    c = 2.5
    n, d_out = X.shape[0], spec.layers[-1].out_dim
    spans = list(tensors(spec))
    b0, b1 = spans[-1]                                               # the last layer's bias
    theta_c = theta.copy()
    theta_c[b0:b1] += np.float32(math.log(c))
    Yc = (Y.astype(np.float64) * c).astype(np.float32)
    assert np.array_equal(Yc > 0, Y > 0)
    # the priors' part of the change: the last bias alone, by the oracle's prior gradient in fp64
    l, h4 = spec.layers[-1], eta[4 * (len(spec.layers) - 1):4 * len(spec.layers)].astype(np.float64)
    W1, B1 = o.unflatten(spec, theta.astype(np.float64))[-1]
    W2, B2 = o.unflatten(spec, theta_c.astype(np.float64))[-1]
    dprior = (o.prior_grad(l, h4, W2, B2, np.float64)[1] - o.prior_grad(l, h4, W1, B1, np.float64)[1]).reshape(-1)
    ch = make_chain(native, monkeypatch, name, spec, k)
    for w in (None, np.random.default_rng(22).integers(0, 4, n).astype(np.float32)):
        ch.set_data(X, Y)
        ch.set_row_weights(w)
        lp1, g1, st1 = ch.logp_grad(theta, eta)
        ch.set_data(X, Yc)
        ch.set_row_weights(w)
        lp2, g2, st2 = ch.logp_grad(theta_c, eta)
        g2d = g2.astype(np.float64)
        g2d[b0:b1] -= dprior
        eg = tensor_errs(spec, g2d, g1.astype(np.float64), 1e-3)
        events = float(np.sum((Y > 0) * (1.0 if w is None else w.astype(np.float64)[:, None])))
        shift = -events * math.log(c)
        ev = abs((st2 - st1) - shift) / max(abs(st1), 1.0)
        print(f"[weibull] {name}{'' if w is None else ' weighted'}: Y -> {c} Y, b_last += log {c}: gradient moves by {max(eg):.3e} of band 1e-4; data term "
              f"{st1:.9g} -> {st2:.9g}, shift {st2 - st1:.9g} (expected {shift:.9g}, {events:g} event elements) err {ev:.3e} of band 4e-6")
        assert max(eg) <= 1e-4, eg
        assert ev <= 4e-6
    ch.close()


@pytest.mark.parametrize("name", ["fast3_two_outputs", "all_events"])
def test_exponential_limit_equals_gamma_of_shape_one(native, monkeypatch, name):
    """k = 1 with every row an event is the exponential model, and so is TBNN_LIK_GAMMA of shape 1: on the same data value, statistic and
    gradient of the two chains agree inside the bands, and both with the oracle's Gamma in fp64"""
    spec, X, Y, theta, eta, _k = wr.problem(name)
    Y = np.abs(Y)
    ch = make_chain(native, monkeypatch, name, spec, 1.0)
    ch.set_data(X, Y)
    lw, gw, sw = ch.logp_grad(theta, eta)
    ch.close()
    gch = make_chain(native, monkeypatch, name, spec, 1.0, lik=o.LIK_GAMMA, word=",gamma;")
    gch.set_data(X, Y)
    lg, gg, sg = gch.logp_grad(theta, eta)
    gch.close()
    dims, _n, act, prior = wr.CASES[name][:4]
    gspec = o.make_spec(dims, act, prior, o.LIK_GAMMA, o.ACT_NONE, lik_df=1.0)
    ref = o.target_log_prob_and_grad(gspec, theta, eta, X, Y, np.float64)
    ref = (float(ref[0]), np.asarray(ref[1], dtype=np.float64))
    mine = wr.target_log_prob_and_grad(spec, 1.0, theta, eta, X, Y, np.float64)
    assert math.isclose(mine[0], ref[0], rel_tol=1e-12) and np.allclose(mine[1], ref[1], rtol=1e-9, atol=1e-10)
    check_value_gradient(name + " Weibull k = 1 against the oracle's Gamma", lw, gw, spec, ref)
    check_value_gradient(name + " Gamma a = 1 against the oracle's Gamma", lg, gg, spec, ref)
    ev, eg = gaps(spec, lw, gw, lg, gg.astype(np.float64))
    print(f"[weibull] {name}: k = 1, all events, against the Gamma chain of shape 1: value {ev:.3e}, gradient {max(eg):.3e}, "
          f"data terms {sw:.9g} and {sg:.9g}")
    assert ev <= 4e-6 and max(eg) <= 1e-4
    assert abs(sw - sg) <= 4e-6 * abs(sg)


@pytest.mark.parametrize("name", ["generic", "fast3_two_outputs"])
def test_sign_cases(native, monkeypatch, name):
    """a censored row and an event row at the same |y| differ by exactly what the definition says.  The data is well conditioned (u of
    order 1: tests/weibull_ref.py), so the data term is a few thousand and every tolerance below is far smaller than the quantity it
    judges: two data terms, each within the value band, bound the error of their difference by 8e-6 |data term| -- hundredths, against
    differences of units (one row) and thousands (all rows); two gradients, each within the gradient band, bound the error of a
    difference of last-bias gradients by 2e-4 of that tensor's largest entry -- against k per output.  The test asserts first that these
    margins hold, so that a kernel which ignored the sign of the flipped row could not pass."""
    spec, X, Y, theta, eta, k = wr.problem(name)
    ch = make_chain(native, monkeypatch, name, spec, k)
    f64 = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)            # [d_out, n]
    t = np.abs(Y.astype(np.float64)).T
    part = math.log(k) + (k - 1.0) * np.log(t) - k * f64                                        # an event's surplus over a censored row
    b0, b1 = list(tensors(spec))[-1]                                                           # the last layer's bias
    ch.set_data(X, Y)
    lp0, g0, st0 = ch.logp_grad(theta, eta)
    ch.set_data(X, np.abs(Y))
    _lp, g_ev, st_ev = ch.logp_grad(theta, eta)
    ch.set_data(X, -np.abs(Y))
    _lp, g_ce, st_ce = ch.logp_grad(theta, eta)
    big = max(abs(st_ev), abs(st_ce), abs(st0))
    tol_st = 8e-6 * big
    tol_g = 2e-4 * max(1e-3, np.abs(g_ev[b0:b1]).max(), np.abs(g_ce[b0:b1]).max())
    want = float(part.sum())
    print(f"[weibull] signs {name}: data term all events {st_ev:.9g}, all censored {st_ce:.9g}, difference {st_ev - st_ce:.9g} (definition "
          f"{want:.9g}, tolerance {tol_st:.3g}); last-bias gradients differ by {np.array2string(g_ce[b0:b1] - g_ev[b0:b1], precision=4)} "
          f"(definition {k * X.shape[0]:g} per output, tolerance {tol_g:.3g})")
    assert abs(want) > 100 * tol_st and abs((st_ev - st_ce) - want) <= tol_st
    # every element's delta is k (u - d): all censored against all events adds k per row to each output's bias gradient
    assert k * X.shape[0] > 100 * tol_g and np.all(np.abs((g_ce[b0:b1] - g_ev[b0:b1]) - k * X.shape[0]) <= tol_g)
    # ONE row flipped from event to censored, the row whose surplus is largest in magnitude among the rows that are events in every output
    ev_rows = np.flatnonzero(np.all(Y > 0, axis=1))
    row = int(ev_rows[np.argmax(np.abs(part[:, ev_rows].sum(axis=0)))])
    Y1 = Y.copy()
    Y1[row] = -Y1[row]
    ch.set_data(X, Y1)
    lp1, g1, st1 = ch.logp_grad(theta, eta)
    ch.close()
    want1 = float(part[:, row].sum())
    tol_g = 2e-4 * max(1e-3, np.abs(g0[b0:b1]).max(), np.abs(g1[b0:b1]).max())
    print(f"[weibull] signs {name}: row {row} censored: data term moves by {st0 - st1:.6g} (definition {want1:.6g}, tolerance {tol_st:.3g}); "
          f"last-bias gradient by {np.array2string(g1[b0:b1] - g0[b0:b1], precision=4)} (definition {k:g}, tolerance {tol_g:.3g})")
    assert abs(want1) > 10 * tol_st and abs((st0 - st1) - want1) <= tol_st
    assert abs((lp0 - lp1) - want1) <= 8e-6 * max(abs(lp0), 1.0)
    assert k > 10 * tol_g and np.all(np.abs((g1[b0:b1] - g0[b0:b1]) - k) <= tol_g)
    check_value_gradient("signs: one row censored", lp1, g1, spec, wr.target_log_prob_and_grad(spec, k, theta, eta, X, Y1, np.float64))


def test_refusals(native, monkeypatch):
    spec, X, Y, theta, eta, k = wr.problem("generic")
    layers = layers_of(spec)
    for df in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(native.TbnnError, match="lik_df"):
            native.Chain(layers, likelihood=LIK, lik_df=df, kernel=native.KERNEL_GENERIC)
        with pytest.raises(native.TbnnError, match="lik_df"):
            native.ChainGroup(layers, 2, likelihood=LIK, lik_df=df, kernel=native.KERNEL_GENERIC)
    with pytest.raises(native.TbnnError, match="no activation"):
        native.Chain(layers[:-1] + [layers[-1][:2] + (native.ACT_SIGMOID,) + layers[-1][3:]], likelihood=LIK, lik_df=3.0, kernel=native.KERNEL_GENERIC)
    for unknown in (15, 17):
        with pytest.raises(native.TbnnError, match="unknown likelihood"):
            native.Chain(layers, likelihood=unknown, lik_df=3.0, kernel=native.KERNEL_GENERIC)
    thetas = (theta[None] + 0.01 * np.random.default_rng(1).standard_normal((4, spec.n_params))).astype(np.float32)
    # a Weibull handle: targets that are zero, not finite or outside [2^-100, 2^100] in magnitude are refused, and the handle keeps its
    # rows; the shape is the descriptor's, the setter is refused; the CRPS and the entropy split are refused by name
    ch = native.Chain(layers, likelihood=LIK, lik_df=k, kernel=native.KERNEL_GENERIC)
    ch.set_data(X, Y)
    before = ch.logp_grad(theta, eta)
    one = np.float32(1)
    up, dn = one + np.float32(2.0 ** -23), one - np.float32(2.0 ** -24)
    for bad in (0.0, -0.0, float("nan"), float("inf"), -float("inf"), np.float32(2.0 ** 100) * up, -np.float32(2.0 ** 100) * up,
                np.float32(2.0 ** -100) * dn, -np.float32(2.0 ** -100) * dn, np.float32(1e-45)):
        Yb = Y.copy()
        Yb[7, 1] = bad
        with pytest.raises(native.TbnnError, match=r"signed time.*2\^-100 <= \|y\| <= 2\^100"):
            ch.set_data(X, Yb)
        after = ch.logp_grad(theta, eta)
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    # the ends of the admitted range are staged, with either sign (at the floor u = (t e^-f)^k is 0 or tiny: a finite value)
    for edge in (2.0 ** 100, -2.0 ** 100, 2.0 ** -100, -2.0 ** -100):
        Yb = Y.copy()
        Yb[7, 1] = np.float32(edge)
        ch.set_data(X, Yb)
        if abs(edge) < 1.0:
            top = ch.logp_grad(theta, eta)
            assert np.isfinite(top[0]) and np.all(np.isfinite(top[1])) and top[0] != before[0]
    ch.set_data(X, Y)
    after = ch.logp_grad(theta, eta)
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    with pytest.raises(native.TbnnError):
        ch.set_row_weights(-np.ones(X.shape[0], np.float32))
    assert ch.logp_grad(theta, eta)[0] == before[0]
    with pytest.raises(native.TbnnError, match="descriptor"):
        ch.set_lik_df(5.0)
    with pytest.raises(native.TbnnError, match="TBNN_LIK_WEIBULL is not built"):
        ch.ensemble_crps(thetas, Y=Y[:64], X=X[:64])
    with pytest.raises(native.TbnnError, match="TBNN_LIK_WEIBULL"):
        ch.ensemble_uncertainty(thetas, X=X[:64])
    per_net, rows = ch.ensemble_loglik(thetas, Y=Y[:64], X=X[:64])
    assert np.all(np.isfinite(per_net)) and np.all(np.isfinite(rows))
    assert ch.logp_grad(theta, eta)[0] == before[0]
    ch.close()
    # a handle of another likelihood: judging under Weibull needs the setter first, and the setter a finite shape > 0
    gch = native.Chain(layers, likelihood=o.LIK_FIXED_GAUSSIAN, fixed_sd=1.0, kernel=native.KERNEL_GENERIC)
    with pytest.raises(native.TbnnError, match="tbnn_set_lik_df"):
        gch.ensemble_loglik(thetas, Y=Y[:64], X=X[:64], likelihood=LIK)
    with pytest.raises(native.TbnnError, match="tbnn_set_lik_df"):
        gch.ensemble_loo(thetas, Y=Y[:64], X=X[:64], likelihood=LIK)
    with pytest.raises(native.TbnnError, match="tbnn_set_lik_df"):
        gch.ensemble_predictive(thetas, probs=[0.5], X=X[:64], likelihood=LIK)
    gch.set_lik_df(k)
    per_net, rows = gch.ensemble_loglik(thetas, Y=Y[:64], X=X[:64], likelihood=LIK)
    assert np.all(np.isfinite(per_net)) and np.all(np.isfinite(rows))
    with pytest.raises(native.TbnnError, match="TBNN_LIK_WEIBULL is not built"):
        gch.ensemble_crps(thetas, Y=Y[:64], X=X[:64], likelihood=LIK)
    with pytest.raises(native.TbnnError, match="TBNN_LIK_WEIBULL"):
        gch.ensemble_uncertainty(thetas, X=X[:64], likelihood=LIK)
    gch.close()


# ---------------------------------------------------------------------------------------------------------------------- pre-training
def test_pretraining_against_the_restatement(native, monkeypatch):
    """Chain.optimize for a few steps against the Adam / AMSGrad restatement of tests/optim_ref.py driven by the reference's gradient: the
    checked objectives to the value band, the last step's gradient to the gradient band, theta to 8 x the restatement's own fp32 gap"""
    name, steps = "fast3_two_outputs", 6
    spec, X, Y, theta0, eta, k = wr.problem(name)

    def run(dtype):
        dt = dtype
        theta = np.asarray(theta0, dtype=dt)
        m = v = vhat = np.zeros_like(theta)
        trace, g = [], None
        for i in range(steps):
            lp, g = wr.target_log_prob_and_grad(spec, k, theta, eta, X, Y, dt)
            trace.append(float(lp))
            theta, m, v, vhat = R.adam_step(theta, g, m, v, vhat, i + 1, R.LR, dtype=dt)
        trace.append(float(wr.target_log_prob_and_grad(spec, k, theta, eta, X, Y, dt)[0]))
        return np.asarray(trace), theta, g

    ch = make_chain(native, monkeypatch, name, spec, k)
    ch.set_data(X, Y); ch.set_state(theta0); ch.set_hypers(eta)
    out = ch.optimize(steps, lr=R.LR, check_every=1, keep="last")
    th, st = ch.get_state(), ch.optim_state()
    ch.set_state(theta0)
    again = ch.optimize(steps, lr=R.LR, check_every=1, keep="last")
    assert np.array_equal(again["trace"], out["trace"]) and np.array_equal(ch.get_state(), th)
    ch.close()
    tr64, th64, g64 = run(np.float64)
    _tr32, th32, _g32 = run(np.float32)
    print(f"[weibull] optimize: trace {out['trace'][0]:.6f} -> {out['trace'][-1]:.6f} (fp64 {tr64[0]:.6f} -> {tr64[-1]:.6f})")
    assert out["steps_done"] == steps and out["diverged"] == 0 and tr64[-1] > tr64[0]
    assert np.all(np.abs(out["trace"] - tr64) <= 4e-6 * np.maximum(np.abs(tr64), 1.0)), (out["trace"], tr64)
    assert max(tensor_errs(spec, st["g"], g64, 1e-3)) <= 1e-4
    gap = np.abs(th32.astype(np.float64) - th64).max()
    assert np.abs(th.astype(np.float64) - th64).max() <= 8 * gap, (np.abs(th - th64).max(), gap)


# ---------------------------------------------------------------------------------------------------------------------- row-sharded chain
def test_row_shard_two_ranks(tmp_path, native, monkeypatch):
    """world 2 on the stub collective library (tests/stubccl/worker_weibull.py: two fresh child processes, each under its own time limit):
    the statistic is all-reduced, every rank taking the constant of its own rows off first, so the sharded chain takes the unsharded
    chain's decisions and reaches its state, within the sharding band of tests/test_gpu_multirank.py"""
    from conftest import wait_gpu_quiet
    from test_gpu_multirank import build_stub
    sys.path.insert(0, os.path.join(HERE, "stubccl"))
    import worker_weibull as ws
    wait_gpu_quiet()
    env = dict(os.environ, TBNN_RCCL_LIB=build_stub(), TBNN_JIT="0", TBNN_PREBUILD_JIT="0")
    idfile = str(tmp_path / "shard.id")
    procs = []
    for rk in range(2):
        out = str(tmp_path / f"shard_{rk}.npz")
        procs.append((out, subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "stubccl", "worker_weibull.py"), str(rk), "2", idfile, out],
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
        k = ws.SHAPES[name][5]
        ref = ws.chain_of(name, spec)
        ref.set_data(X, Y); ref.set_state(theta); ref.set_hypers(eta)
        lp0, g0, st0 = ref.logp_grad(theta, eta)
        p0 = np.random.default_rng(5).standard_normal(spec.n_params).astype(np.float32)
        outs = [ref.hmc_step(1e-5, 4, p0=p0, log_u=-1e30, trace=True), ref.hmc_step(1e-5, 3)]
        th_ref = ref.get_state()
        n = X.shape[0]
        rows = [tuple(rk[name + "_rows"]) for rk in ranks]
        assert rows[0][0] == 0 and rows[0][1] == rows[1][0] and rows[1][1] == n, rows
        for lo, hi in rows:
            assert (Y[lo:hi] > 0).any() and (Y[lo:hi] < 0).any()                              # both kinds of row on every rank
        for rk in ranks:
            assert str(rk[name + "_kernel"]) == ref.kernel_name
            assert abs(float(rk[name + "_lp"]) - lp0) <= 1e-7 * abs(lp0) + 1e-6
            assert abs(float(rk[name + "_st"]) - st0) <= 1e-9 * abs(st0)
            np.testing.assert_allclose(rk[name + "_g"], g0, rtol=0, atol=4e-6 * np.abs(g0).max())
            np.testing.assert_allclose(rk[name + "_trace"], outs[0]["trace_logp"], rtol=1e-7, atol=1e-5)
            for j in range(2):
                assert abs(rk[name + "_lar"][j] - outs[j]["log_accept_ratio"]) <= 2e-3 + 1e-5 * abs(outs[j]["log_accept_ratio"])
                assert rk[name + "_acc"][j] == outs[j]["accepted"]
            np.testing.assert_allclose(rk[name + "_theta"], th_ref, rtol=0, atol=2e-6 * max(1.0, np.abs(th_ref).max()))
        np.testing.assert_array_equal(ranks[0][name + "_theta"], ranks[1][name + "_theta"])       # every rank took the same decisions
        np.testing.assert_array_equal(ranks[0][name + "_g"], ranks[1][name + "_g"])
        assert float(ranks[0][name + "_lp"]) == float(ranks[1][name + "_lp"])
        check_value_gradient("shard " + name, float(ranks[0][name + "_lp"]), ranks[0][name + "_g"], spec,
                             wr.target_log_prob_and_grad(spec, k, theta, eta, X, Y, np.float64))
        ref.close()


# ---------------------------------------------------------------------------------------------------------------------- network / train
SHAPE = 1.5
CENSOR = 1.5 ** (1.0 / SHAPE)              # censoring scale over event scale: P(censored) = 1 / (1 + CENSOR^SHAPE) = 0.4


def log_scale(x):
    """a smooth log-scale: scales from 1 to 8"""
    return math.log(8.0) * (0.5 + 0.5 * np.sin(1.5 * x))


def survival_rows(n, seed, censor=True):
    """x ~ U(-2, 2), the event time Weibull of shape 1.5 around exp(log_scale(x)), the censoring time the same model times CENSOR (about
    40 % of the rows censored): (X, times [n, 1], observed [n, 1])"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, 1)).astype(np.float32)
    lam = np.exp(log_scale(X.astype(np.float64)))
    T = np.maximum(lam * rng.weibull(SHAPE, (n, 1)), 1e-30)
    Cn = np.maximum(CENSOR * lam * rng.weibull(SHAPE, (n, 1)), 1e-30)
    if not censor:
        return X, T.astype(np.float32), np.ones((n, 1), bool)
    return X, np.minimum(T, Cn).astype(np.float32), T <= Cn


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
    from tensorbnn_amd.likelihood import WeibullLikelihood
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, t, d = survival_rows(400, 1)
    Xv, tv, dv = survival_rows(200, 2)
    Y, Yv = WeibullLikelihood.encode(t, d), WeibullLikelihood.encode(tv, dv)
    C, EPOCHS = 3, 14
    lik = lambda: WeibullLikelihood(shape=SHAPE)
    grp_net = make_net(X, Y, Xv, Yv)
    rec = grp_net.trainChains(C, EPOCHS, 4, lik(), adjustHypers=True, folderName="multi", networksPerFile=2)
    assert len(rec) == EPOCHS and all(len(rc["main"]) == C for rc in rec)
    for c in range(C):
        net = make_net(X, Y, Xv, Yv, chain_id=c)
        solo = net.train(EPOCHS, 4, lik(), adjustHypers=True, folderName="solo%d" % c, networksPerFile=2, verbose=False)
        assert net._chain.kernel_name.startswith("jit-fast3<") and ",weibull;" in net._chain.kernel_name, net._chain.kernel_name
        for rg, rs in zip(rec, solo):
            assert rg["eps"][c] == rs["eps"] and rg["L"][c] == rs["L"]
            for key in ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new", "sjd"):
                assert rg["main"][c][key] == rs["main"][key], (c, rg["iter"], key)
            assert rg["hyper"][c]["log_accept_ratio"] == rs["hyper"]["log_accept_ratio"]
            assert rg["hyper_step_size"][c] == rs["hyper_step_size"]


def test_fit_knows_the_censoring(tmp_path, monkeypatch, native):
    """[1, 16, 16, 1] on 400 rows whose event times are Weibull of shape 1.5 around a smooth scale (1 .. 8), about 40 % of them
    right-censored; pretrain then a short train (tests/test_gpu_gamma.py's recipe), once with the censoring flags and once with the same
    times handed over as events.  On 300 held-out inputs the fit that knows the censoring recovers the true log-scale with the smaller mean
    squared error.  Only that inequality is asserted; both errors and the coverage of the 90 % predictive interval on held-out event rows
    are printed (NOTES.md records them)."""
    from tensorbnn_amd.likelihood import WeibullLikelihood
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, t, d = survival_rows(400, 1)
    Xv, tv, dv = survival_rows(200, 2)
    Xh, th_, _dh = survival_rows(300, 3, censor=False)                  # held-out rows, every one an observed event
    print(f"[weibull] fit: {100 * (1 - d.mean()):.1f} % of the {len(X)} training rows are censored")
    truth = log_scale(Xh.astype(np.float64))[:, 0]
    lik = WeibullLikelihood(shape=SHAPE)
    mse = {}
    for tag, Y, Yv in (("censoring known", WeibullLikelihood.encode(t, d), WeibullLikelihood.encode(tv, dv)),
                       ("times as events", WeibullLikelihood.encode(t, True), WeibullLikelihood.encode(tv, True))):
        net = make_net(X, Y, Xv, Yv)
        hist = net.pretrain(lik, cycles=2, epochs=400, learningRate=0.01, verbose=False)
        net.train(70, 4, lik, folderName=tag.replace(" ", "_"), networksPerFile=1, verbose=False)
        assert ",weibull;" in net._chain.kernel_name, net._chain.kernel_name
        p = predictor(str(tmp_path / tag.replace(" ", "_")) + "/", likelihood=lik)
        fm, _fv = p.predictMoments(Xh, transform="none")
        lower, median, upper = p.predictiveInterval(Xh, level=0.9)
        yh = th_[:, 0].astype(np.float64)
        cover = float(np.mean((yh >= lower[0]) & (yh <= upper[0])))
        mse[tag] = float(np.mean((fm[0] - truth) ** 2))
        assert np.all(np.isfinite(fm)) and np.all(lower > 0) and np.all(lower <= median) and np.all(median <= upper)
        print(f"[weibull] fit, {tag}: {p.numNetworks} networks after {hist['steps']} pre-training steps; on {len(Xh)} held-out inputs: mean squared "
              f"error of the log-scale {mse[tag]:.4f} (bias {float(np.mean(fm[0] - truth)):+.3f}); 90 % predictive interval covers "
              f"{cover:.3f} of the held-out event rows")
    assert mse["censoring known"] < mse["times as events"], mse
