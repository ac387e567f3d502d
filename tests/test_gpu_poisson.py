"""GPU: PoissonLikelihood (TBNN_LIK_POISSON) -- counts under a log link, log p(y | f) = y f - exp(f) - lgamma(y + 1) -- on every kernel
family: the narrow fast3 and fast kernels and their one-launch trajectory kernel, mid, tall and wide (the VALU last layer of one or two
outputs and the MFMA output tile of 3 .. 16), each likelihood path of the layered family (k_lay_tail, k_lay_last, k_lay_lik) and the
generic kernel.  Against the fp64 oracle (o.target_log_prob_and_grad under LIK_POISSON): value (with the
constant C = sum lgamma(y + 1) the library computes once per data staging), gradient per tensor, forward log-rates, an injected weight
transition with both decisions, a hyper transition, every launch repeated bit for bit.  Then: overflowing proposals, row weights, refused
targets and descriptors, trainChains against solo runs, a Gaussian and a Poisson chain side by side, the ensemble reductions, a
row-sharded chain on the stub collective library, and an end-to-end fit judged by its held-out log predictive density.

Bands: those of tests/test_gpu_categorical.py.  The inputs keep the log-rates in about [-3, 6].  The one "large rate" case has log-rates
up to 20 (rates to 5e8): there an fp32 evaluation of the log-rate itself (rounding ~1e-7 |f| sqrt(fan-in), i.e. ~1e-5 absolute at f = 20)
moves exp(f) by ~1e-5 relative, which is more than the 4e-6 band of the value.  `test_reference_in_fp32_stays_inside_the_bands` (CPU
arithmetic only) evaluates the oracle's fp32 arm (the fp64 reference's own formula in fp32) and asserts that it stays inside the project's
bands for every normal
case; for the large-rate case it measures the fp32-vs-fp64 gap of that reference, and the band there is max(project band, 8 x that gap):
8 = two independent fp32 evaluations (the reference's and the kernel's, each that far from fp64) x 4 for the kernel's other summation
order and its hardware exp2 (whose argument f log2(e) is rounded once more: 0.7 ulp(29) = 7e-7 relative at f = 20, next to the 1e-5
above).  The margin comes from the reference alone, never from the kernel's output.  Measured (fp32 reference vs fp64,
large-rate case, log-rates -12.9 .. 20.0): value gap 4.1e-7 relative, gradient gap 3.7e-6 of the tensor's largest entry; times 8: 3.3e-6 and
2.9e-5, both inside the project's 4e-6 and 1e-4, so the margin does not widen the bands here (the rule stays for a BLAS that sums in
another order).  The log accept ratio of the large-rate transition differences two energies of 1.1e9: the fp32 reference's data
terms, summed in fp64 at the fp64 transition's two ends, give it 1291 off (one ulp of a log-rate near 20 moves a rate of 4.8e8 by 900), outside the
project's 2e-2 + 1e-4 |lar| + 4e-7 |logp| = 457; by the same rule the band there is 8 x 1291.  Normal cases: value gaps to 1.7e-8, gradient gaps to 5.6e-7.  One choice of inputs follows from the same check: the two
30-80-80-10 cases use ELU, because with Relu the fp32 reference itself misses the gradient band there (5.4e-4: see CASES)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import tbnn_oracle as o
from tensor_checks import layers_of, tensor_errs
from test_gpu_freerun import SEED

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FUSED = {"fast3": "", "fast": "fast3", "mid": "fast3,fast,tall,wide", "tall": "fast3,fast,mid,wide", "wide": "fast3,fast,mid,tall"}

CASES = {
    # dims, rows, hidden activation, prior, family, environment, kind
    "fast3": ([5, 50, 50, 50, 1], 3001, o.ACT_RELU, o.PRIOR_CAUCHY, "fast3", {}, "normal"),                  # ragged last tile
    "fast3_two_outputs": ([7, 17, 33, 2], 777, o.ACT_TANH, o.PRIOR_GAUSSIAN, "fast3", {}, "normal"),
    # (a shape of its own: a process that has registered the fast3 table of a shape keeps handing it out)
    "fast": ([4, 30, 30, 1], 2500, o.ACT_TANH, o.PRIOR_GAUSSIAN, "fast", {}, "normal"),                      # TBNN_JIT_SKIP=fast3
    "mid1": ([20, 64, 64, 1], 2000, o.ACT_SIGMOID, o.PRIOR_CAUCHY, "mid", {}, "normal"),                     # VALU last layer
    # (ELU: with Relu at this shape the fp32 REFERENCE misses the gradient band -- a pre-activation that rounds across Relu's kink flips a
    # unit's derivative, and count-sized residuals (|y - exp f| to 400) make one flip 5e-4 of the tensor's largest entry; see the docstring)
    "mid10": ([30, 80, 80, 10], 3001, o.ACT_ELU, o.PRIOR_CAUCHY, "mid", {}, "normal"),                       # MFMA output tile
    "mid10_large_rate": ([30, 80, 80, 10], 2000, o.ACT_ELU, o.PRIOR_CAUCHY, "mid", {}, "large"),
    "tall": ([784, 20, 20, 1], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "tall", {}, "normal"),
    "wide1": ([10, 200, 200, 1], 3001, o.ACT_RELU, o.PRIOR_CAUCHY, "wide", {}, "normal"),
    "wide10": ([10, 200, 200, 10], 1000, o.ACT_ELU, o.PRIOR_GAUSSIAN, "wide", {}, "normal"),
    # the layered family (no run-time instantiation, no tall registry): which likelihood kernel runs follows from lay_plan_shape
    "lay_last": ([784, 100, 100, 10], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "layered", {}, "normal"),                          # k_lay_last
    "lay_separate": ([784, 100, 100, 10], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "layered", {"TBNN_LAY_LAST": "0"}, "normal"),  # k_lay_lik
    "lay_tail": ([784, 20, 20, 10], 1205, o.ACT_TANH, o.PRIOR_GAUSSIAN, "layered", {}, "normal"),                          # k_lay_tail
    "lay_both_off": ([784, 20, 20, 10], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "layered",
                     {"TBNN_LAY_TAIL": "0", "TBNN_LAY_LAST": "0"}, "normal"),                                              # k_lay_lik
    "generic": ([5, 16, 16, 4], 517, o.ACT_TANH, o.PRIOR_CAUCHY, "generic", {}, "normal"),
}
TRAJ = ([1, 10, 10, 1], 500, o.ACT_RELU, o.PRIOR_CAUCHY)          # one workgroup takes all the rows: the trajectory kernel
NET = [1, 16, 16, 1]                                              # the network(...) of the trainChains and end-to-end tests (tanh)


def spec_of(dims, act, prior):
    return o.make_spec(dims, act, prior, o.LIK_POISSON, o.ACT_NONE)


def job(spec, lik=o.LIK_POISSON, skip="", weighted=False):
    j = {"layers": [list(l) for l in layers_of(spec)], "likelihood": lik, "skip": skip, "flags": ""}
    if weighted:
        j["weighted"] = True
    return j


def jit_jobs():
    """the run-time instantiations this module asks for (jit.prebuild's job format): 14 libraries"""
    jobs = []
    for dims, _n, act, prior, fam, _env, _kind in CASES.values():
        if fam in FUSED:
            jobs.append(job(spec_of(dims, act, prior), skip=FUSED[fam]))
    jobs.append(job(spec_of(*TRAJ[:1], *TRAJ[2:])))
    jobs.append(job(spec_of([5, 50, 50, 50, 1], o.ACT_RELU, o.PRIOR_CAUCHY), weighted=True))
    jobs.append(job(spec_of(NET, o.ACT_TANH, o.PRIOR_CAUCHY)))
    jobs.append(job(spec_of(NET, o.ACT_TANH, o.PRIOR_CAUCHY), weighted=True))
    # the predictor's forward chain of the fitted network (a fixed-sd Gaussian handle: forward passes and the ensemble reductions only)
    jobs.append(job(o.make_spec(NET, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_FIXED_GAUSSIAN), lik=o.LIK_FIXED_GAUSSIAN))
    return [j for i, j in enumerate(jobs) if j not in jobs[:i]]


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """compile this module's run-time shapes side by side before any test touches the GPU (cached: a second run compiles nothing)"""
    from tensorbnn_amd import jit
    jobs = jit_jobs()
    assert len(jobs) <= 16
    assert jit.prebuild(jobs) == len(jobs)


def problem_of(dims, n, act, prior, kind="normal"):
    _g, X, Yr, theta, eta = o.synth_problem(dims, n, act, prior, o.LIK_GAUSSIAN)     # X, standardised teacher outputs [n, K], the initial state
    spec = spec_of(dims, act, prior)
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1)
    eta = np.asarray(eta[:spec.n_hypers], dtype=np.float32)          # no likelihood hyper
    # counts drawn from a teacher's rates: its standardised outputs (mean 0, sd 1) stretched to log-rates of mean 1.5, sd 1.5 in [-3, 6]
    ft = np.clip(1.5 + 1.5 * Yr.astype(np.float64), -3.0, 6.0)
    Y = np.random.default_rng(11).poisson(np.exp(ft)).astype(np.float32)
    # the state's own log-rates: the last layer scaled so that they stay within [-5, 5] (normal), or so that the largest is 20 (large rates:
    # a negative scale mirrors the last layer when the extreme of the unscaled state is a negative one)
    f = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    scale = 1.0
    if kind == "large":
        scale = 20.0 / (f.max() if f.max() >= -f.min() else f.min())
    elif np.abs(f).max() > 5.0:
        scale = 5.0 / np.abs(f).max()
    if scale != 1.0:
        ow, _ob = spec.offsets()[-1]
        theta = theta.copy()
        theta[ow:] = (theta[ow:].astype(np.float64) * scale).astype(np.float32)
    f = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    assert (19.0 < f.max() <= 20.01) if kind == "large" else np.abs(f).max() <= 5.01
    return spec, X, Y, theta, eta


def problem(name):
    dims, n, act, prior, _fam, _env, kind = CASES[name]
    return problem_of(dims, n, act, prior, kind)


def data_terms_gap32(spec, theta, X, Y):
    """sum over (row, output) of y f - exp(f) evaluated in fp32 minus the same in fp64, both summed in fp64, at the fp32 state `theta`"""
    out = []
    for dt in (np.float32, np.float64):
        f = o.forward(spec, np.asarray(np.float32(theta), dt), np.asarray(X, dt), dt)
        y = np.asarray(Y, dt).reshape(f.shape[1], -1).T
        out.append(np.sum((y * f - np.exp(f)).astype(np.float64)))
    return out[0] - out[1]


def gaps(spec, lp, g, lp64, g64):
    """(value error / max(|lp64|, 1), per tensor: gradient error / max(|g64|_inf, 1e-3))"""
    return abs(lp - lp64) / max(abs(lp64), 1.0), tensor_errs(spec, g, g64, 1e-3)


def bands(name, spec, theta, eta, X, Y, ref64):
    """(value band, gradient band per tensor): the project's 4e-6 and 1e-4; the large-rate case: max(those, 8 x the gap of the fp32 reference)"""
    nt = 2 * len(spec.layers)
    if CASES.get(name, (0,) * 7)[6] != "large":
        return 4e-6, [1e-4] * nt
    lp32, g32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)
    gv, gg = gaps(spec, lp32, g32, *ref64)
    print(f"[poisson] {name}: fp32 reference vs fp64: value gap {gv:.3e}, gradient gaps max {max(gg):.3e}")
    return max(4e-6, 8 * gv), [max(1e-4, 8 * x) for x in gg]


def check_value_gradient(name, lp, g, spec, theta, eta, X, Y, w=None):
    ref64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64, w=w)
    bv, bg = bands(name, spec, theta, eta, X, Y, ref64)
    ev, eg = gaps(spec, lp, g, *ref64)
    print(f"[poisson] {name}: logp {lp:.9g} (fp64 {ref64[0]:.9g}) err {ev:.3e} of band {bv:.3e}; gradient err/band max {max(e / b for e, b in zip(eg, bg)):.3f}")
    assert np.isfinite(lp) and np.all(np.isfinite(g))
    assert ev <= bv, (name, lp, ref64[0])
    for k, (e, b) in enumerate(zip(eg, bg)):
        assert e <= b, (name, k, e, b)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_in_fp32_stays_inside_the_bands(name):
    """CPU arithmetic only: the reference's own formula evaluated in fp32 against fp64 -- inside the project's bands for every normal
    case (so the bands are a fair demand on an fp32 kernel); the large-rate case reports the gap its margin is derived from"""
    spec, X, Y, theta, eta = problem(name)
    ref64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)
    lp32, g32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)
    gv, gg = gaps(spec, lp32, g32, *ref64)
    f = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    print(f"[poisson] {name}: log-rates [{f.min():.2f}, {f.max():.2f}], counts to {Y.max():.0f}; fp32 reference: value gap {gv:.3e}, gradient gap {max(gg):.3e}")
    if CASES[name][6] == "normal":
        assert -5.01 <= f.min() and f.max() <= 5.01
        assert gv <= 4e-6 and max(gg) <= 1e-4, (gv, gg)
    else:
        assert f.max() > 19.0 and np.isfinite(gv) and np.all(np.isfinite(gg))


def make_chain(native, monkeypatch, name, spec, **kw):
    fam, env = CASES[name][4], CASES[name][5]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if fam in FUSED:
        monkeypatch.setenv("TBNN_JIT_SKIP", FUSED[fam])
        ch = native.Chain(layers_of(spec), likelihood=o.LIK_POISSON, jit=True, **kw)
        assert ch.kernel_name.startswith(f"jit-{fam}<") and ",poisson;" in ch.kernel_name, ch.kernel_name
    elif fam == "layered":
        monkeypatch.setenv("TBNN_TALL", "0")
        monkeypatch.setenv("TBNN_REGISTERED", "0")
        ch = native.Chain(layers_of(spec), likelihood=o.LIK_POISSON, jit=False, **kw)
        assert ch.kernel_name.startswith("layered<"), ch.kernel_name
    else:
        ch = native.Chain(layers_of(spec), likelihood=o.LIK_POISSON, kernel=native.KERNEL_GENERIC, **kw)
        assert ch.kernel_name == "generic", ch.kernel_name
    assert ch.H == 4 * len(spec.layers)
    return ch


@pytest.mark.parametrize("name", list(CASES))
def test_value_gradient_forward(native, monkeypatch, name):
    spec, X, Y, theta, eta = problem(name)
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
    check_value_gradient(name, lp, g, spec, theta, eta, X, Y)
    # stat is the data term of the true log-density (the constant included): logp minus the priors
    parts = o.unflatten(spec, theta.astype(np.float64))
    prior = sum(o.layer_log_prob(l, eta.astype(np.float64)[4 * i:4 * i + 4], W, b, np.float64) for i, (l, (W, b)) in enumerate(zip(spec.layers, parts)))
    assert abs((lp - st) - prior) <= 4e-6 * max(abs(lp), 1.0)        # (the value's own band: the device sums the priors in fp32 terms)
    f64 = o.forward(spec, theta, X[:m], np.float64)
    assert f.shape == f64.shape == (spec.layers[-1].out_dim, m)
    assert np.abs(f - f64).max() <= 1e-4 * max(1.0, np.abs(f64).max())


@pytest.mark.parametrize("name", list(CASES))
def test_transitions(native, monkeypatch, name):
    spec, X, Y, theta, eta = problem(name)
    rng = np.random.default_rng(4)
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    ch = make_chain(native, monkeypatch, name, spec, seed=SEED, chain_id=2)
    ch.set_data(X, Y)
    vg = lambda q: o.target_log_prob_and_grad(spec, q, eta, X, Y, np.float64)
    lp64 = vg(theta)[0]
    # (large rates: the fp64 gradient's largest entry is 2.8e9 there against 4.8e4 in the normal case of the same shape; the step size
    # shrinks by that ratio, 3e-5 x 4.8e4 / 2.8e9, so that one kick eps |g| moves the momentum as far as it does there -- a choice of input
    # from the reference alone; the bands are the same)
    eps = 5e-10 if CASES[name][6] == "large" else 3e-5
    for log_u in (-1e30, 1e30):
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hmc_step(eps, 4, p0=p0, log_u=log_u)
        ref = o.hmc_step(vg, theta, eps, 4, p0, log_u, np.float64)
        print(f"[poisson] {name}: lar {out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g}), logp {lp64:.6g}")
        tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
        if CASES[name][6] == "large":
            # the docstring's rule for large rates: max(project band, 8 x the gap of the fp32 reference) -- here the log accept ratio of the
            # reference's data terms evaluated in fp32 (summed in fp64, as the kernels sum their statistic) at the fp64 transition's two ends
            gap = abs(data_terms_gap32(spec, ref.theta_proposed, X, Y) - data_terms_gap32(spec, theta, X, Y))
            print(f"[poisson] {name}: fp32 reference vs fp64: log accept ratio gap {gap:.1f} (project band {tol:.1f})")
            tol = max(tol, 8 * gap)
        assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= tol
        assert bool(out["accepted"]) == ref.accepted == (log_u < 0)
        assert abs(out["logp_old"] - lp64) <= 4e-6 * max(abs(lp64), 1.0)              # the record carries the true log-density
        assert np.abs(ch.get_state() - ref.theta).max() <= 1e-5 * max(1.0, np.abs(ref.theta).max())
        again = ch.set_state(theta) or ch.hmc_step(eps, 4, p0=p0, log_u=log_u)
        assert again["log_accept_ratio"] == out["log_accept_ratio"] and again["logp_new"] == out["logp_new"]
    # the hyper transition: the layer priors only (no likelihood hyper; the oracle adds a data term for the Gaussian likelihood alone)
    ph = rng.standard_normal(spec.n_hypers).astype(np.float32)
    ch.set_state(theta); ch.set_hypers(eta)
    ch.logp_grad(theta, eta)
    out = ch.hyper_step(1e-4, 9, p0=ph, log_u=-1e30)
    ref = o.hyper_step(spec, eta, theta, X, Y, 1e-4, 9, ph, -1e30, np.float64)
    assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= 2e-2 + 1e-3 * abs(ref.log_accept_ratio)
    assert np.allclose(ch.get_hypers(), ref.theta, rtol=1e-4, atol=1e-5)
    # after the accepted hyper transition the cached gradient is refreshed for the new priors: the next weight step starts from it
    lp_new, g_new, _ = ch.logp_grad(theta, ch.get_hypers())
    check_value_gradient(name, lp_new, g_new, spec, theta, ch.get_hypers(), X, Y)
    ch.close()


def test_trajectory_kernel(native, monkeypatch):
    """a small narrow problem takes the one-launch trajectory kernel; the traced run of the same transition (per-step kernels) agrees with
    fp64 step by step"""
    dims, n, act, prior = TRAJ
    spec, X, Y, theta, eta = problem_of(dims, n, act, prior)
    monkeypatch.setenv("TBNN_TRAJ", "1")
    monkeypatch.setenv("TBNN_JIT_SKIP", "")
    ch = native.Chain(layers_of(spec), likelihood=o.LIK_POISSON, jit=True, seed=SEED)
    assert ch.kernel_name.startswith("jit-fast3<") and ",poisson;" in ch.kernel_name, ch.kernel_name
    ch.set_data(X, Y)
    p0 = np.random.default_rng(5).standard_normal(spec.n_params).astype(np.float32)
    vg = lambda q: o.target_log_prob_and_grad(spec, q, eta, X, Y, np.float64)
    lp64 = vg(theta)[0]
    for L in (1, 9):
        ref = o.hmc_step(vg, theta, 2e-4, L, p0, -1e30, np.float64)
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hmc_step(2e-4, L, p0=p0, log_u=-1e30)
        assert ch.last_transition_path == "trajectory"
        tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
        print(f"[poisson] trajectory L={L}: lar {out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g})")
        assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= tol
        assert bool(out["accepted"]) == ref.accepted
        assert abs(out["logp_new"] - ref.logp_new) <= 4e-6 * max(abs(ref.logp_new), 1.0)
        np.testing.assert_allclose(ch.get_state(), ref.theta, rtol=2e-5, atol=2e-6)
        ch.set_state(theta); ch.set_hypers(eta)
        again = ch.hmc_step(2e-4, L, p0=p0, log_u=-1e30)
        assert again["log_accept_ratio"] == out["log_accept_ratio"] and ch.last_transition_path == "trajectory"
        ch.set_state(theta); ch.set_hypers(eta)
        traced = ch.hmc_step(2e-4, L, p0=p0, log_u=-1e30, trace=True)
        assert ch.last_transition_path == "per-step"
        tr, tr64 = np.asarray(traced["trace_logp"]), np.asarray(ref.trace_logp)
        assert tr.shape == tr64.shape and np.max(np.abs(tr - tr64) / np.maximum(np.abs(tr64), 1.0)) <= 4e-6
        assert abs(traced["log_accept_ratio"] - ref.log_accept_ratio) <= tol
    ch.close()


@pytest.mark.parametrize("name", ["fast3", "mid10", "lay_last", "generic"])
def test_overflowing_proposal_is_rejected(native, monkeypatch, name):
    """a momentum that carries the proposal's log-rates past the fp32 range of exp: the statistic is -inf or NaN, the transition is
    rejected whatever log u, and the chain keeps its state bit for bit"""
    spec, X, Y, theta, eta = problem(name)
    ch = make_chain(native, monkeypatch, name, spec, seed=SEED)
    ch.set_data(X, Y); ch.set_state(theta); ch.set_hypers(eta)
    before = ch.logp_grad()
    p0 = (3e4 * np.random.default_rng(8).standard_normal(spec.n_params)).astype(np.float32)
    f_prop = o.forward(spec, theta.astype(np.float64) + 1e-2 * p0.astype(np.float64), X.astype(np.float64), np.float64)
    assert f_prop.max() > 1000.0                                    # far beyond log(FLT_MAX) = 88.7
    out = ch.hmc_step(1e-2, 2, p0=p0, log_u=-1e30)
    assert out["accepted"] == 0 and out["log_accept_ratio"] == -np.inf
    assert np.array_equal(ch.get_state(), theta) and np.array_equal(ch.get_hypers(), eta)
    after = ch.logp_grad()
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.all(np.isfinite(after[1]))
    ok = ch.hmc_step(3e-5, 3, p0=(p0 / 3e4).astype(np.float32), log_u=-1e30)          # and it goes on from there
    assert ok["accepted"] == 1 and np.isfinite(ok["log_accept_ratio"]) and np.all(np.isfinite(ch.get_state()))
    ch.close()


@pytest.mark.parametrize("name", ["fast3", "lay_last", "generic"])
def test_row_weights(native, monkeypatch, name):
    spec, X, Y, theta, eta = problem(name)
    n = min(600, X.shape[0])
    X, Y = X[:n], Y[:n]
    rng = np.random.default_rng(21)
    w = rng.integers(0, 4, n).astype(np.float32)
    ch = make_chain(native, monkeypatch, name, spec)
    ch.set_data(X, Y)
    plain = ch.logp_grad(theta, eta)
    # a weight of 1 everywhere: the unweighted bits
    ch.set_row_weights(np.ones(n, np.float32))
    if CASES[name][4] in FUSED:
        assert ",poisson,weighted;" in ch.kernel_name, ch.kernel_name
    ones = ch.logp_grad(theta, eta)
    if CASES[name][4] in FUSED:                  # (a weighted handle without a weighted table runs another family: the same values, not bits)
        assert ones[0] == plain[0] and ones[2] == plain[2] and np.array_equal(ones[1], plain[1])
    check_value_gradient(name, ones[0], ones[1], spec, theta, eta, X, Y)
    # integer weights: the rows duplicated
    ch.set_row_weights(w)
    lp, g, st = ch.logp_grad(theta, eta)
    check_value_gradient(name, lp, g, spec, theta, eta, X, Y, w)
    idx = np.repeat(np.arange(n), w.astype(int))
    ch.set_row_weights(None)
    ch.set_data(X[idx], Y[idx])
    dup = ch.logp_grad(theta, eta)
    check_value_gradient(name, dup[0], dup[1], spec, theta, eta, X[idx], Y[idx])      # the duplicated run against its own fp64 reference
    ev, eg = gaps(spec, lp, g, dup[0], dup[1])                                        # ... and the weighted run against it, at the bands
    print(f"[poisson] {name}: weights vs duplicated rows: value {ev:.3e}, gradient {max(eg):.3e}")
    assert ev <= 4e-6 and max(eg) <= 1e-4, (ev, eg)
    # rows of weight zero: whatever finite, >= 0 targets they carry, nothing changes -- bit for bit
    Y2 = Y.copy()
    Y2[w == 0] = rng.integers(0, 100000, Y2[w == 0].shape).astype(np.float32) + 0.5
    ch.set_data(X, Y2); ch.set_row_weights(w)
    z = ch.logp_grad(theta, eta)
    assert z[0] == lp and z[2] == st and np.array_equal(z[1], g)
    # clearing the weights brings the unweighted constant back
    ch.set_data(X, Y); ch.set_row_weights(w); ch.set_row_weights(None)
    back = ch.logp_grad(theta, eta)
    assert back[0] == plain[0] and np.array_equal(back[1], plain[1])
    ch.close()


def test_refusals(native, monkeypatch):
    spec, X, Y, theta, eta = problem("fast3")
    ch = make_chain(native, monkeypatch, "fast3", spec)
    ch.set_data(X, Y)
    good = ch.logp_grad(theta, eta)
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        Yb = Y.copy()
        Yb[17, 0] = bad
        with pytest.raises(native.TbnnError, match="counts"):
            ch.set_data(X[:100], Yb[:100])
        again = ch.logp_grad(theta, eta)                             # the handle keeps the rows it had
        assert again[0] == good[0] and np.array_equal(again[1], good[1])
    ch.set_data(X[:100], Y[:100])                                    # ... and takes good rows afterwards
    lp, g, _ = ch.logp_grad(theta, eta)
    check_value_gradient("refusals", lp, g, spec, theta, eta, X[:100], Y[:100])
    ch.close()
    for act in (o.ACT_EXP, o.ACT_SIGMOID):
        layers = layers_of(o.make_spec([5, 8, 1], o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_POISSON, act))
        with pytest.raises(native.TbnnError, match="log-rate"):
            native.Chain(layers, likelihood=o.LIK_POISSON, jit=False)


def test_gaussian_and_poisson_chain_of_one_shape(native, monkeypatch):
    """a Gaussian chain on its ahead-of-time fast3 table and the Poisson chain of the same layers on its own run-time table, side by side"""
    spec, X, Y, theta, eta = problem("fast3")
    gspec = o.make_spec([5, 50, 50, 50, 1], o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN)
    gch = native.Chain(layers_of(gspec), likelihood=o.LIK_GAUSSIAN, jit=True)
    assert gch.kernel_name.startswith("fast3<") and "poisson" not in gch.kernel_name, gch.kernel_name
    geta = np.concatenate([eta, [np.sqrt(0.1)]]).astype(np.float32)
    gch.set_data(X, Y)
    glp, gg, _ = gch.logp_grad(theta, geta)
    ch = make_chain(native, monkeypatch, "fast3", spec)
    ch.set_data(X, Y)
    lp, g, _ = ch.logp_grad(theta, eta)
    g2 = gch.logp_grad(theta, geta)
    assert g2[0] == glp and np.array_equal(g2[1], gg)                    # the Gaussian chain unchanged beside it
    p2 = ch.logp_grad(theta, eta)
    assert p2[0] == lp and np.array_equal(p2[1], g)
    gch.close(); ch.close()
    check_value_gradient("mixed", lp, g, spec, theta, eta, X, Y)
    glp64 = o.target_log_prob_and_grad(gspec, theta, geta, X, Y, np.float64)[0]
    assert abs(glp - glp64) <= 4e-6 * abs(glp64)


# ---------------------------------------------------------------------------------------------------------------------- ensemble reductions
def test_ensemble_loglik(native, monkeypatch):
    """tbnn_ensemble_loglik under TBNN_LIK_POISSON on a Poisson handle and on a Gaussian handle, against the terms in fp64 from the device's
    fp32 predictions, to the bands of tests/test_gpu_ensemble.py (its fp64 term model: 8 ulp of every magnitude that enters a term, the sum
    over n d_out terms, the mixture's m + 8 ulp)"""
    from test_gpu_ensemble import U, logsumexp_rows
    spec, X, Y, theta, eta = problem("fast3")
    X, Y = X[:700], Y[:700]
    m, n, d_out = 6, 700, 1
    rng = np.random.default_rng(31)
    thetas = (theta[None] + 0.02 * rng.standard_normal((m, spec.n_params))).astype(np.float32)
    gspec = o.make_spec([5, 50, 50, 50, 1], o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN)
    handles = {"poisson": make_chain(native, monkeypatch, "fast3", spec),
               "gaussian": native.Chain(layers_of(gspec), likelihood=o.LIK_GAUSSIAN, jit=True)}
    for tag, ch in handles.items():
        f = ch.forward_many(thetas, X=X).astype(np.float64)                          # [m, d_out, n]
        y = Y.reshape(n, d_out).T.astype(np.float64)[None]
        t1, t2, t3 = y * f, np.exp(f), o.lgamma(y + 1.0) + 0 * f
        l = (t1 - t2 - t3).sum(axis=1)                                               # [m, n]
        err = (8 * U * (np.abs(t1) + t2 + np.abs(t3))).sum(axis=1)
        mag = np.abs(t1 - t2 - t3).sum(axis=(1, 2))
        for wts in (None, np.array([1, 0, 2.5, 1, 0.25, 3], dtype=np.float32)):
            per_net, rows = ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=o.LIK_POISSON, weights=wts)
            again = ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=o.LIK_POISSON, weights=wts)
            assert np.array_equal(per_net, again[0]) and np.array_equal(rows, again[1])
            want = l.sum(axis=1)
            tol = err.sum(axis=1) + n * d_out * U * mag + np.spacing(np.abs(want))
            e = np.abs(per_net - want)
            print(f"[poisson] ensemble on a {tag} handle: per_net worst err/tol {np.max(e / tol):.3f}")
            assert np.all(np.isfinite(per_net)) and np.all(e <= tol)
            ww = np.ones(m) if wts is None else wts.astype(np.float64)
            want = logsumexp_rows(l, ww) - math.log(ww.sum())
            tol = err[ww > 0].max(axis=0) + (m + 8) * U + 4 * U * np.abs(want)
            e = np.abs(rows - want)
            print(f"[poisson] ensemble on a {tag} handle: lppd worst err/tol {np.max(e / tol):.3f}")
            assert np.all(np.isfinite(rows)) and np.all(e <= tol)
        ch.close()


# ---------------------------------------------------------------------------------------------------------------------- row-sharded chain
def test_row_shard_two_ranks(tmp_path, native, monkeypatch):
    """world 2 on the stub collective library (tests/stubccl/worker_poisson.py: two fresh child processes, each under its own time limit):
    the sharded chain takes the unsharded chain's decisions and reaches its state, within the sharding band of tests/test_gpu_multirank.py"""
    from conftest import wait_gpu_quiet
    from test_gpu_multirank import build_stub
    sys.path.insert(0, os.path.join(HERE, "stubccl"))
    import worker_poisson as wp
    wait_gpu_quiet()
    env = dict(os.environ, TBNN_RCCL_LIB=build_stub(), TBNN_JIT="0", TBNN_PREBUILD_JIT="0")
    idfile = str(tmp_path / "shard.id")
    procs = []
    for r in range(2):
        out = str(tmp_path / f"shard_{r}.npz")
        procs.append((out, subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "stubccl", "worker_poisson.py"), str(r), "2", idfile, out],
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
    for name in wp.SHAPES:
        spec, X, Y, theta, eta = wp.problem(name)
        ref = wp.chain_of(name, spec)
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
        check_value_gradient("shard " + name, float(ranks[0][name + "_lp"]), ranks[0][name + "_g"], spec, theta, eta, X, Y)
        ref.close()


# ---------------------------------------------------------------------------------------------------------------------- network / train
def rate_of(x):
    return np.exp(1.0 + 1.3 * np.sin(2.0 * x))                       # 0.74 .. 10: clearly not constant


def counts(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, 1)).astype(np.float32)
    return X, rng.poisson(rate_of(X.astype(np.float64))).astype(np.float32)


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
    from tensorbnn_amd.likelihood import PoissonLikelihood
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, Y = counts(600, 1)
    Xv, Yv = counts(200, 2)
    C, EPOCHS = 2, 16
    grp_net = make_net(X, Y, Xv, Yv)
    rec = grp_net.trainChains(C, EPOCHS, 4, PoissonLikelihood(), adjustHypers=True, folderName="multi", networksPerFile=2)
    assert len(rec) == EPOCHS and all(len(r["main"]) == C for r in rec)
    for c in range(C):
        net = make_net(X, Y, Xv, Yv, chain_id=c)
        solo = net.train(EPOCHS, 4, PoissonLikelihood(), adjustHypers=True, folderName="solo%d" % c, networksPerFile=2, verbose=False)
        assert net._chain.kernel_name.startswith("jit-fast3<") and "poisson" in net._chain.kernel_name, net._chain.kernel_name
        for rg, rs in zip(rec, solo):
            assert rg["eps"][c] == rs["eps"] and rg["L"][c] == rs["L"]
            for k in ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new", "sjd"):
                assert rg["main"][c][k] == rs["main"][k], (c, rg["iter"], k)
            assert rg["hyper"][c]["log_accept_ratio"] == rs["hyper"]["log_accept_ratio"]
            assert rg["hyper_step_size"][c] == rs["hyper_step_size"]


def test_train_beats_the_constant_rate_model(tmp_path, monkeypatch, native):
    """network(...).train on counts from rate(x) = exp(1 + 1.3 sin 2x), with trainWeights= of one everywhere; the saved ensemble's held-out
    mean log predictive density (predictor.logPredictiveDensity, on the device) must beat the constant-rate model rate = mean(y_train)"""
    from tensorbnn_amd.likelihood import PoissonLikelihood
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, Y = counts(600, 1)
    Xv, Yv = counts(300, 2)
    yv = Yv.astype(np.float64)
    logpmf = lambda rate: yv * np.log(rate) - rate - o.lgamma(yv + 1.0)
    base = float(np.mean(logpmf(np.full_like(yv, Y.astype(np.float64).mean()))))
    truth = float(np.mean(logpmf(rate_of(Xv.astype(np.float64)))))
    assert truth > base + 0.5, (truth, base)                         # the generating function itself wins by a wide margin: no luck needed
    net = make_net(X, Y, Xv, Yv, trainWeights=np.ones(600, np.float32))
    net.train(120, 5, PoissonLikelihood(), folderName="counts", networksPerFile=1, verbose=False)
    assert ",poisson,weighted;" in net._chain.kernel_name, net._chain.kernel_name
    p = predictor(str(tmp_path / "counts") + "/", likelihood=PoissonLikelihood())
    per_net, per_row = p.logPredictiveDensity(Xv, Yv)
    lpd = float(np.mean(per_row))
    print(f"[poisson] held-out mean log predictive density: ensemble {lpd:.4f}, constant rate {base:.4f}, generating function {truth:.4f} "
          f"({p.numNetworks} saved networks)")
    assert per_net.shape == (p.numNetworks,) and per_row.shape == (300,) and np.all(np.isfinite(per_row))
    assert lpd > base
    mean, var = p.predictMoments(Xv)                                 # rate: exp by default under the Poisson likelihood
    mean2, tot = p.predictMoments(Xv, countVariance=True)
    assert np.array_equal(mean, mean2) and np.array_equal(tot, mean + var) and np.all(mean > 0) and np.all(var >= 0)
