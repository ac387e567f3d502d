"""WeibullLikelihood (TBNN_LIK_WEIBULL, right-censored targets) without a GPU: the fp64 arm of tests/weibull_ref.py against
torch.autograd (value and gradient, five cases: weighted and unweighted, all-event, all-censored, d_out = 3) and against SciPy's Weibull
log density and log survival function, the Python class and its `encode`, the predictor's plumbing, refusals and `survival` on a stub
chain, the kernels' likelihood code and the run-time kernel plumbing, the C ABI's admission rules (tbnn_fused_kernel_available runs the
descriptor checks of tbnn_create on the host), and `test_reference_in_fp32_stays_inside_the_bands`: the kernel's own formula in fp32
against the fp64 definition at every case of tests/test_gpu_weibull.py, inside the project's bands -- value 4e-6 relative, gradient 1e-4
of each tensor's largest entry (floor 1e-3), log accept ratio 2e-2 + 1e-4 |lar| + 4e-7 |logp|.  The figures are printed on every run.

Which of these fail without the feature: everything from "the Python class" down (28 tests: the class, the predictor, the codes, the
admission rules, the header, the cross-compiled libraries).  The 23 tests of the first section pin tests/weibull_ref.py itself -- against
SciPy, torch.autograd and its own fp32 arm -- and touch nothing of the package: they pass on any tree that holds this module and the
reference, as reference-pinning tests must."""
import ctypes as C
import math

import numpy as np
import pytest

import weibull_ref as wr
import tbnn_oracle as o
from tensor_checks import tensor_errs
from test_predictive_host import HYPERS, StubChain, X as SX, Y as SY, stub_predictor

DIMS_GRID = [c[0] for c in wr.CASES.values()] + [[2, 12, 1], [1, 100, 1], [5, 20, 20, 3], [20, 100, 100, 2], [8, 90, 130, 70, 3], [8, 300, 300, 1]]


def layers_for(dims, hidden_act, last_act=0):
    return [(dims[i], dims[i + 1], hidden_act if i < len(dims) - 2 else last_act, 0) for i in range(len(dims) - 1)]


# ---------------------------------------------------------------------------------------------------------------------- the reference
def test_reference_formula():
    from scipy.stats import weibull_min
    rng = np.random.default_rng(1)
    f = 0.5 + 0.8 * rng.standard_normal((3, 50))
    for k in (0.5, 1.0, 1.5, 3.0, 8.0):
        t = np.exp(f) * rng.weibull(k, f.shape)                           # [d_out, rows]
        d = rng.random(f.shape) < 0.6
        y = np.where(d, t, -t).T                                          # [rows, d_out], signed
        got = wr.terms(f, y, k)
        assert got.shape == (3, 50) and got.dtype == np.float64 and np.all(np.isfinite(got))
        dist = weibull_min(k, scale=np.exp(f))
        want = np.where(d, dist.logpdf(t), dist.logsf(t))
        u = (t * np.exp(-f)) ** k
        mag = abs(math.log(k)) + np.abs((k - 1.0) * np.log(t)) + np.abs(k * f) + u
        err = np.abs(got - want)
        print(f"[weibull] k {k:g}: fp64 arm against scipy.stats.weibull_min, worst gap {np.max(err / mag):.3e} of the terms' magnitudes")
        assert np.all(err <= 1e-13 * mag)
    # k = 1 with every row an event is the exponential distribution of mean lambda
    y = rng.exponential(np.exp(f)).T
    assert np.allclose(wr.terms(f, y, 1.0), -f - y.T * np.exp(-f), rtol=1e-13, atol=1e-13)
    # a censored row and an event row at the same time differ by log k + (k - 1) log t - k f, and their deltas by k
    te, de = wr.elementwise(f, t.T, 1.5, np.float64)
    tc, dc = wr.elementwise(f, -t.T, 1.5, np.float64)
    assert np.allclose(te - tc, 1.5 * f, rtol=1e-14, atol=1e-14) and np.allclose(dc - de, 1.5, rtol=1e-13)
    assert np.allclose(wr.terms(f, t.T, 1.5) - wr.terms(f, -t.T, 1.5), math.log(1.5) + 0.5 * np.log(t) - 1.5 * f, rtol=1e-12, atol=1e-12)
    # the delta is k (u - d): -k d at t -> 0, 0 on an event at t = lambda (u = 1)
    _t, dl = wr.elementwise(f, np.exp(f).T, 2.5, np.float64)
    assert np.all(np.abs(dl) <= 1e-13)


def _torch_value_and_grad(spec, k, theta, eta, X, Y, w=None):
    """the log posterior and its gradient by torch.autograd in float64: the data term written out from the definition with torch
    operations over the oracle's layers (dense W a + b, the activation), the priors' part taken from the oracle (it does not depend on the
    likelihood)"""
    import torch
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    a = torch.tensor(np.asarray(X, dtype=np.float64).T)
    off = 0
    for l in spec.layers:
        W = th[off:off + l.in_dim * l.out_dim].reshape(l.out_dim, l.in_dim)
        off += l.in_dim * l.out_dim
        b = th[off:off + l.out_dim].reshape(l.out_dim, 1)
        off += l.out_dim
        z = W @ a + b
        a = {o.ACT_NONE: lambda v: v, o.ACT_TANH: torch.tanh, o.ACT_RELU: torch.relu, o.ACT_SIGMOID: torch.sigmoid}[l.act](z)
    f = a                                                                                  # [d_out, n]
    y = torch.tensor(np.asarray(Y, dtype=np.float64).reshape(f.shape[1], -1).T)
    t = y.abs()
    u = torch.exp(k * (torch.log(t) - f))
    ll = torch.where(y > 0, math.log(k) + (k - 1.0) * torch.log(t) - k * f - u, -u)
    if w is not None:
        ll = ll * torch.tensor(np.asarray(w, dtype=np.float64))
    data = ll.sum()
    data.backward()
    return float(data.detach()), th.grad.numpy()


AUTOGRAD_CASES = {
    "unweighted": ([3, 6, 5, 2], "mixed", False, 1.5),
    "weighted": ([3, 6, 5, 2], "mixed", True, 0.5),
    "all_events": ([3, 6, 5, 1], "events", False, 3.0),
    "all_censored": ([3, 6, 5, 1], "censored", True, 1.0),
    "three_outputs": ([4, 7, 3], "mixed", False, 1.5),
}


@pytest.mark.parametrize("case", list(AUTOGRAD_CASES))
def test_reference_value_and_gradient_against_autograd(case):
    dims, kind, weighted, k = AUTOGRAD_CASES[case]
    n = 40
    spec, X, Y, theta, eta = wr.problem_of(dims, n, o.ACT_TANH, o.PRIOR_CAUCHY, k, kind)
    if kind == "mixed":
        assert (Y > 0).any() and (Y < 0).any()
    w = np.random.default_rng(2).integers(0, 3, n).astype(np.float64) if weighted else None
    th = theta.astype(np.float64)
    lp, g = wr.target_log_prob_and_grad(spec, k, th, eta, X, Y, np.float64, w)
    data, gdata = _torch_value_and_grad(spec, k, th, eta, X, Y, w)
    # the priors' part: the same call with every weight 0 (no data term)
    lp0, g0 = wr.target_log_prob_and_grad(spec, k, th, eta, X, Y, np.float64, np.zeros(n))
    assert math.isclose(lp - lp0, data, rel_tol=1e-12, abs_tol=1e-10), (lp - lp0, data)
    assert np.allclose(g - g0, gdata, rtol=1e-10, atol=1e-10)
    f = o.forward(spec, th, X.astype(np.float64), np.float64)
    tt = wr.terms(f, Y, k)
    assert math.isclose(data, float(np.sum(tt if w is None else w * tt)), rel_tol=1e-12)
    if weighted:
        # integer weights are duplicated rows, the constant included
        idx = np.repeat(np.arange(n), w.astype(int))
        b_ = wr.target_log_prob_and_grad(spec, k, th, eta, X[idx], Y[idx], np.float64)
        assert math.isclose(lp, b_[0], rel_tol=1e-12) and np.allclose(g, b_[1], rtol=1e-10, atol=1e-12)


def test_fp32_arm_non_finite_rules():
    """u past the fp32 range gives a non-finite term (the proposal is rejected); a NaN stays a NaN, through f and through the target"""
    f = np.array([[-1e4, -60.0, -20.0, 0.0, 20.0, 1e4]], dtype=np.float32)
    for sign in (1.0, -1.0):
        y = np.full((f.shape[1], 1), sign * 7.0, dtype=np.float32)
        t, d = wr.elementwise(f, y, 2.0, np.float32)
        assert not np.isfinite(t[0, :2]).any() and np.all(np.isfinite(t[0, 2:])) and np.all(np.isfinite(d[0, 2:]))
        assert d[0, 5] == (-2.0 if sign > 0 else 0.0)
    t, d = wr.elementwise(np.array([[np.nan]], dtype=np.float32), y[:1], 2.0, np.float32)
    assert np.isnan(t).all() and np.isnan(d).all()
    t, d = wr.elementwise(np.array([[0.5]], dtype=np.float32), np.array([[np.nan]], dtype=np.float32), 2.0, np.float32)
    assert np.isnan(t).all() and np.isnan(d).all()


@pytest.mark.parametrize("name", list(wr.CASES))
def test_reference_in_fp32_stays_inside_the_bands(name):
    """CPU arithmetic only: the kernel's formula in fp32 against the fp64 definition -- value, gradient per tensor, and the log accept ratio
    of the GPU module's injected transition"""
    spec, X, Y, theta, eta, k = wr.problem(name)
    lp64, g64 = wr.ref64(name)
    lp32, g32 = wr.target_log_prob_and_grad(spec, k, theta, eta, X, Y, np.float32)
    gv, gg = abs(lp32 - lp64) / max(abs(lp64), 1.0), tensor_errs(spec, g32, g64, 1e-3)
    f = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    ev = float(np.mean(Y > 0))
    print(f"[weibull] {name}: k {k:g}, {100 * ev:.0f} % events, |y| {np.abs(Y).min():.3g} .. {np.abs(Y).max():.3g}, f in [{f.min():.2f}, {f.max():.2f}]; "
          f"fp32 arm: value gap {gv:.3e}, gradient gap {max(gg):.3e}")
    assert np.all(np.isfinite(Y)) and np.abs(Y).min() >= 2.0 ** -100 and np.abs(Y).max() <= 2.0 ** 100
    kind = wr.CASES[name][7]
    assert (ev == 1.0) if kind == "events" else (ev == 0.0) if kind == "censored" else (0.3 < ev < 0.9)
    assert np.isfinite(lp64) and gv <= 4e-6 and max(gg) <= 1e-4, (gv, gg)
    p0 = np.random.default_rng(4).standard_normal(spec.n_params).astype(np.float32)
    r64 = wr.weight_step(spec, k, theta, eta, X, Y, wr.step_size(name), 4, p0, -1e30, np.float64)
    r32 = wr.weight_step(spec, k, theta, eta, X, Y, wr.step_size(name), 4, p0, -1e30, np.float32)
    tol = 2e-2 + 1e-4 * abs(r64.log_accept_ratio) + 4e-7 * abs(lp64)
    move = float(np.abs(r64.theta_proposed - theta).max())
    gap = float(np.abs(r32.theta_proposed.astype(np.float64) - r64.theta_proposed).max())
    print(f"[weibull] {name}: lar fp32 {r32.log_accept_ratio:.6g} fp64 {r64.log_accept_ratio:.6g} (band {tol:.3g}); the proposal moves theta by "
          f"{move:.3g}, the fp32 arm's proposal is within {gap:.3g} of it")
    assert abs(r32.log_accept_ratio - r64.log_accept_ratio) <= tol
    # the transition is no no-op and the data is well conditioned: the state moves by far more than the state checks' tolerance, the
    # log-posterior is a sum of terms of order 1, the fp32 arm follows the trajectory
    assert np.isfinite(r64.log_accept_ratio) and abs(r64.log_accept_ratio) < 50.0
    assert move >= wr.MIN_MOVE and gap <= 1e-5 * max(1.0, np.abs(theta).max())
    assert abs(lp64) <= 40.0 * Y.size + 1e3
    assert abs(r32.logp_new - r64.logp_new) <= 4e-6 * max(abs(r64.logp_new), 1.0)


def test_cases_are_the_student_cases_with_spread_shapes():
    import student_ref as sr
    assert list(wr.CASES)[:len(sr.CASES)] == list(sr.CASES)
    for name in sr.CASES:
        assert wr.CASES[name][:6] == sr.CASES[name][:6] and wr.CASES[name][7] == "mixed"
    assert {c[6] for c in wr.CASES.values()} == {0.5, 1.0, 1.5, 3.0}
    assert wr.CASES["all_events"][7] == "events" and wr.CASES["all_censored"][7] == "censored"


# ---------------------------------------------------------------------------------------------------------------------- the Python class
def test_python_class_encode_and_terms():
    import tensorbnn_amd
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import WeibullLikelihood
    assert tensorbnn_amd.WeibullLikelihood is WeibullLikelihood
    lik = WeibullLikelihood(shape=1.5)
    assert nat.LIK_WEIBULL == 16 and lik.kind == nat.LIK_WEIBULL and lik.shape == 1.5
    assert lik.hypers == [] and lik.mainProbsInHypers is False
    assert lik.calcultateLogProb(hypers=[1, 2, 3]) == [0, 0, 0]
    rng = np.random.default_rng(3)
    f = (1.0 + rng.standard_normal((2, 31))).astype(np.float32)            # [d_out, rows], as network.predict returns
    t = (np.exp(f.T) * rng.weibull(1.5, (31, 2))).astype(np.float32)       # [rows, d_out]
    seen = rng.random((31, 2)) < 0.6
    y = WeibullLikelihood.encode(t, seen)
    assert y.dtype == np.float32 and y.shape == t.shape and np.array_equal(np.abs(y), t) and np.array_equal(y > 0, seen)
    assert np.array_equal(WeibullLikelihood.encode([1.0, 2.0, 3.0], [1, 0, 1]), np.array([1.0, -2.0, 3.0], dtype=np.float32))
    assert np.array_equal(WeibullLikelihood.encode([1.0, 2.0], True), np.array([1.0, 2.0], dtype=np.float32))
    for bad in ([1.0, 0.0], [1.0, -2.0], [float("nan"), 1.0], [float("inf"), 1.0]):
        with pytest.raises(ValueError, match="finite and > 0"):
            WeibullLikelihood.encode(bad, [True, True])
    out = lik.makeResponseLikelihood(None, predict=lambda train, _x: f, realVals=y)
    assert out.shape == (2, 31) and out.dtype == np.float64 and np.all(np.isfinite(out))
    np.testing.assert_allclose(out, wr.terms(f.astype(np.float64), y.astype(np.float64), 1.5), rtol=1e-12)
    np.testing.assert_allclose(lik.logDensity(f, y.T), out, rtol=0, atol=0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            WeibullLikelihood(shape=bad)
    with pytest.raises(KeyError):
        WeibullLikelihood()


class WeibullStubChain(StubChain):
    """tests/test_predictive_host.py's stub with the calls the Weibull likelihood adds: the shape set on the forward chain, the moments of
    the scale, and a CDF that depends on the target so that `survival` can be followed"""

    def __init__(self, d_out=2):
        super().__init__(d_out)
        self.df = []

    def set_lik_df(self, df):
        self.df.append(float(df))

    def ensemble_moments(self, thetas, **kw):
        self.calls.append((np.asarray(thetas), None, None, kw))
        rows = np.asarray(kw["X"]).shape[0]
        return np.full((self.d_out, rows), 6.0), np.full((self.d_out, rows), 2.0)

    def ensemble_predictive(self, thetas, probs=None, Y=None, **kw):
        q, F, Fb = super().ensemble_predictive(thetas, probs=probs, Y=Y, **kw)
        if Y is not None:
            F = -np.expm1(-np.abs(np.asarray(Y, dtype=np.float64)).T)         # [d_out, rows]: the unit exponential's CDF at |y|
        return q, F, Fb

    def ensemble_crps(self, *a, **kw):
        raise AssertionError("the CRPS must be refused on the host")

    def ensemble_uncertainty(self, *a, **kw):
        raise AssertionError("the entropy split must be refused on the host")


def test_predictor_host_paths():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import GammaLikelihood, WeibullLikelihood
    from tensorbnn_amd.predictor import predictor
    rng = np.random.default_rng(5)
    X = rng.standard_normal((20, 2)).astype(np.float32)
    preds = [(1.0 + rng.standard_normal((2, 20))).astype(np.float32) for _ in range(2)]
    Y = WeibullLikelihood.encode(np.exp(preds[0].T) * rng.weibull(3.0, (20, 2)), rng.random((20, 2)) < 0.6)
    p = predictor.__new__(predictor)                     # no saved networks, no device: only the host-side steps
    p.predict = lambda x, n=1: preds
    p.hypers = []
    lik = WeibullLikelihood(shape=3.0)
    got = p._data_logprob(lik, X, Y, 1)
    for g, f in zip(got, preds):
        assert np.isclose(g, wr.terms(f.astype(np.float64), Y.astype(np.float64), 3.0).sum(), rtol=1e-6)
    assert got[0] > got[1]
    # the stub chain: the likelihood code, no sd, the shape set on the forward chain before the call, F alone (a continuous CDF)
    p = stub_predictor(lik, HYPERS)
    p._chain = WeibullStubChain()
    assert p._transform(None) == "exp"
    q = p.predictiveQuantiles(SX, [0.25, 0.75], n=2)
    th, probs, y, kw = p._chain.calls[-1]
    assert q.shape == (2, 2, 3) and y is None and np.array_equal(th[:, 0], [0, 2, 4])
    assert kw["likelihood"] == nat.LIK_WEIBULL == 16 and kw["sd"] is None and p._chain.df == [3.0]
    lo, med, hi = p.predictiveInterval(SX)
    assert p._chain.calls[-1][1].tolist() == [0.05, 0.5, 0.95] and np.all(hi == 2.0)
    F = p.predictiveCDF(SX, SY + 1.0)
    assert isinstance(F, np.ndarray) and F.shape == (2, 3) and p._chain.calls[-1][3]["likelihood"] == 16
    assert p.logPredictiveDensity(SX, SY) == ("per_net", "rows")
    assert p._chain.calls[-1][3]["likelihood"] == 16 and p._chain.calls[-1][3]["sd"] is None and p._chain.df[-1] == 3.0
    n_calls = len(p._chain.calls)
    for kw in ({"sd": 2.0}, {"mean": 1.0}):
        with pytest.raises(ValueError, match="WeibullLikelihood"):
            p.predictiveQuantiles(SX, [0.5], **kw)
    with pytest.raises(ValueError, match="not built for a WeibullLikelihood"):
        p.crps(SX, SY)
    with pytest.raises(ValueError, match="WeibullLikelihood's time to an event"):
        p.predictUncertainty(SX)
    assert len(p._chain.calls) == n_calls
    # survival: a host loop of predictiveCDF, one call per time, every target of a call that time
    times = [0.5, 1.0, 4.0]
    S = p.survival(SX, times, n=2)
    assert S.shape == (3, 2, 3) and S.dtype == np.float64 and len(p._chain.calls) == n_calls + 3
    for j, t in enumerate(times):
        th, _pr, yy, kw = p._chain.calls[n_calls + j]
        assert np.array_equal(th[:, 0], [0, 2, 4]) and yy.shape == (3, 2) and np.all(yy == np.float32(t)) and kw["likelihood"] == 16
        assert np.allclose(S[j], math.exp(-t), rtol=1e-12)
    assert np.all(S[0] > S[1]) and np.all(S[1] > S[2])
    n_calls = len(p._chain.calls)
    for bad in ([], [0.0], [-1.0], [1.0, float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="times must be finite and > 0"):
            p.survival(SX, bad)
    with pytest.raises(ValueError, match="needs a WeibullLikelihood"):
        p.survival(SX, [1.0], likelihood=GammaLikelihood(shape=2.0))
    assert len(p._chain.calls) == n_calls
    g_ = stub_predictor(GammaLikelihood(shape=2.0), HYPERS)
    g_._chain = WeibullStubChain()
    with pytest.raises(ValueError, match="needs a WeibullLikelihood"):
        g_.survival(SX, [1.0])
    assert g_.survival(SX, [1.0], likelihood=lik).shape == (1, 2, 3)
    # noiseVariance: (g1 E[lambda], g1^2 Var[lambda] + (g2 - g1^2) E[lambda^2]) on the host, from the device's mean 6 and variance 2
    m, v = p.predictMoments(SX, noiseVariance=True)
    assert p._chain.calls[-1][3]["xform"] == nat.XFORM_EXP
    g1, g2 = math.gamma(1.0 + 1.0 / 3.0), math.gamma(1.0 + 2.0 / 3.0)
    assert np.allclose(m, 6.0 * g1, rtol=1e-15) and np.allclose(v, g1 * g1 * 2.0 + (g2 - g1 * g1) * (2.0 + 36.0), rtol=1e-14)
    m, v = p.predictMoments(SX)
    assert np.all(m == 6.0) and np.all(v == 2.0) and p._chain.calls[-1][3]["xform"] == nat.XFORM_EXP
    for kw in ({"sd": 2.0}, {"mean": 1.0}, {"transform": "none"}, {"countVariance": True}):
        with pytest.raises(ValueError, match="WeibullLikelihood"):
            p.predictMoments(SX, noiseVariance=True, **kw)


# ---------------------------------------------------------------------------------------------------------------------- codes and plumbing
def test_codes_shape_and_cache_key():
    from tensorbnn_amd import _native as nat, jit
    assert jit.LIK_WEIBULL == 24
    assert jit.lik_code(nat.LIK_WEIBULL) == 27 and jit.lik_code(nat.LIK_WEIBULL, True) == 31
    # every existing code keeps its value
    assert (jit.LIK_GAUSS, jit.LIK_BERN, jit.LIK_CAT, jit.LIK_POIS, jit.LIK_WEIGHTED, jit.LIK_STUDENT, jit.LIK_NEGBIN, jit.LIK_HETERO,
            jit.LIK_GAMMA) == (0, 1, 2, 3, 4, 8, 8, 16, 16)
    assert [jit.lik_code(k) for k in (nat.LIK_GAUSSIAN, nat.LIK_FIXED_GAUSSIAN, nat.LIK_BERNOULLI, nat.LIK_CATEGORICAL, nat.LIK_POISSON,
                                      nat.LIK_STUDENT_T, nat.LIK_NEG_BINOMIAL, nat.LIK_HETERO_GAUSSIAN, nat.LIK_GAMMA)] == [0, 0, 1, 2, 3, 8, 11, 16, 19]
    assert (nat.LIK_GAUSSIAN, nat.LIK_FIXED_GAUSSIAN, nat.LIK_BERNOULLI, nat.LIK_CATEGORICAL, nat.LIK_POISSON, nat.LIK_STUDENT_T,
            nat.LIK_NEG_BINOMIAL, nat.LIK_HETERO_GAUSSIAN, nat.LIK_GAMMA, nat.LIK_WEIBULL) == (0, 1, 2, 3, 5, 8, 10, 12, 14, 16)
    for unknown in (15, 17):
        assert jit.lik_code(unknown) == 0                                  # (no code of its own: tbnn_create refuses the value)
    layers = layers_for([30, 80, 80, 10], nat.ACT_RELU)
    g, gm, t, tw = (jit.shape_of(layers, lk, w) for lk, w in ((nat.LIK_POISSON, False), (nat.LIK_GAMMA, False),
                                                              (nat.LIK_WEIBULL, False), (nat.LIK_WEIBULL, True)))
    assert g[:3] == gm[:3] == t[:3] == tw[:3] and (g[3], gm[3], t[3], tw[3]) == (3, 19, 27, 31)
    assert len({jit.cache_key(*s) for s in (g, gm, t, tw)}) == 4
    src = jit.source(*t, "mid")
    inner = src.split("Shape<")[1].split(">")[0]
    assert "SHAPE_LIK_POIS | SHAPE_LIK_WEIBULL" in inner and "WEIGHTED" not in inner and src != jit.source(*g, "mid") and src != jit.source(*gm, "mid")
    inner = jit.source(*tw, "mid").split("Shape<")[1].split(">")[0]
    assert "SHAPE_LIK_WEIBULL" in inner and "SHAPE_LIK_WEIGHTED" in inner
    assert jit.source(*gm, "mid").split("Shape<")[1].split(">")[0].split(", ")[2] == "SHAPE_LIK_POIS | SHAPE_LIK_GAMMA"       # untouched
    assert jit.families([5, 20, 20, 3], jit.LIK_POIS | jit.LIK_WEIBULL) != []


@pytest.mark.parametrize("dims", DIMS_GRID, ids=lambda d: "-".join(map(str, d)))
def test_families_equal_the_poisson_reach(dims):
    from tensorbnn_amd import jit
    want = jit.families(dims, jit.LIK_POIS)
    assert jit.families(dims, jit.LIK_POIS | jit.LIK_WEIBULL) == want
    assert jit.families(dims, jit.LIK_POIS | jit.LIK_WEIBULL | jit.LIK_WEIGHTED) == jit.families(dims, jit.LIK_POIS | jit.LIK_WEIGHTED) == want


def _admission(dims, act_last, lik, fixed_sd=0.1, lik_df=0.0):
    from tensorbnn_amd import _native as nat
    layers = layers_for(dims, nat.ACT_RELU, act_last)
    arr = (nat.LayerDesc * len(layers))(*[nat.LayerDesc(*l) for l in layers])
    desc = nat.NetDesc(len(layers), arr, lik, fixed_sd, nat.KERNEL_AUTO, lik_df)
    rc = nat.lib.tbnn_fused_kernel_available(C.byref(desc))
    return rc, nat.lib.tbnn_last_error().decode()


def test_c_abi_admission(monkeypatch):
    from tensorbnn_amd import _native as nat
    # (the ahead-of-time tables are what is judged: a run-time library that an earlier test of the same process registered does not count)
    monkeypatch.setenv("TBNN_REGISTERED", "0")
    assert C.sizeof(nat.NetDesc) == 32 and nat.NetDesc.lik_df.offset == 28 and nat.lib.tbnn_abi_version() == 3
    for dims in ([5, 8, 1], [5, 8, 3], [5, 8, 40]):                       # any d_out >= 1
        assert _admission(dims, nat.ACT_NONE, nat.LIK_WEIBULL, lik_df=1.5)[0] >= 0
        for act in (nat.ACT_TANH, nat.ACT_SIGMOID, nat.ACT_EXP):         # the output is the log of the scale: no last activation
            rc, err = _admission(dims, act, nat.LIK_WEIBULL, lik_df=1.5)
            assert rc == -1 and "Weibull" in err and "no activation" in err, err
    for df in (0.0, -1.0, float("nan"), float("inf")):
        rc, err = _admission([5, 8, 1], nat.ACT_NONE, nat.LIK_WEIBULL, lik_df=df)
        assert rc == -1 and "lik_df" in err and "Weibull" in err, (df, err)
    for sd in (0.0, -0.5, float("nan")):                                  # fixed_sd is not read
        assert _admission([5, 8, 1], nat.ACT_NONE, nat.LIK_WEIBULL, fixed_sd=sd, lik_df=1.5)[0] >= 0
    for unknown in (15, 17, 18, 32):
        rc, err = _admission([5, 8, 3], nat.ACT_NONE, unknown, lik_df=1.5)
        assert rc == -1 and "unknown likelihood" in err
    # an ahead-of-time Gaussian table is no table for the Weibull network of the same layers
    for dims in ([7, 33, 18, 50, 2], [5, 50, 50, 50, 1]):
        assert _admission(dims, nat.ACT_NONE, nat.LIK_FIXED_GAUSSIAN)[0] > 0
        assert _admission(dims, nat.ACT_NONE, nat.LIK_WEIBULL, lik_df=1.5)[0] == 0


def test_header_text():
    import os
    from tensorbnn_amd import _native as nat
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    hdr = open(os.path.join(root, "include", "tbnn.h")).read()
    assert "TBNN_LIK_WEIBULL = 16" in hdr and "TBNN_LIK_GAMMA = 14" in hdr
    assert "#define TBNN_ABI_VERSION 3" in hdr and nat.ABI_VERSION == 3
    assert "log p = log k + (k - 1) log t - k f - u" in hdr and "log S = -u" in hdr and "dL/df = k (u - d)" in hdr
    common = open(os.path.join(root, "tensorbnn_amd", "csrc", "common.hpp")).read()
    assert "enum { SHAPE_LIK_WEIBULL = 8 | 16 };" in common and "weibull_term" in common and "weibull_elem" in common


@pytest.mark.parametrize("dims,skip,family,name,weighted", [
    ([3, 12, 12, 1], "", "fast3", b"<relu,none,weibull;3,12,12,1>", False),
    ([20, 64, 64, 3], "wide", "mid", b"jit-mid<relu,none,weibull,weighted;20,64,64,3>", True),
])
def test_weibull_library_cross_compiles_checked(tmp_path, monkeypatch, dims, skip, family, name, weighted):
    """jit.build of a narrow and a weighted mid-width Weibull shape: hipcc for gfx950 through checked_compile, the MFMA hazard check clean,
    the kernel name carrying weibull; a Gamma table is no table for the Weibull network of the same layers"""
    import os
    from tensorbnn_amd import _native as nat, jit
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    monkeypatch.setenv("TBNN_JIT_DIR", str(tmp_path))
    monkeypatch.setenv("TBNN_JIT_SKIP", skip)
    so = jit.build(layers_for(dims, nat.ACT_RELU), nat.LIK_WEIBULL, weighted=weighted)
    assert so and os.path.exists(so)
    st = jit.lint_status(so)
    assert st.startswith(family + ":") and "listing checked" in st and "disassembly clean" in st, st
    lib = C.CDLL(so)
    buf = (C.c_char * 4096)()
    assert lib.tbnn_jit_ops(buf) == 0
    assert name in bytes(buf), bytes(buf)[:400]
    if weighted:
        return
    monkeypatch.delenv("TBNN_REGISTERED", raising=False)
    gso = jit.build(layers_for(dims, nat.ACT_RELU), nat.LIK_GAMMA)
    assert gso and gso != so
    before = _admission(dims, nat.ACT_NONE, nat.LIK_WEIBULL, lik_df=2.0)[0]
    assert nat.lib.tbnn_register_kernel_lib(gso.encode()) >= 0, nat.lib.tbnn_last_error().decode()
    assert _admission(dims, nat.ACT_NONE, nat.LIK_GAMMA, lik_df=2.0)[0] > 0
    assert _admission(dims, nat.ACT_NONE, nat.LIK_WEIBULL, lik_df=2.0)[0] == before
    if before == 0:
        assert nat.lib.tbnn_register_kernel_lib(so.encode()) >= 0, nat.lib.tbnn_last_error().decode()
        assert _admission(dims, nat.ACT_NONE, nat.LIK_WEIBULL, lik_df=2.0)[0] > 0
