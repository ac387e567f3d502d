"""GPU: the ensemble entry points under TBNN_LIK_WEIBULL -- tbnn_ensemble_loglik, tbnn_ensemble_loo, tbnn_ensemble_predictive and the
predictor's predictiveQuantiles / predictiveInterval / predictiveCDF / survival / predictMoments(noiseVariance=True) -- with m = 24
networks of 1-16-16-1 over 257 rows (the sizes of tests/test_gpu_hetero_ensemble.py), events and right-censored rows mixed, against fp64
NumPy / SciPy applied to the fp32 predictions Chain.forward_many returns for the same thetas and rows: both sides start from the same
bits, so the tests isolate the reductions.  Every test fails on a library without the likelihood (code 16 is an unknown likelihood there).

Log-likelihoods: an event row gives log k + (k - 1) log t - k f - u, a censored row -u, u = exp(k (log t - f)); both sides evaluate that
fp64 expression from the same fp32 outputs, so the band is rounding alone: 16 ulp64 of the magnitudes that enter a term, where u counts
with 1 + k |log t - f| (the rounding of the exponent is a relative error of u).  LOO, WAIC and lppd against tests/psis_ref.py fed with
the device's matrix, by the bound of tests/test_gpu_loo.py.

Predictive CDF: F(t) = sum_i w_i / W (-expm1(-u_i)) at t = |y|, within T(m) = (m + 8) U + 4 P_FIG of tests/test_gpu_gamma_predictive.py,
the bound of its continuous kind.  Its per-term figure P_FIG = 4.8e-15 covers this term: a term 1 - e^-u moves by u e^-u <= 0.37 times the
relative error of u, which is (2 + k |log t - f|) U from the logarithm, the product and the exponential -- below 40 U = 4.4e-15 while
k |log t - f| <= 100, and beyond that u e^-u is 0 or u is below 1e-43.
Quantiles: the property of tests/test_gpu_gamma_predictive.py -- q > 0, monotone in p, F_ref(q) >= p - T and F_ref four fp64 steps below
q <= p + T -- at five probabilities, 0.001 and 0.999 among them."""
import ctypes as C
import math

import numpy as np
import pytest

import tbnn_oracle as o
import weibull_ref as wr
from tensor_checks import layers_of
from test_gpu_gamma_predictive import T
from test_gpu_predictive import U, int_weights, mix

pytestmark = pytest.mark.gpu

LIK = wr.LIK_WEIBULL
M, N, DIMS, K = 24, 257, [1, 16, 16, 1], 1.5
PROBS = [0.001, 0.05, 0.5, 0.95, 0.999]


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """the two run-time shapes of test_predictor_end_to_end, compiled before any test touches the GPU (cached)"""
    from tensorbnn_amd import jit
    layers = [[DIMS[i], DIMS[i + 1], 2 if i < len(DIMS) - 2 else 0, 0] for i in range(len(DIMS) - 1)]      # tanh, Cauchy priors
    jobs = [{"layers": layers, "likelihood": lik, "skip": "", "flags": ""} for lik in (LIK, 1)]
    assert jit.prebuild(jobs, processes=2) == len(jobs)


_SETUP = {}


def setup(native, lik=LIK):
    """(chain, X, Y, thetas, f): the generic kernel (a row per thread: a row's forward bits do not depend on its block), 24 networks around
    the oracle's initial state, signed targets drawn from the model (events and censored rows); computed once and left unchanged"""
    if "data" not in _SETUP:
        spec, X, Y, theta, _eta = wr.problem_of(DIMS, N, o.ACT_TANH, o.PRIOR_CAUCHY, K)
        rng = np.random.default_rng(7)
        thetas = (theta[None] + 0.3 * rng.standard_normal((M, spec.n_params))).astype(np.float32)
        assert (Y > 0).sum() > 100 and (Y < 0).sum() > 50
        _SETUP["data"] = (spec, X, Y, thetas)
    spec, X, Y, thetas = _SETUP["data"]
    kw = dict(lik_df=K) if lik == LIK else dict(fixed_sd=1.0)
    ch = native.Chain(layers_of(spec), likelihood=lik, kernel=native.KERNEL_GENERIC, **kw)
    f = ch.forward_many(thetas, X=X)
    assert f.shape == (M, 1, N) and np.all(np.isfinite(f))
    return ch, X, Y, thetas.copy(), f


def wei_terms(y, f, k):
    """1 - exp(-u_i) per network at t = |y|, 0 at t = 0: y [d_out, n] (or broadcastable), f fp32 [m, d_out, n]"""
    t = np.abs(np.asarray(y, dtype=np.float64))
    kk = float(np.float32(k))                                       # the shape as the library holds it: an fp32
    with np.errstate(over="ignore", divide="ignore"):
        u = np.exp(kk * (np.log(t)[None] - f.astype(np.float64)))
    return np.where(t[None] > 0, -np.expm1(-u), 0.0)


def F_ref(y, f, w, k=K):
    """F(|y|); networks of weight 0 are left out of the sum (they add nothing, whatever they hold)"""
    if w is not None:
        keep = np.asarray(w) > 0
        f, w = f[keep], np.asarray(w)[keep]
    return mix(wei_terms(y, f, k), w)


def check_quantiles(tag, q, probs, f, w, k=K):
    m = f.shape[0]
    t = T(m)
    worst = 0.0
    for j, p in enumerate(probs):
        assert np.all(np.isfinite(q[j])) and np.all(q[j] > 0), (tag, p)
        at = F_ref(q[j], f, w, k)
        below = F_ref(q[j] - 4 * np.spacing(q[j]), f, w, k)
        worst = max(worst, float((p - at).max()), float((below - p).max()))
        assert np.all(at >= p - t), (tag, p, float((p - at).max()), t)
        assert np.all(below <= p + t), (tag, p, float((below - p).max()), t)
    print(f"[weibull predictive] {tag}: m={m} k={k:g} quantiles, worst excess over p {worst:.3e} (T {t:.3e})")
    order = np.argsort(probs)
    assert np.all(np.diff(q[order], axis=0) >= 0), tag       # monotone in p


def test_loglik_loo_and_waic(native):
    from psis_ref import psis_ref
    from test_gpu_ensemble import logsumexp_rows
    from test_gpu_loo import TOL
    ch, X, Y, thetas, f = setup(native)
    f64 = f.astype(np.float64)
    kk = float(np.float32(K))
    l = np.stack([wr.terms(f64[i], Y, kk).sum(axis=0) for i in range(M)])                       # [m, n]
    lt = np.log(np.abs(Y.astype(np.float64))).T[None]                                            # [1, 1, n]
    u = np.exp(kk * (lt - f64))
    mag = (np.where(Y.T[None] > 0, abs(math.log(kk)) + np.abs((kk - 1.0) * lt) + np.abs(kk * f64), 0.0)
           + u * (1.0 + kk * np.abs(lt - f64))).sum(axis=1)
    got = ch.ensemble_loo(thetas, Y=Y, X=X, pointwise=True)
    again = ch.ensemble_loo(thetas, Y=Y, X=X, likelihood=LIK, pointwise=True)
    for key in got:
        assert np.array_equal(got[key], again[key], equal_nan=True), key
    pw = got["pointwise"]
    e, tol = np.abs(pw - l), 16 * U * mag
    print(f"[weibull] ensemble: matrix against the fp64 definition, err max {e.max():.3e}, worst err/tol {np.max(e / tol):.3f}")
    assert pw.shape == (M, N) and np.all(np.isfinite(pw)) and np.all(e <= tol)
    # a censored row gives the log survival function: never positive, and above the same row's value as an event less its surplus
    cens = Y[:, 0] < 0
    assert np.all(pw[:, cens] <= 0.0)
    ref = psis_ref(pw, 1.0)
    for key in ("elpd_loo", "pareto_k", "lppd", "p_waic"):
        g_, w_ = got[key], ref[key]
        assert np.array_equal(np.isposinf(g_), np.isposinf(w_)) and np.array_equal(np.isnan(g_), np.isnan(w_)), key
        fin = np.isfinite(w_)
        d = np.abs(g_[fin] - w_[fin]) / (np.abs(w_[fin]) if key in ("elpd_loo", "lppd") else 1.0)
        print(f"[weibull] ensemble: {key} diff {d.max(initial=0.0):.3e} (bound {TOL:.3e})")
        assert d.max(initial=0.0) <= TOL, key
    rng = np.random.default_rng(31)
    for wts in (None, (rng.random(M) * (rng.random(M) > 0.2)).astype(np.float32)):
        per_net, rows = ch.ensemble_loglik(thetas, Y=Y, X=X, weights=wts)
        assert np.all(np.abs(per_net - pw.sum(axis=1)) <= N * U * np.abs(pw).sum(axis=1))
        ww = np.ones(M) if wts is None else wts.astype(np.float64)
        want = logsumexp_rows(pw, ww) - math.log(ww.sum())
        assert np.all(np.abs(rows - want) <= (M + 8) * U + 4 * U * np.abs(want))
        if wts is None:
            assert np.array_equal(rows.view(np.uint64), got["lppd"].view(np.uint64))
    ch.close()
    # a forward chain of another likelihood (the predictor's is a fixed-sd Gaussian one) needs set_lik_df first, then gives the same bits
    gch, _X, _Y, _th, _f = setup(native, o.LIK_FIXED_GAUSSIAN)
    for call in (lambda: gch.ensemble_loo(thetas, Y=Y, X=X, likelihood=LIK), lambda: gch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=LIK),
                 lambda: gch.ensemble_predictive(thetas, probs=[0.5], X=X, likelihood=LIK)):
        with pytest.raises(native.TbnnError, match="TBNN_LIK_WEIBULL needs the shape: call tbnn_set_lik_df"):
            call()
    gch.set_lik_df(K)
    other = gch.ensemble_loo(thetas, Y=Y, X=X, likelihood=LIK, pointwise=True)
    assert np.array_equal(other["pointwise"].view(np.uint64), pw.view(np.uint64))
    gch.close()


def test_predictive_cdf_and_quantiles(native):
    ch, X, Y, thetas, f = setup(native)
    t = T(M)
    real_w = (np.random.default_rng(3).random(M) + 0.05).astype(np.float32)
    real_w[5] = 0.0
    Yz = Y.copy()
    Yz[0, 0] = 0.0                                                   # t = 0: F = 0
    for tag, w in (("equal", None), ("importance weights", real_w), ("integer weights", int_weights(M))):
        q, F, Fb = ch.ensemble_predictive(thetas, probs=PROBS, Y=Yz, X=X, weights=w)
        assert q.shape == (5, 1, N) and F.shape == (1, N) and Fb is None and q.dtype == F.dtype == np.float64
        err = np.abs(F - F_ref(Yz.T, f, w))
        print(f"[weibull predictive] {tag}: CDF err max {err.max():.3e} (T {t:.3e})")
        assert np.all(err <= t), (tag, float(err.max()))
        assert F[0, 0] == 0.0 and np.all((F >= 0) & (F <= 1))
        check_quantiles(tag, q, PROBS, f, w)
        # the same bits from run to run
        again = ch.ensemble_predictive(thetas, probs=PROBS, Y=Yz, X=X, weights=w)
        assert again[2] is None and all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(again[:2], (q, F)))
    # the CDF reads |y|: flipping every sign changes nothing
    F_flip = ch.ensemble_predictive(thetas, Y=-Yz, X=X, weights=real_w)[1]
    F_same = ch.ensemble_predictive(thetas, Y=Yz, X=X, weights=real_w)[1]
    assert np.array_equal(F_flip.view(np.uint64), F_same.view(np.uint64))
    # a network of weight 0 holding NaN is not looked at: the bits of the run above; with equal weights it counts and everything is NaN
    q, F, _b = ch.ensemble_predictive(thetas, probs=PROBS, Y=Yz, X=X, weights=real_w)
    th = thetas.copy()
    th[5, -1] = np.nan
    assert np.isnan(ch.forward_many(th, X=X)[5]).all()
    q2, F2, _b = ch.ensemble_predictive(th, probs=PROBS, Y=Yz, X=X, weights=real_w)
    assert np.array_equal(q2.view(np.uint64), q.view(np.uint64)) and np.array_equal(F2.view(np.uint64), F.view(np.uint64))
    q3, F3, _b = ch.ensemble_predictive(th, probs=PROBS, Y=Yz, X=X)
    assert np.isnan(q3).all() and np.isnan(F3).all()
    # a NaN target: a NaN CDF in that element alone
    Yn = Yz.copy()
    Yn[11, 0] = np.nan
    Fn = ch.ensemble_predictive(thetas, Y=Yn, X=X, weights=real_w)[1]
    assert np.isnan(Fn[0, 11]) and np.isnan(Fn).sum() == 1
    ch.close()


def test_identical_networks_give_one_weibull(native):
    """five copies of one network, weighted or not: q = exp(f) (-log1p(-p))^(1/k) within 8 ulp64 plus the conditioning of the root -- F is
    known to E = 4 P_FIG + (m + 5) U of tests/test_gpu_gamma_predictive.py and has the slope (k / q) u e^-u, u = -log1p(-p), there"""
    from test_gpu_gamma_predictive import P_FIG
    ch, X, _Y, thetas, f = setup(native)
    kk = float(np.float32(K))
    th = np.repeat(thetas[:1], 5, axis=0)
    pr = np.asarray(PROBS)
    u = -np.log1p(-pr)[:, None, None]
    want = np.exp(f[0].astype(np.float64))[None] * u ** (1.0 / kk)
    slope = (kk / want) * u * np.exp(-u)
    for w in (None, int_weights(5)):
        q = ch.ensemble_predictive(th, probs=PROBS, X=X, weights=w)[0]
        tol = (4 * P_FIG + 10 * U) / slope + 8 * np.spacing(want)
        err = np.abs(q - want)
        print(f"[weibull predictive] identical networks: worst err / tol {np.max(err / tol):.3f}, worst err {np.max(err / np.spacing(want)):.1f} ulp64 of q*")
        assert np.all(err <= tol)
    ch.close()


def test_far_off_network_and_tiny_shape(native):
    """one network whose log-scale is 300 below the others, judged with k = 3 on a Gaussian handle: at every trial point its
    u = exp(k (log t - f_i)) is past the fp64 range, its CDF term is 1 and its density term 0 (formed as exp(z - u), not as inf * 0), so
    the CDF and the quantiles outside that network's own mass meet the same checks as ever.  A shape so small that the standard quantile (-log1p(-p))^(1/k) leaves fp64's
    normal range is refused before anything is staged."""
    ch, X, Y, thetas, _f = setup(native, o.LIK_FIXED_GAUSSIAN)
    th = thetas.copy()
    far = M - 1                                                      # (int_weights gives the last network a positive weight)
    th[far, -1] = np.float32(-300.0)
    ch.set_lik_df(3.0)
    f = ch.forward_many(th, X=X)
    assert np.all(3.0 * (np.log(np.abs(Y.T.astype(np.float64))) - f[far].astype(np.float64)) > 709.0) and np.all(np.isfinite(f))
    for w in (None, int_weights(M)):
        assert w is None or w[far] > 0
        q, F, _b = ch.ensemble_predictive(th, probs=PROBS, Y=Y, X=X, likelihood=LIK, weights=w)
        err = np.abs(F - F_ref(Y.T, f, w, 3.0))
        print(f"[weibull predictive] far-off network: CDF err max {err.max():.3e} (T {T(M):.3e})")
        assert np.all(err <= T(M))
        check_quantiles("far-off network", q[1:], PROBS[1:], f, w, 3.0)
        # (p = 0.001 lies inside the far-off network's own mass: its quantile is e^-300 times the bracket's upper end, which the search's
        # arithmetic midpoints do not reach in ENS_PRED_PASSES = 256 trials -- a limit of the positive-axis search, Gamma's too: DESIGN 4.6.
        # What is returned is an upper end with F >= p, positive and finite.)
        assert np.all(np.isfinite(q[0])) and np.all(q[0] > 0) and np.all(F_ref(q[0], f, w, 3.0) >= PROBS[0] - T(M))
    ch.set_lik_df(1e-3)
    with pytest.raises(native.TbnnError, match="shape is too small"):
        ch.ensemble_predictive(thetas, probs=[0.5, 0.999], X=X, likelihood=LIK)
    with pytest.raises(native.TbnnError, match="shape is too small"):
        ch.ensemble_predictive(thetas, probs=[0.001], X=X, likelihood=LIK)
    ch.set_lik_df(K)
    assert np.all(np.isfinite(ch.ensemble_predictive(thetas, probs=[0.5], X=X, likelihood=LIK)[0]))
    ch.close()


def test_row_blocks_carry_over(native, monkeypatch):
    """257 rows in blocks of 64 (five blocks, the last of one row), and the staged rows and targets: both outputs, the log-likelihood
    sums and the LOO results bit for bit those of the single-block call"""
    ch, X, Y, thetas, _f = setup(native)
    kw = {"weights": int_weights(M), "probs": PROBS}
    whole = ch.ensemble_predictive(thetas, Y=Y, X=X, **kw)
    ll = ch.ensemble_loglik(thetas, Y=Y, X=X)
    loo = ch.ensemble_loo(thetas, Y=Y, X=X)
    budget = M * 64 + 7
    assert max(64, budget // M // 64 * 64) == 64 and -(-N // 64) == 5
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    cut = ch.ensemble_predictive(thetas, Y=Y, X=X, **kw)
    ll_cut = ch.ensemble_loglik(thetas, Y=Y, X=X)
    loo_cut = ch.ensemble_loo(thetas, Y=Y, X=X)
    ch.set_data(X, Y)
    staged = ch.ensemble_predictive(thetas, which=0, cdf=True, **kw)
    monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
    for x, y, z in zip(whole[:2], cut[:2], staged[:2]):
        assert x is not None and np.array_equal(x.view(np.uint64), y.view(np.uint64)) and np.array_equal(x.view(np.uint64), z.view(np.uint64))
    assert whole[2] is None and cut[2] is None and staged[2] is None
    for a_, b_ in zip(ll, ll_cut):
        assert np.array_equal(a_.view(np.uint64), b_.view(np.uint64))
    for key in loo:
        assert np.array_equal(loo[key], loo_cut[key], equal_nan=True), key
    ch.close()


def test_refusals_by_name(native):
    dp = C.POINTER(C.c_double)
    ch, X, Y, thetas, _f = setup(native)
    before = ch.forward_many(thetas, X=X)
    with pytest.raises(native.TbnnError, match="TBNN_LIK_WEIBULL is not built"):
        ch.ensemble_crps(thetas, Y=Y, X=X)
    with pytest.raises(native.TbnnError, match="not of TBNN_LIK_WEIBULL"):
        ch.ensemble_uncertainty(thetas, X=X)
    with pytest.raises(native.TbnnError, match="descriptor"):
        ch.set_lik_df(2.0)
    # cdf_below_out is refused: a continuous CDF has no step; nothing is written
    lib, p = native.lib, native._p
    qo, Fo, Bo = np.full((5, 1, N), 7.0), np.full((1, N), 7.0), np.full((1, N), 7.0)
    pr = np.asarray(PROBS, dtype=np.float64)
    rc = lib.tbnn_ensemble_predictive(ch._h, p(thetas), M, thetas.shape[1], LIK, None, None, 1, p(X), p(Y), N, pr.ctypes.data_as(dp), 5,
                                      qo.ctypes.data_as(dp), Fo.ctypes.data_as(dp), Bo.ctypes.data_as(dp))
    assert rc < 0 and "continuous CDF has no step" in lib.tbnn_last_error().decode()
    assert np.all(qo == 7.0) and np.all(Fo == 7.0) and np.all(Bo == 7.0)
    assert np.array_equal(ch.forward_many(thetas, X=X), before)
    ch.close()


# ---------------------------------------------------------------------------------------------------------------- predictor, end to end
def test_predictor_end_to_end(tmp_path, monkeypatch, native):
    """censored times trained for a few epochs under WeibullLikelihood(shape=1.5), then the saved run: the predictive interval is ordered
    and positive, the PIT is the mixture CDF of the saved networks at |y|, the survival curve decreases in t and is 1 - predictiveCDF,
    noiseVariance gives (E[m_i], Var[m_i] + E[v_i]) of the networks' own Weibull means and variances, and CRPS and the entropy split are
    refused"""
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.likelihood import WeibullLikelihood
    from tensorbnn_amd.network import network
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    rng = np.random.default_rng(71)
    X = rng.uniform(-2, 2, (300, 1)).astype(np.float32)
    lam = np.exp(1.0 + np.sin(2 * X.astype(np.float64)))
    t_ev, t_ce = lam * rng.weibull(K, (300, 1)), 1.3 * lam * rng.weibull(K, (300, 1))
    Y = WeibullLikelihood.encode(np.maximum(np.minimum(t_ev, t_ce), 1e-30), t_ev <= t_ce)
    assert 0.2 < np.mean(Y < 0) < 0.6
    lik = WeibullLikelihood(shape=K)
    net = network(np.float32, 1, X, Y, X[:50], Y[:50])
    net.add(DenseLayer(1, 16, seed=1000)); net.add(Tanh())
    net.add(DenseLayer(16, 16, seed=2000)); net.add(Tanh())
    net.add(DenseLayer(16, 1, seed=3000))
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    net.train(30, 2, lik, folderName="wei", networksPerFile=1, verbose=False)
    assert ",weibull;" in net._chain.kernel_name, net._chain.kernel_name
    p = predictor(str(tmp_path / "wei") + "/", likelihood=lik)
    m = p.numNetworks
    assert m >= 4
    lower, median, upper = p.predictiveInterval(X, level=0.9)
    assert lower.shape == median.shape == upper.shape == (1, 300)
    assert np.all(lower > 0) and np.all(lower < median) and np.all(median < upper)
    q = p.predictiveQuantiles(X, [0.05, 0.5, 0.95])
    assert np.array_equal(q[0], lower) and np.array_equal(q[1], median) and np.array_equal(q[2], upper)
    f = np.array(p.predict(X))
    check_quantiles("predictor", q, [0.05, 0.5, 0.95], f, None)
    F = p.predictiveCDF(X, Y)
    assert isinstance(F, np.ndarray) and np.all(np.abs(F - F_ref(Y.T, f, None)) <= T(m))
    # the survival curve: decreasing in t, 1 - predictiveCDF at each time, the bits of a call with that time in every target
    times = [0.25, 1.0, 3.0, 9.0, 40.0]
    S = p.survival(X, times)
    # (S is 1 - F as the device returns F: the sum of the normalised weights may exceed 1 by a rounding, so S >= -T, not >= 0)
    assert S.shape == (5, 1, 300) and S.dtype == np.float64 and np.all((S >= -T(m)) & (S <= 1))
    assert np.all(np.diff(S, axis=0) <= 0) and np.all(S[0] > S[-1])
    for j, tt in enumerate(times):
        Fj = p.predictiveCDF(X, np.full((300, 1), tt, dtype=np.float32))
        assert np.array_equal(S[j], 1.0 - Fj)
        assert np.all(np.abs((1.0 - S[j]) - F_ref(np.full((1, 300), np.float32(tt)), f, None)) <= T(m))
    with pytest.raises(ValueError, match="times must be finite and > 0"):
        p.survival(X, [1.0, 0.0])
    # noiseVariance: (E[m_i], Var[m_i] + E[v_i]) of the networks' own Weibull means m_i = lambda_i Gamma(1 + 1/k) and variances
    # v_i = lambda_i^2 (Gamma(1 + 2/k) - Gamma(1 + 1/k)^2).  The moments of lambda = exp(f) are the device's (its exp runs in fp32: judged
    # by tests/test_gpu_ensemble.py's check_moments); the host's part is exact in them; and the whole against the definition in fp64 from the
    # fp32 predictions, within the relative error of the device's fp32 exp (XFORM_ULP ulp32, an ulp32 at most 2^-23 of its value), twice
    # that for its square
    from test_gpu_ensemble import XFORM_ULP, check_moments
    sc, var = p.predictMoments(X)
    check_moments("predictor, the scale", sc, var, f, None, xform="exp")
    g1, g2 = math.gamma(1.0 + 1.0 / K), math.gamma(1.0 + 2.0 / K)
    mean, tot = p.predictMoments(X, noiseVariance=True)
    assert np.array_equal(mean, g1 * sc) and np.array_equal(tot, g1 * g1 * var + (g2 - g1 * g1) * (var + sc * sc)) and np.all(tot > g1 * g1 * var)
    lam_i = np.exp(f.astype(np.float64))                                                    # [m, 1, rows]
    mi, vi = lam_i * g1, lam_i ** 2 * (g2 - g1 * g1)
    rel = XFORM_ULP["exp"] * 2.0 ** -23
    assert np.allclose(mean, mi.mean(axis=0), rtol=rel + 1e-14, atol=0)
    assert np.allclose(tot - g1 * g1 * var, vi.mean(axis=0), rtol=2 * rel + rel * rel + 1e-13, atol=0)
    # every second network, reweighted; Weibull times take no de-normalisation
    w = np.arange(1, len(range(0, m, 2)) + 1, dtype=np.float32)
    q2 = p.predictiveQuantiles(X, [0.25, 0.75], n=2, weights=w)
    check_quantiles("predictor, every second network", q2, [0.25, 0.75], f[::2], w)
    with pytest.raises(ValueError, match="WeibullLikelihood"):
        p.predictiveQuantiles(X, [0.5], sd=2.0)
    with pytest.raises(ValueError, match="not built for a WeibullLikelihood"):
        p.crps(X, Y)
    with pytest.raises(ValueError, match="WeibullLikelihood"):
        p.predictUncertainty(X)
    per_net, per_row = p.logPredictiveDensity(X, Y)
    assert per_net.shape == (m,) and np.all(np.isfinite(per_row))
    loo, waic = p.loo(X, Y), p.waic(X, Y)
    assert np.isfinite(loo["elpd_loo"]) and np.isfinite(waic["elpd_waic"])
    cmp_ = predictor.compareLoo(loo, loo)
    assert cmp_["elpd_diff"] == 0.0
    p.trainProbs(X, Y, 1, lik)
    assert len(p.weightsTrain) == m and np.all(np.isfinite(np.asarray(p.weightsTrain, dtype=np.float64)))
