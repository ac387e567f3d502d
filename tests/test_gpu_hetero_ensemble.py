"""GPU: the ensemble entry points under TBNN_LIK_HETERO_GAUSSIAN -- tbnn_ensemble_loglik, tbnn_ensemble_loo, tbnn_ensemble_predictive and
predictor.predictMoments(noiseVariance=True) -- with m = 24 networks of 1-16-16-2 over 257 rows, against fp64 NumPy / SciPy applied to the
fp32 predictions Chain.forward_many returns for the same thetas and rows: both sides start from the same bits, so the tests isolate the
reductions.  Every test fails on a library without the likelihood (code 12 is an unknown likelihood there).

Log-likelihoods: both sides evaluate the fp64 definition -1/2 log(2 pi) - gc - 1/2 r^2 exp(-2 gc) from the same fp32 outputs; the band is
rounding alone, 16 ulp64 of the magnitudes that enter a term (the rule of tests/test_gpu_negbin.py::test_ensemble_loglik_and_loo).  LOO,
WAIC and lppd against tests/psis_ref.py fed with the device's matrix, by the bound of tests/test_gpu_loo.py.

Predictive CDF: F(y) = sum_i w_i / W Phi((y - f_i) / s_i), s_i = exp(gc_i), against scipy.special.ndtr, within T(m) = (m + 8) U + 4 PHI_FIG
of tests/test_gpu_predictive.py (its Gaussian CDF check; the device's c_i = exp(-gc_i) / sqrt 2 is off by an ulp or two of itself, which
moves a term by at most |z| phi(z) 2 U <= 0.5 U: inside the 4 PHI_FIG of the term).
Predictive quantiles: the property of tests/test_gpu_predictive.py -- F_ref(q) >= p - T and F_ref one fp64 step (4 ulp64) below q <= p + T --
and a brentq inversion of F_ref on a sample of rows: |q - q_brentq| <= 2 T / F_ref'(q) + 8 ulp64(q) + brentq's own 4 ulp64, the first term
the conditioning of the root (F is known to T only; the mixtures here have no flat stretch at the probabilities asked)."""
import math

import numpy as np
import pytest
import scipy.special as sp
from scipy.optimize import brentq

import hetero_ref as hr
import tbnn_oracle as o
from tensor_checks import layers_of
from test_gpu_predictive import LD, PHI_FIG, U, int_weights, mix

pytestmark = pytest.mark.gpu

LIK = o.LIK_HETERO_GAUSSIAN
M, N, DIMS = 24, 257, [1, 16, 16, 2]
PROBS = [0.05, 0.5, 0.95]


def T(m):
    return (m + 8) * U + 4 * PHI_FIG


_SETUP = {}


def setup(native):
    """(chain, X, Y, thetas, f): the generic kernel (a row per thread: a row's forward bits do not depend on its block), 24 networks
    around the oracle's initial state, their log-sd outputs spread over about [-2.5, 0.5]; computed once and left unchanged"""
    if "data" not in _SETUP:
        spec, X, Y, theta, _eta = hr.problem_of(DIMS, N, o.ACT_TANH, o.PRIOR_CAUCHY)
        rng = np.random.default_rng(7)
        thetas = (theta[None] + 0.3 * rng.standard_normal((M, spec.n_params))).astype(np.float32)
        thetas[:, hr.last_bias_index(spec, 1)] = rng.uniform(-2.5, 0.5, M).astype(np.float32)
        _SETUP["data"] = (spec, X, Y, thetas)
    spec, X, Y, thetas = _SETUP["data"]
    ch = native.Chain(layers_of(spec), likelihood=LIK, kernel=native.KERNEL_GENERIC)
    f = ch.forward_many(thetas, X=X)
    assert f.shape == (M, 2, N) and np.abs(f[:, 1]).max() < 8.0
    return ch, X, Y, thetas.copy(), f


def F_ref(y, f, w):
    """the mixture CDF at y [n] (or broadcastable) from the fp32 outputs f [m, 2, n], fp64 with the sum in extended precision"""
    f64 = f.astype(np.float64)
    s = np.exp(np.clip(f64[:, 1], -o.LOG_CLIP, o.LOG_CLIP))
    return mix(sp.ndtr((np.asarray(y, dtype=np.float64)[None] - f64[:, 0]) / s), w)


def test_loglik_loo_and_waic(native):
    from psis_ref import psis_ref
    from test_gpu_ensemble import logsumexp_rows
    from test_gpu_loo import TOL
    ch, X, Y, thetas, f = setup(native)
    f64 = f.astype(np.float64)
    l = np.stack([o.hetero_terms(f64[i], Y) for i in range(M)])                                   # [m, n]: one term per row
    gc = np.clip(f64[:, 1], -o.LOG_CLIP, o.LOG_CLIP)
    mag = o.HALF_LOG_2PI + np.abs(gc) + 0.5 * (Y.astype(np.float64)[None] - f64[:, 0]) ** 2 * np.exp(-2.0 * gc)
    got = ch.ensemble_loo(thetas, Y=Y, X=X, pointwise=True)
    again = ch.ensemble_loo(thetas, Y=Y.reshape(-1, 1), X=X, likelihood=LIK, pointwise=True)       # [n, 1] targets: the same bits
    for key in got:
        assert np.array_equal(got[key], again[key], equal_nan=True), key
    pw = got["pointwise"]
    e, tol = np.abs(pw - l), 16 * U * mag
    print(f"[hetero] ensemble: matrix against the fp64 definition, err max {e.max():.3e}, worst err/tol {np.max(e / tol):.3f}")
    assert pw.shape == (M, N) and np.all(np.isfinite(pw)) and np.all(e <= tol)
    ref = psis_ref(pw, 1.0)
    for key in ("elpd_loo", "pareto_k", "lppd", "p_waic"):
        g_, w_ = got[key], ref[key]
        assert np.array_equal(np.isposinf(g_), np.isposinf(w_)) and np.array_equal(np.isnan(g_), np.isnan(w_)), key
        fin = np.isfinite(w_)
        d = np.abs(g_[fin] - w_[fin]) / (np.abs(w_[fin]) if key in ("elpd_loo", "lppd") else 1.0)
        print(f"[hetero] ensemble: {key} diff {d.max(initial=0.0):.3e} (bound {TOL:.3e})")
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
    # a fixed-sd Gaussian handle of the same layers judges under the new likelihood too (the predictor's forward chain is one)
    gch = native.Chain(layers_of(_SETUP["data"][0]), likelihood=o.LIK_FIXED_GAUSSIAN, fixed_sd=1.0, kernel=native.KERNEL_GENERIC)
    other = gch.ensemble_loo(thetas, Y=Y, X=X, likelihood=LIK, pointwise=True)
    assert np.array_equal(other["pointwise"].view(np.uint64), pw.view(np.uint64))
    gch.close()
    ch.close()


def test_predictive_cdf_and_quantiles(native):
    ch, X, Y, thetas, f = setup(native)
    t = T(M)
    f64 = f.astype(np.float64)
    s = np.exp(np.clip(f64[:, 1], -o.LOG_CLIP, o.LOG_CLIP))
    real_w = (np.random.default_rng(3).random(M) + 0.05).astype(np.float32)
    real_w[5] = 0.0
    for tag, w in (("equal", None), ("importance weights", real_w), ("integer weights", int_weights(M))):
        q, F, Fb = ch.ensemble_predictive(thetas, probs=PROBS, Y=Y, X=X, weights=w)
        assert q.shape == (3, 1, N) and F.shape == (1, N) and Fb is None and q.dtype == F.dtype == np.float64
        err = np.abs(F[0] - F_ref(Y, f, w))
        print(f"[hetero] predictive {tag}: CDF err max {err.max():.3e} (T {t:.3e})")
        assert np.all(err <= t), (tag, float(err.max()))
        worst = 0.0
        for j, p in enumerate(PROBS):
            qj = q[j, 0]
            at, below = F_ref(qj, f, w), F_ref(qj - 4 * np.spacing(np.abs(qj)), f, w)
            worst = max(worst, float((p - at).max()), float((below - p).max()))
            assert np.all(np.isfinite(qj)) and np.all(at >= p - t) and np.all(below <= p + t), (tag, p)
        print(f"[hetero] predictive {tag}: quantiles, worst excess over p {worst:.3e} (T {t:.3e})")
        assert np.all(np.diff(q[:, 0], axis=0) >= 0)
        # brentq on a sample of the rows
        ww = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
        ww = ww / ww.sum()
        for row in range(0, N, 8):
            fr, sr = f64[:, 0, row], s[:, row]
            cdf = lambda x: float(np.sum(ww * sp.ndtr((x - fr) / sr)))
            for j, p in enumerate(PROBS):
                lo, hi = float((fr - 12.0 * sr).min()), float((fr + 12.0 * sr).max())
                qb = brentq(lambda x: cdf(x) - p, lo, hi, xtol=1e-300, rtol=4 * np.finfo(float).eps, maxiter=500)
                slope = float(np.sum(ww * np.exp(-0.5 * ((qb - fr) / sr) ** 2) / (sr * math.sqrt(2.0 * math.pi))))
                tol = 2 * t / slope + 8 * np.spacing(abs(q[j, 0, row])) + 4 * np.spacing(abs(qb))
                assert abs(q[j, 0, row] - qb) <= tol, (tag, row, p, q[j, 0, row], qb, tol)
    again = ch.ensemble_predictive(thetas, probs=PROBS, Y=Y, X=X, weights=w)
    assert np.array_equal(again[0].view(np.uint64), q.view(np.uint64)) and np.array_equal(again[1].view(np.uint64), F.view(np.uint64))
    # the staged rows and targets (padded to two columns by set_data) give the bits of the explicit ones
    ch.set_data(X, Y)
    staged = ch.ensemble_predictive(thetas, probs=PROBS, which=0, cdf=True, weights=w)
    assert np.array_equal(staged[0].view(np.uint64), q.view(np.uint64)) and np.array_equal(staged[1].view(np.uint64), F.view(np.uint64))
    ch.close()


def test_nan_networks(native):
    """a network of weight 0 that holds a NaN is ignored; a NaN in a network that counts gives NaN rows"""
    ch, X, Y, thetas, f = setup(native)
    w = int_weights(M)
    assert w[0] == 0 and w[-1] > 0
    clean = ch.ensemble_predictive(thetas, probs=PROBS, Y=Y, X=X, weights=w)
    th = thetas.copy()
    th[0, 3] = np.nan                                                    # network 0: weight 0
    assert np.isnan(ch.forward_many(th, X=X)[0]).all()
    q, F, _b = ch.ensemble_predictive(th, probs=PROBS, Y=Y, X=X, weights=w)
    assert np.array_equal(q.view(np.uint64), clean[0].view(np.uint64)) and np.array_equal(F.view(np.uint64), clean[1].view(np.uint64))
    th = thetas.copy()
    th[M - 1, hr.last_bias_index(_SETUP["data"][0], 1)] = np.nan          # the log-sd output alone of a network that counts
    fm = ch.forward_many(th, X=X)
    assert np.isnan(fm[M - 1, 1]).all() and np.isfinite(fm[M - 1, 0]).all()
    q, F, _b = ch.ensemble_predictive(th, probs=PROBS, Y=Y, X=X, weights=w)
    assert np.isnan(q).all() and np.isnan(F).all()
    # a NaN input row: that row alone
    Xn = X.copy()
    Xn[7, 0] = np.nan
    q, F, _b = ch.ensemble_predictive(thetas, probs=PROBS, Y=Y, X=Xn, weights=w)
    bad = np.zeros(N, bool)
    bad[7] = True
    for a in (q[0, 0], q[1, 0], q[2, 0], F[0]):
        assert np.array_equal(np.isnan(a), bad)
    ch.close()


def test_row_blocks(native, monkeypatch):
    """257 rows in blocks of 64: five blocks, the last of one row; bit for bit the single-block results"""
    ch, X, Y, thetas, f = setup(native)
    w = int_weights(M)
    whole = ch.ensemble_predictive(thetas, probs=PROBS, Y=Y, X=X, weights=w)
    whole_loo = ch.ensemble_loo(thetas, Y=Y, X=X, pointwise=True)
    budget = M * 2 * 64 + 7
    assert max(64, budget // (M * 2) // 64 * 64) == 64
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    cut = ch.ensemble_predictive(thetas, probs=PROBS, Y=Y, X=X, weights=w)
    cut_loo = ch.ensemble_loo(thetas, Y=Y, X=X, pointwise=True)
    monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
    for a, b in zip(whole[:2], cut[:2]):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(whole_loo["pointwise"].view(np.uint64), cut_loo["pointwise"].view(np.uint64))
    ch.close()


def test_refusals(native):
    ch, X, Y, thetas, f = setup(native)
    F = np.empty((1, N))
    q = np.empty((3, 1, N))
    pr = np.asarray(PROBS, dtype=np.float64)
    Y2, Xc, Fb = native.pad_targets(Y, N, 2, LIK), np.ascontiguousarray(X, dtype=np.float32), np.empty((1, N))
    rc = native.lib.tbnn_ensemble_predictive(ch._h, native._p(thetas), M, thetas.shape[1], LIK, None, None, 1, native._p(Xc), native._p(Y2), N,
                                             native._pd(pr), 3, native._pd(q), native._pd(F), native._pd(Fb))
    assert rc == -1 and "cdf_below_out" in native.lib.tbnn_last_error().decode()
    ch.close()
    spec = _SETUP["data"][0]
    layers = layers_of(spec)
    one = native.Chain(layers[:-1] + [(layers[-1][0], 1) + layers[-1][2:]], likelihood=o.LIK_FIXED_GAUSSIAN, fixed_sd=1.0, kernel=native.KERNEL_GENERIC)
    th1 = np.zeros((2, one.P), np.float32)
    for call in (lambda: one.ensemble_predictive(th1, probs=PROBS, X=X, likelihood=LIK),
                 lambda: one.ensemble_loglik(th1, Y=Y.reshape(-1, 1), X=X, likelihood=LIK),
                 lambda: one.ensemble_loo(th1, Y=Y.reshape(-1, 1), X=X, likelihood=LIK)):
        with pytest.raises(native.TbnnError, match="needs exactly 2 outputs"):
            call()
    one.close()


def test_predictor_noise_variance_and_intervals(tmp_path, monkeypatch, native):
    """the predictor over saved networks: predictMoments(noiseVariance=True) = (E[f], Var[f] + E[s^2]) against the fp64 formula,
    predict / plain predictMoments keep both outputs, predictiveInterval / predictiveCDF return one distribution per row, and the flag is
    refused under another likelihood or with a transform"""
    from tensorbnn_amd.likelihood import FixedGaussianLikelihood, HeteroscedasticGaussianLikelihood
    from tensorbnn_amd.predictor import predictor
    from test_gpu_hetero import hetero_data, make_net
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "0")
    X, Y = hetero_data(200, 1)
    Xv, Yv = hetero_data(100, 2)
    net = make_net(X, Y, Xv, Yv)
    net.train(30, 2, HeteroscedasticGaussianLikelihood(), folderName="h", networksPerFile=1, verbose=False)          # (10 burn-in epochs)
    p = predictor(str(tmp_path / "h") + "/", likelihood=HeteroscedasticGaussianLikelihood())
    f = np.asarray(p.predict(Xv), dtype=np.float64)                                         # [networks, 2, rows]
    assert f.shape[1:] == (2, 100)
    m, v = p.predictMoments(Xv)
    assert m.shape == v.shape == (2, 100)
    mean, tot = p.predictMoments(Xv, noiseVariance=True)
    assert mean.shape == tot.shape == (1, 100)
    s2 = np.exp(2.0 * np.clip(f[:, 1], -o.LOG_CLIP, o.LOG_CLIP))
    want = f[:, 0].var(axis=0) + s2.mean(axis=0)
    assert np.allclose(mean[0], f[:, 0].mean(axis=0), rtol=1e-12, atol=1e-12)
    # (the device forms exp(g) from the fp32 output in fp32: 1e-6 of the value)
    assert np.allclose(tot[0], want, rtol=2e-6), float(np.max(np.abs(tot[0] - want) / want))
    lower, median, upper = p.predictiveInterval(Xv, level=0.9)
    pit = p.predictiveCDF(Xv, Yv)
    assert lower.shape == median.shape == upper.shape == pit.shape == (1, 100)
    assert np.all(lower < median) and np.all(median < upper) and np.all((pit >= 0) & (pit <= 1))
    per_net, rows = p.logPredictiveDensity(Xv, Yv)
    assert per_net.shape == (f.shape[0],) and rows.shape == (100,) and np.all(np.isfinite(rows))
    p.trainProbs(X, Y, 1, HeteroscedasticGaussianLikelihood())
    assert len(p.weightsTrain) == f.shape[0] and np.all(np.isfinite(p.weightsTrain))
    for kw in ({"transform": "exp"}, {"sd": 2.0}, {"mean": 1.0}):
        with pytest.raises(ValueError):
            p.predictMoments(Xv, noiseVariance=True, **kw)
    p.likelihood = FixedGaussianLikelihood(sd=0.1)
    with pytest.raises(ValueError):
        p.predictMoments(Xv, noiseVariance=True)
