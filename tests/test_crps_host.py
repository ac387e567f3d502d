"""The CRPS of the predictive mixture (tbnn_ensemble_crps, predictor.crps / compareCrps) without a GPU: tests/crps_ref.py, which the GPU
tests compare the device against, is itself checked here -- the closed form against quadrature of the defining integral, the fp64
restatement against the 40-digit one over the GPU module's own cases (predictions from the oracle's fp32 forward in place of the device's:
the same networks, rows, scales, weights and targets), and the properties of the score -- with the host-only parts of the Python API.

The yardstick.  test_fp64_restatement_against_40_digits prints the worst deviation of the plain fp64 NumPy restatement from the 40-digit
reference over those cases, in units of u = 2^-53 (error_ref + spread_ref).  NP_WORST records that figure; the band of
tests/test_gpu_crps.py is K = 8 x it rounded up to a power of two = 64 (its module docstring), and the test asserts that the figure it
finds still gives that K: at most K / 8."""
import math

import mpmath as mp
import numpy as np
import pytest

import crps_ref as cr
import forward_ref as fr

# the worst deviation of crps_np from ref40 over the cases below, in units of 2^-53 (error_ref + spread_ref), as this module's own print
# gave it (x86-64, NumPy's pairwise sums, SciPy's erf); K = 8 x 4.10 = 32.8, rounded up to a power of two
NP_WORST = 4.10
K = 64

_CACHE = {}


def host_case(kind, m, rows, noise, weighted):
    """the case's predictions from the oracle's fp32 forward, its targets, scales and weights, and both references; computed once"""
    key = (kind, m, rows, noise, weighted)
    if key not in _CACHE:
        spec, X, thetas = cr.case_problem(kind, m, rows)
        f = fr.reference(spec, thetas, X, dtype=np.float32).astype(np.float32)
        Y = cr.case_targets(f, kind, seed=m + rows)
        sd = cr.sds(m) if kind != cr.HETERO else None
        w = cr.weights_with_zeros(m) if weighted else None
        _CACHE[key] = (f, Y, sd, w) + cr.case_reference(f, Y, kind, noise, sd, w)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------- the closed form itself
@pytest.mark.parametrize("seed,m", [(1, 1), (2, 3), (3, 7)])
def test_closed_form_against_quadrature(seed, m):
    """integral of (F(x) - 1{x >= y})^2 dx for a weighted mixture of m Gaussians, by mpmath.quad split at the target and the components'
    centres, against the closed form at 40 digits: 25 digits"""
    rng = np.random.default_rng(seed)
    f = rng.normal(0.0, 1.5, (m, 1))
    s = 10.0 ** rng.uniform(-1.0, 0.5, m)
    w = rng.gamma(1.0, size=m) + 0.05
    y = np.array([0.3])
    crps, _err, _spr = cr.ref40(f, s, w, y)
    with mp.workdps(cr.DPS):
        om = [mp.mpf(float(x)) / mp.fsum(mp.mpf(float(v)) for v in w) for x in w]
        F = lambda x: mp.fsum(om[i] * mp.ncdf((x - mp.mpf(float(f[i, 0]))) / mp.mpf(float(s[i]))) for i in range(m))
        yy = mp.mpf(float(y[0]))
        cuts = sorted({float(yy)} | {float(v) for v in f[:, 0]})
        lo, hi = min(cuts) - 40 * float(s.max()), max(cuts) + 40 * float(s.max())
        below = [c for c in cuts if c <= float(yy)]
        above = [c for c in cuts if c >= float(yy)]
        integral = mp.quad(lambda x: F(x) ** 2, [lo] + below) + mp.quad(lambda x: (1 - F(x)) ** 2, above + [hi])
        assert abs(integral - crps[0]) <= mp.mpf(10) ** -25 * crps[0], (integral, crps[0])


# --------------------------------------------------------------------------------------------- the fp64 restatement: the yardstick
def test_fp64_restatement_against_40_digits():
    worst, where = 0.0, None
    for case in cr.shape_cases() + cr.kind_cases():
        _f, _Y, _sd, _w, r40, rnp = host_case(*case)
        dev = cr.deviation_u(rnp, r40)
        if dev.max() > worst:
            worst, where = float(dev.max()), case
        assert np.all(r40[0] >= 0)
    print(f"[crps] fp64 NumPy restatement against the 40-digit one: worst deviation {worst:.2f} u at (kind, m, rows, noise, weighted) = {where} "
          f"(recorded: {NP_WORST}); the GPU band is K = 8 x the recorded figure, rounded up to a power of two = {K}")
    assert worst <= K / 8


# ------------------------------------------------------------------------------------------------------------------------- properties
def small(m=6, n=9, seed=5):
    rng = np.random.default_rng(seed)
    f = rng.normal(0.0, 1.0, (m, n)).astype(np.float32).astype(np.float64)
    s = (10.0 ** rng.uniform(-1.5, 0.5, m)).astype(np.float32).astype(np.float64)
    w = rng.gamma(0.7, size=m).astype(np.float32).astype(np.float64) + 0.01
    y = rng.normal(0.0, 1.5, n).astype(np.float32).astype(np.float64)
    return f, s, w, y


def close(a, b, scale, k=64):
    return np.all(np.abs(a - b) <= k * cr.U * scale)


def test_nonnegative_and_one_network():
    f, s, w, y = small()
    for noise_s in (s, None):
        crps, err, spr = cr.crps_np(f, noise_s, w, y)
        assert np.all(crps >= 0) and np.all(err >= spr) and np.all(spr >= 0)
    # m = 1: s [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt pi]
    import scipy.special as sp
    f1, s1 = f[:1], s[:1]
    z = (y - f1[0]) / s1[0]
    want = s1[0] * (z * (2.0 * sp.ndtr(z) - 1.0) + 2.0 * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) - 1.0 / math.sqrt(math.pi))
    crps, err, spr = cr.crps_np(f1, s1, None, y)
    assert close(crps, want, err + spr) and close(spr, np.full_like(spr, s1[0] / math.sqrt(math.pi)), spr)
    r40 = cr.ref40(f1, s1, None, y)
    assert cr.deviation_u((want, err, spr), r40)[0].max() <= 16


def test_duplicates_zero_weights_shift_and_scale():
    f, s, w, y = small()
    base = cr.crps_np(f, s, w, y)
    unit = base[1] + base[2]
    # a network listed twice at half weight: nothing beyond rounding
    f2, s2, w2 = np.concatenate([f, f[2:3]]), np.concatenate([s, s[2:3]]), np.concatenate([w, w[2:3] / 2])
    w2[2] /= 2
    for a, b in zip(cr.crps_np(f2, s2, w2, y), base):
        assert close(a, b, unit)
    # a network of weight 0: nothing at all, whatever it holds
    f0, s0, w0 = np.concatenate([f, np.full((1, f.shape[1]), np.inf)]), np.concatenate([s, [3.0]]), np.concatenate([w, [0.0]])
    for a, b in zip(cr.crps_np(f0, s0, w0, y), base):
        assert np.array_equal(a, b)
    r40a, r40b = cr.ref40(f0[:, :2], s0, w0, y[:2]), cr.ref40(f[:, :2], s, w, y[:2])
    assert all(x[0] == z[0] and x[1] == z[1] for x, z in zip(r40a, r40b))
    # f and y shifted together (by a power of two, exactly): invariant up to the rounding of the shifted inputs' differences
    for a, b in zip(cr.crps_np(f + 4.0, s, w, y + 4.0), base):
        assert close(a, b, unit, k=256)
    # f, y and s scaled together (by a power of two: exact): the result scales, bit for bit
    for a, b in zip(cr.crps_np(8.0 * f, 8.0 * s, w, 8.0 * y), base):
        assert np.array_equal(a, 8.0 * b)


def test_no_noise_is_the_sorted_formula():
    for m, seed in ((1, 1), (2, 2), (9, 3), (40, 4)):
        f, _s, w, y = small(m=m, n=33, seed=seed)
        w[1::3] = 0.0
        if m == 1:
            w[:] = 1.0
        for wts in (None, w):
            a, b = cr.crps_np(f, None, wts, y), cr.crps_sorted(f, wts, y)
            unit = a[1] + a[2] + np.abs(f).max(axis=0)                # (the sorted form multiplies the raw values: it cancels where crps_np does not)
            for x, z in zip(a, b):
                assert close(x, z, unit, k=8 * m)
        r40 = cr.ref40(f[:, :3], None, w, y[:3])
        assert cr.deviation_u([x[:3] for x in cr.crps_np(f, None, w, y)], r40).max() <= K / 8


def test_the_limit_of_small_noise():
    """noise = 0 is the limit s -> 0 of the formula with noise"""
    f, _s, w, y = small()
    a = cr.crps_np(f, np.full(f.shape[0], 1e-12), w, y)
    b = cr.crps_np(f, None, w, y)
    for x, z in zip(a, b):
        assert np.allclose(x, z, rtol=0, atol=1e-11)


# ------------------------------------------------------------------------------------------------------------ the Python API, host only
def test_library_declares_and_binds_the_entry_point(native):
    import ctypes as C
    assert ("tbnn_ensemble_crps" in {name for name, _r, _a in native.SYMBOLS}) and hasattr(C.CDLL(native.LIB_PATH), "tbnn_ensemble_crps")
    dp = np.zeros(1).ctypes.data_as(C.POINTER(C.c_double))
    assert native.lib.tbnn_ensemble_crps(None, None, 1, 1, 0, None, None, 1, None, None, 0, 1, dp, dp, dp) < 0       # a null handle


def test_summary_fields_and_compare():
    from tensorbnn_amd.predictor import predictor
    rng = np.random.default_rng(9)
    a = rng.gamma(2.0, size=(2, 50))
    b = a + rng.normal(0.1, 0.05, a.shape)
    a[1, 7] = np.nan
    s = predictor._crps_summary(a)
    assert s["n_bad"] == 1 and s["mean_crps"].shape == s["se"].shape == (2,)
    assert s["mean_crps"][0] == a[0].mean() and s["se"][0] == np.sqrt(np.var(a[0], ddof=1) / 50)
    ok = np.delete(a[1], 7)
    assert s["mean_crps"][1] == ok.mean() and s["se"][1] == np.sqrt(np.var(ok, ddof=1) / 49)
    one = predictor._crps_summary(np.array([[1.5]]))
    assert one["mean_crps"][0] == 1.5 and np.isnan(one["se"][0]) and one["n_bad"] == 0
    c = predictor.compareCrps({"crps": a}, {"crps": b})
    d0 = a[0] - b[0]
    assert c["crps_diff"][0] == d0.mean() and c["se_diff"][0] == np.sqrt(np.var(d0, ddof=1) / 50) and c["crps_diff"][0] < 0
    d1 = np.delete(a[1] - b[1], 7)
    assert c["crps_diff"][1] == d1.mean() and c["se_diff"][1] == np.sqrt(np.var(d1, ddof=1) / 49)
    back = predictor.compareCrps({"crps": b}, {"crps": a})
    assert np.array_equal(back["crps_diff"], -c["crps_diff"]) and np.array_equal(back["se_diff"], c["se_diff"])
    with pytest.raises(ValueError, match="same rows"):
        predictor.compareCrps({"crps": a}, {"crps": b[:, :49]})
    with pytest.raises(ValueError, match="crps returns"):
        predictor.compareCrps({"elpd_loo_rows": a[0]}, {"crps": b})


def test_refused_likelihoods():
    from tensorbnn_amd.likelihood import (BernoulliLikelihood, CategoricalLikelihood, FixedGaussianLikelihood, NegativeBinomialLikelihood,
                                          PoissonLikelihood, StudentTLikelihood)
    from tensorbnn_amd.predictor import predictor
    p = predictor.__new__(predictor)
    p.likelihood = FixedGaussianLikelihood(sd=0.5)
    assert p._crps_likelihood(None) is p.likelihood
    for lik, word in ((BernoulliLikelihood(), "label"), (CategoricalLikelihood(), "label"), (PoissonLikelihood(), "count"),
                      (NegativeBinomialLikelihood(dispersion=2.0), "count"), (StudentTLikelihood(df=4.0, sd=0.5), "t distributions")):
        with pytest.raises(ValueError, match=word):
            p._crps_likelihood(lik)
