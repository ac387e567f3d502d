"""GPU: posterior-predictive quantiles over an ensemble's network axis (tbnn_ensemble_quantiles, Chain.ensemble_quantiles,
predictor.predictQuantiles / predictInterval) against np.quantile applied to the fp32 predictions Chain.forward_many returns for the same
thetas and rows.  The forward kernels are shared, so both sides rank the same bits and the test isolates the selection.  Every test here
fails without the entry point (it does not exist before this module's feature).

Bounds (U = 2^-53, ulp32(x) = the spacing of fp32 at x):

  inverted CDF.  The result is one of the m fp32 values, converted exactly; the weights are small integers and the probabilities dyadic,
  so p W and every partial sum of weights are exact in fp64 in any order: np.array_equal.

  linear.  a = t_(lo), b = t_(lo+1) are fp32 values, exact in fp64; g = (m - 1) p - lo is the same number on both sides (one fp64
  product, a floor and an exact subtraction: np.quantile's "linear" forms (n - 1) * q too).  Write M = max(|a|, |b|), D = |b - a| <= 2 M;
  the result lies between a and b, so its magnitude is at most M; every operation has a relative error of at most U.
    device, a + g (b - a):                  the difference and the product each err by U g D, the sum by U M:      (4 g + 1) U M
    NumPy's lerp, g < 1/2, the same form:                                                                         (4 g + 1) U M
    NumPy's lerp, g >= 1/2, b - (b - a)(1 - g): 1 - g, the difference and the product err by U (1 - g) D each,
                                            the final subtraction by U M:                                         (6 (1 - g) + 1) U M
  Three roundings on each side (NumPy's second form has a fourth).  The two sides together: (8 g + 2) U M < 6 U M for g < 1/2 and
  (8 - 2 g) U M <= 7 U M otherwise; the terms of second order in U fit into what is left to 8 U max(|a|, |b|), the bound the test
  asserts.  p = 0, p = 1 and m = 1 have g = 0: the device returns a as it is and NumPy a + 0 (b - a): equal.

  transforms.  The device ranks t_i = xform(f_i) * scale + shift formed in fp32, the oracle the same expression in fp64 from the same fp32
  f_i.  An order statistic is 1-Lipschitz in the sup norm of its arguments, and so is a convex combination of two, so the result moves by
  at most max_i |t_i(device) - t_i(fp64)|: XFORM_ULP ulp32 of the transformed value (the figures of tests/test_gpu_ensemble.py and DESIGN
  section 4.6 for these same device expressions) times |scale|, plus one ulp32 of t for the fused scale-and-shift, plus the linear bound.
"""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_ensemble import CASES, XFORM_ULP, make_chain, problem, transform64, ulp32

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
P_CDF = [0.0, 1 / 64, 0.25, 0.5, 61 / 64, 1.0]
P_LIN = [0.0, 0.05, 0.5, 0.95, 1.0]
ROWS = {"narrow": 1237, "mid2": 333, "layered10": 209, "generic4": 517}      # never a multiple of 16; d_out rows > one workgroup
SMALL_M = [1, 2, 3, 64, 65]


def setup(native, name, m, seed=0, tie=True):
    X, thetas = problem(name, m, seed=seed, n=ROWS[name])
    if tie and m > 2:
        thetas[2] = thetas[0]                              # ties in every element
    return make_chain(native, name), X, thetas


def int_weights(m, seed=1):
    """0 .. 3, with zeros and at least one positive"""
    w = np.random.default_rng(seed).integers(0, 4, m).astype(np.float32)
    w[0] = 0.0 if m > 1 else 2.0
    w[-1] = 2.0
    return w


def lin_bound(t64, probs):
    """8 U max(|t_(lo)|, |t_(lo+1)|) per probability and element; t64 [m, ...]"""
    s = np.sort(t64, axis=0)
    m = s.shape[0]
    out = []
    for p in probs:
        lo = int(math.floor((m - 1) * p))
        out.append(8 * U * np.maximum(np.abs(s[lo]), np.abs(s[min(lo + 1, m - 1)])))
    return np.stack(out)


def check_linear(tag, got, t64, probs, extra=None):
    """extra: what a transform evaluated in fp32 adds to the bound (None: the device ranks the very values of t64; g = 0 is then exact)"""
    ref = np.quantile(t64, probs, axis=0)
    tol = lin_bound(t64, probs) + (0.0 if extra is None else extra)
    err = np.abs(got - ref)
    print(f"[quantiles] {tag}: m={t64.shape[0]} linear err max {err.max():.3e}, worst err/tol {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.all(err <= tol), (tag, float(np.max(err / np.maximum(tol, 1e-300))))
    m = t64.shape[0]
    for j, p in enumerate(probs):
        if extra is None and (m == 1 or p in (0.0, 1.0)):
            assert np.array_equal(got[j], ref[j]), (tag, p)


# ------------------------------------------------------------------------------------------------------------ both methods, every shape
@pytest.mark.parametrize("name,m", [(n_, m_) for n_ in ROWS for m_ in SMALL_M] + [("generic4", 257), ("narrow", 257)])
def test_quantiles_against_numpy(native, name, m):
    """m = 1 (one value), 2 (no interior), 3, the wavefront size and one more, 257; d_out 1, 2, 4 and 10 over the cases; network 2 is a copy
    of network 0.  Inverted CDF unweighted and with integer weights (zeros among them) bit for bit; linear within the docstring's bound."""
    ch, X, thetas = setup(native, name, m)
    d_out = CASES[name][0][-1]
    f = ch.forward_many(thetas, X=X)
    t64 = f.astype(np.float64)
    if m > 2:
        assert np.array_equal(f[0], f[2])
    got = ch.ensemble_quantiles(thetas, P_CDF, X=X, method="inverted_cdf")
    assert got.shape == (len(P_CDF), d_out, X.shape[0]) and got.dtype == np.float64
    assert np.array_equal(got, np.quantile(t64, P_CDF, axis=0, method="inverted_cdf"))
    w = int_weights(m)
    got = ch.ensemble_quantiles(thetas, P_CDF, X=X, method="inverted_cdf", weights=w)
    assert np.array_equal(got, np.quantile(t64, P_CDF, axis=0, method="inverted_cdf", weights=w.astype(np.float64)))
    check_linear(f"{name}", ch.ensemble_quantiles(thetas, P_LIN, X=X), t64, P_LIN)
    ch.close()


def test_more_probabilities_than_one_register_group(native):
    """19 probabilities run as groups of 8, 8 and 3; every k / (m - 1) hits an order statistic itself"""
    m = 19
    ch, X, thetas = setup(native, "generic4", m, seed=3)
    t64 = ch.forward_many(thetas, X=X).astype(np.float64)
    probs = [k / (m - 1) for k in range(m)]
    check_linear("19 probabilities", ch.ensemble_quantiles(thetas, probs, X=X), t64, probs)
    got = ch.ensemble_quantiles(thetas, [k / 16 for k in range(17)], X=X, method="inverted_cdf")
    assert np.array_equal(got, np.quantile(t64, [k / 16 for k in range(17)], axis=0, method="inverted_cdf"))
    ch.close()


@pytest.mark.parametrize("m", [7, 100])
def test_inverted_cdf_at_probabilities_that_are_not_dyadic(native, m):
    """p m is then a rounded fp64 product (0.05 * 100 rounds to 5, 0.07 * 100 to 7.000000000000001): the device's count ceil(p m) must be
    NumPy's own index, floor(p m - 1) and one more where p m - 1 is no integer (the same product on both sides, the subtraction exact).
    Unweighted only: with weights the device compares partial sums with p W as its definition says, NumPy the sums divided by W with p,
    and the two agree for certain only where p W is exact (the dyadic probabilities of the other tests)."""
    probs = [0.05, 0.07, 0.1, 0.29, 0.3, 0.57, 0.7, 0.95, 0.99]
    ch, X, thetas = setup(native, "generic4", m, seed=9)
    t64 = ch.forward_many(thetas, X=X).astype(np.float64)
    got = ch.ensemble_quantiles(thetas, probs, X=X, method="inverted_cdf")
    assert np.array_equal(got, np.quantile(t64, probs, axis=0, method="inverted_cdf"))
    ch.close()


@pytest.mark.parametrize("n_probs", [1, 3, 4])
def test_up_to_four_probabilities(native, n_probs):
    """up to four probabilities (an interval's three) run the kernel that carries four bisection states, not eight: both methods, m = 65"""
    m = 65
    ch, X, thetas = setup(native, "generic4", m, seed=7)
    t64 = ch.forward_many(thetas, X=X).astype(np.float64)
    check_linear(f"{n_probs} probabilities", ch.ensemble_quantiles(thetas, [0.05, 0.5, 0.95, 1.0][:n_probs], X=X), t64, [0.05, 0.5, 0.95, 1.0][:n_probs])
    probs = [1 / 64, 0.5, 61 / 64, 0.0][:n_probs]
    w = int_weights(m)
    assert np.array_equal(ch.ensemble_quantiles(thetas, probs, X=X, method="inverted_cdf"), np.quantile(t64, probs, axis=0, method="inverted_cdf"))
    assert np.array_equal(ch.ensemble_quantiles(thetas, probs, X=X, method="inverted_cdf", weights=w),
                          np.quantile(t64, probs, axis=0, method="inverted_cdf", weights=w.astype(np.float64)))
    ch.close()


# --------------------------------------------------------------------------------------------------------------------------- transforms
@pytest.mark.parametrize("name,xform", [("narrow", "exp"), ("generic4", "sigmoid"), ("layered10", "softmax")])
def test_transforms_rank_the_transformed_values(native, name, xform):
    scale, shift = 1.7, -0.3
    code = {"exp": native.XFORM_EXP, "sigmoid": native.XFORM_SIGMOID, "softmax": native.XFORM_SOFTMAX}[xform]
    m = 9
    ch, X, thetas = setup(native, name, m, seed=6)
    f = ch.forward_many(thetas, X=X)
    for tag, sc, sh in (("plain", 1.0, 0.0), ("scaled", scale, shift), ("negative scale", -scale, shift)):
        x = transform64(f, xform)
        t64 = x * np.float64(np.float32(sc)) + np.float64(np.float32(sh))
        dt = XFORM_ULP[xform] * ulp32(x) * abs(sc)
        if sc != 1.0 or sh != 0.0:
            dt = dt + ulp32(t64)
        dt = dt.max(axis=0)                                  # the largest per-network error of the element
        check_linear(f"{name} {xform} {tag}", ch.ensemble_quantiles(thetas, P_LIN, X=X, xform=code, scale=sc, shift=sh), t64, P_LIN, extra=dt)
        # inverted CDF: one of the device's fp32 values, within dt of the fp64 order statistic
        w = int_weights(m)
        got = ch.ensemble_quantiles(thetas, P_CDF, X=X, xform=code, scale=sc, shift=sh, method="inverted_cdf", weights=w)
        ref = np.quantile(t64, P_CDF, axis=0, method="inverted_cdf", weights=w.astype(np.float64))
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))
        assert np.all(np.abs(got - ref) <= dt), (tag, float(np.max(np.abs(got - ref) / dt)))
    ch.close()


# --------------------------------------------------------------------------------------------------------------------------- row blocks
def test_row_blocks(native, monkeypatch):
    """517 rows in blocks of 128: five blocks, the last of 5 rows.  The driver's rule: rb = floor(budget / (m d_out)) rounded down to a
    multiple of 64, never below 64, whatever the number of probabilities (a block's results are held outside the budget).  The oracle runs
    forward_many on the same five row slices (whether a row's forward bits depend on its position in a launch is not assumed).  The staged
    rows give the bits of the explicit X."""
    name, m, rb = "generic4", 8, 128
    ch, X, thetas = setup(native, name, m, seed=2)
    d_out = CASES[name][0][-1]
    n = X.shape[0]
    assert n == 517 and n % rb == 5
    whole = ch.ensemble_quantiles(thetas, P_LIN, X=X)
    budget = m * d_out * rb + 7
    assert max(64, budget // (m * d_out) // 64 * 64) == rb                       # the driver's rule gives 128 rows ...
    slices = [(r0, min(rb, n - r0)) for r0 in range(0, n, rb)]
    assert len(slices) == 5 and slices[-1] == (512, 5)                           # ... five blocks, the last of 5 rows
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    t64 = np.concatenate([ch.forward_many(thetas, X=X[r0:r0 + r]) for r0, r in slices], axis=2).astype(np.float64)
    assert t64.shape == (m, d_out, n)
    got = ch.ensemble_quantiles(thetas, P_LIN, X=X)
    check_linear("row blocks", got, t64, P_LIN)
    w = int_weights(m)
    cdf = ch.ensemble_quantiles(thetas, P_CDF, X=X, method="inverted_cdf", weights=w)
    assert np.array_equal(cdf, np.quantile(t64, P_CDF, axis=0, method="inverted_cdf", weights=w.astype(np.float64)))
    x = transform64(t64, "softmax")                          # the transform kernel over blocks, the last of 5 rows
    ts = x * np.float64(np.float32(1.7)) + np.float64(np.float32(-0.3))
    check_linear("row blocks, softmax", ch.ensemble_quantiles(thetas, P_LIN, X=X, xform=native.XFORM_SOFTMAX, scale=1.7, shift=-0.3), ts, P_LIN,
                 extra=(XFORM_ULP["softmax"] * ulp32(x) * 1.7 + ulp32(ts)).max(axis=0))
    ch.set_data(X, np.zeros((n, d_out), dtype=np.float32))
    assert np.array_equal(ch.ensemble_quantiles(thetas, P_LIN, which=0), got)
    assert np.array_equal(ch.ensemble_quantiles(thetas, P_CDF, which=0, method="inverted_cdf", weights=w), cdf)
    monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
    assert np.array_equal(ch.ensemble_quantiles(thetas, P_LIN, which=0), whole)
    ch.close()


# ---------------------------------------------------------------------------------------------------------------- NaN, determinism
def test_nan_stays_visible(native):
    m = 5
    ch, X, thetas = setup(native, "generic4", m, seed=4)
    dims = CASES["generic4"][0]
    off = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 2))
    thetas[3, off + dims[-2] * dims[-1] + 1] = np.nan        # the bias of output 1 of network 3 (the tensors' order does not matter:
    f = ch.forward_many(thetas, X=X)                         # the test reads where the NaN went from forward_many)
    bad = np.isnan(f[3])
    assert bad.any() and not bad.all() and not np.isnan(np.delete(f, 3, axis=0)).any()
    for kw in ({"method": "linear"}, {"method": "inverted_cdf"}, {"method": "inverted_cdf", "weights": int_weights(m)}):
        got = ch.ensemble_quantiles(thetas, P_CDF, X=X, **kw)
        assert np.array_equal(np.isnan(got), np.broadcast_to(bad, got.shape)), kw
    ch.close()


def test_infinities_rank_as_numbers(native):
    m = 6
    ch, X, thetas = setup(native, "generic4", m, seed=8)
    P = thetas.shape[1]
    thetas[1, P - 1] = np.inf                                # the last parameter feeds an output, whichever the tensors' order
    thetas[4, P - 1] = -np.inf
    f = ch.forward_many(thetas, X=X)
    assert np.isinf(f[1]).any() and np.isinf(f[4]).any() and not np.isnan(f).any()
    t64 = f.astype(np.float64)
    got = ch.ensemble_quantiles(thetas, P_CDF, X=X, method="inverted_cdf")
    assert np.array_equal(got, np.quantile(t64, P_CDF, axis=0, method="inverted_cdf"))
    assert np.isinf(got[0]).any() and np.isinf(got[-1]).any() and np.all(np.isfinite(got[2:4]))
    ch.close()


def test_two_calls_return_the_same_bits(native):
    ch, X, thetas = setup(native, "narrow", 65, seed=5)
    w = int_weights(65)
    for kw in ({}, {"method": "inverted_cdf", "weights": w}, {"xform": native.XFORM_EXP, "scale": 1.7, "shift": -0.3}):
        a = ch.ensemble_quantiles(thetas, P_LIN, X=X, **kw)
        b = ch.ensemble_quantiles(thetas, P_LIN, X=X, **kw)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), kw
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_usable(native):
    dp = C.POINTER(C.c_double)
    ch, X, thetas = setup(native, "narrow", 4)
    n, Pn = X.shape[0], thetas.shape[1]
    lib, p = native.lib, native._p
    before = ch.ensemble_quantiles(thetas, P_LIN, X=X)
    out = np.full((65, 1, n), 7.0)

    def call(probs=(0.5,), n_probs=None, w=None, method=0, xform=0, probs_null=False, out_null=False, stride=Pn):
        pr = np.asarray(probs, dtype=np.float64)
        return lib.tbnn_ensemble_quantiles(ch._h, p(thetas), 4, stride, p(w), method, xform, 1.0, 0.0, 1, p(X), n,
                                           None if probs_null else pr.ctypes.data_as(dp), len(pr) if n_probs is None else n_probs,
                                           None if out_null else out.ctypes.data_as(dp))

    f32 = lambda *v: np.array(v, dtype=np.float32)
    err = lambda: lib.tbnn_last_error().decode()
    assert call(probs=(0.5, 1.5)) < 0 and "not in [0, 1]" in err()
    assert call(probs=(np.nan,)) < 0 and "not in [0, 1]" in err()
    assert call(probs=(-0.25,)) < 0 and "not in [0, 1]" in err()
    assert call(n_probs=0) < 0 and "n_probs" in err()
    assert call(probs=[0.5] * 65) < 0 and "n_probs" in err()
    assert call(probs_null=True) < 0 and "null" in err()
    assert call(out_null=True) < 0 and "null" in err()
    assert call(w=f32(1, 1, 1, 1), method=native.QUANT_LINEAR) < 0 and "takes no weights" in err()
    assert call(w=f32(1, -1, 1, 1), method=native.QUANT_INVERTED_CDF) < 0 and "negative" in err()
    assert call(w=f32(0, 0, 0, 0), method=native.QUANT_INVERTED_CDF) < 0 and "all weights are zero" in err()
    assert call(w=f32(1, np.nan, 1, 1), method=native.QUANT_INVERTED_CDF) < 0 and "not finite" in err()
    assert call(method=2) < 0 and "unknown method" in err()
    assert call(xform=4) < 0 and "unknown transform" in err()
    assert call(xform=native.XFORM_SOFTMAX) < 0 and "at least 2 outputs" in err()
    assert call(stride=Pn - 1) < 0 and "theta_stride < P" in err()
    assert np.all(out == 7.0)                                # nothing written
    with pytest.raises(native.TbnnError, match="takes no weights"):
        ch.ensemble_quantiles(thetas, [0.5], X=X, weights=[1, 1, 1, 1])
    with pytest.raises(native.TbnnError, match="n_probs"):
        ch.ensemble_quantiles(thetas, [], X=X)
    with pytest.raises(ValueError, match="method"):
        ch.ensemble_quantiles(thetas, [0.5], X=X, method="nearest")
    assert call(probs=[k / 63 for k in range(64)]) == 0      # 64 probabilities are accepted
    assert np.array_equal(ch.ensemble_quantiles(thetas, P_LIN, X=X), before)
    ch.close()


# ---------------------------------------------------------------------------------------------------------------- predictor, end to end
def test_predictor_round_trip(tmp_path, monkeypatch, native):
    """a predictor over saved networks, set up as tests/test_gpu_ensemble.py does: the interval's three arrays are ordered and are the
    quantiles at the three probabilities; the default transform under the categorical likelihood is the softmax"""
    from test_gpu_categorical import blobs, make_net
    from tensorbnn_amd.likelihood import CategoricalLikelihood
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    X, Y = blobs(600, 1)
    Xv, Yv = blobs(301, 2)
    net = make_net(X, Y, Xv, Yv)
    net.train(30, 2, CategoricalLikelihood(), folderName="blobs", networksPerFile=1, verbose=False)
    p = predictor(str(tmp_path / "blobs") + "/", likelihood=CategoricalLikelihood())
    assert p.numNetworks >= 4
    lower, median, upper = p.predictInterval(Xv, level=0.9)
    assert lower.shape == median.shape == upper.shape == (3, 301)
    assert np.all(lower <= median) and np.all(median <= upper)
    assert np.all(lower >= 0) and np.all(upper <= 1 + 3 * 2.0 ** -23)
    q = p.predictQuantiles(Xv, [0.05, 0.5, 0.95])
    assert np.array_equal(q[0], lower) and np.array_equal(q[1], median) and np.array_equal(q[2], upper)
    assert np.array_equal(p.predictQuantiles(Xv, 0.5), median)
    logits = np.array(p.predict(Xv))                                                   # [m, 3, rows]
    x = transform64(logits, "softmax")
    check_linear("predictor softmax", q, x, [0.05, 0.5, 0.95], extra=(XFORM_ULP["softmax"] * ulp32(x)).max(axis=0))
    w = np.ones(p.numNetworks)
    lo_w, med_w, up_w = p.predictInterval(Xv, level=0.5, weights=w, transform="none", sd=2.0, mean=0.5)
    t = logits.astype(np.float64) * 2.0 + 0.5
    ref = np.quantile(t, [0.25, 0.5, 0.75], axis=0, method="inverted_cdf", weights=w)
    for got, r in zip((lo_w, med_w, up_w), ref):
        assert np.all(np.abs(got - r) <= ulp32(t).max(axis=0))
    with pytest.raises(ValueError, match="linear"):
        p.predictQuantiles(Xv, [0.5], weights=w, method="linear")
