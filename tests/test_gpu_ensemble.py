"""GPU: the reductions over an ensemble's network axis (tbnn_ensemble_moments / tbnn_ensemble_loglik, Chain.ensemble_moments /
ensemble_loglik, predictor.predictMoments / logPredictiveDensity) against NumPy applied to the fp32 predictions Chain.forward_many returns
for the same thetas and rows.  The forward kernels are shared, so both paths see the same f_i bit for bit and the test isolates the
reduction.  Every test here fails without the entry points (they do not exist before this module's feature).

Bounds (U = 2^-53, u = 2^-24, ulp32(x) = the spacing of fp32 at x):

  moments, no transform.  The device keeps t_ref = f_0 and adds S1 = sum w_i d_i, S2 = sum w_i d_i^2, d_i = f_i - f_0, in fp64 in network
  order; d_i is exact or rounded once, each product once or twice, and a sequential sum of m terms carries at most (m - 1) U times the sum of
  their magnitudes (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4).  With sum w_i |d_i| / W <= max |d_i| that is
  m U max|d_i| for S1 / W, and for var = S2 / W - (S1 / W)^2 it is m U max d_i^2 for the first term and twice that for the square; the
  shift, the products and the final division and subtraction fit in the factor 4:
      |mean err| <= 4 m U max_i |f_i - f_0| + 1 fp64 ulp of the mean,   |var err| <= 4 m U max_i (f_i - f_0)^2 + 1 fp64 ulp of the variance.
  The reference is np.average(f, axis=0, weights=w) and the weighted population variance.  np.average adds the UNSHIFTED w_i f_i, so
  evaluated in fp64 its own rounding error is of the order m U max |f_i| -- larger than the bound wherever the networks agree to more
  digits than they differ.  It is therefore evaluated on np.longdouble copies of the same fp32 predictions where that type is wider than
  fp64 (x86: 64-bit significand, error 2^-11 of the bound's unit); the bound is unchanged.

  transforms.  expf, the sigmoid 1 / (1 + expf(-f)) and the softmax expf(f - max) / sum (the difference taken exactly) run in fp32 on the device, NumPy applies exp in
  fp64 to the same fp32 f.  No ULP statement for the HIP device functions is installed with the toolkit (its headers and documents
  were searched for one), so the bounds are 4 x the largest error observed on the first green run on an MI355X, in ulp32 of the fp64 value --
  XFORM_ULP below; both figures and the date are in DESIGN.md (section "Ensemble reductions").  A value below the fp32 normal range gets
  2^-126 of absolute slack (it may be flushed).  With m networks the transformed values' errors enter the mean at most once each, and the
  variance through 2 max|t_i - t_0| times that.

  log-likelihoods.  Gaussian kinds: fp64 on the device from the fp32 prediction -- eight roundings per term cover the subtraction, the
  division, the square, the host's log sigma and the sums: 8 U (|log sigma| + d^2 / 2 + log(2 pi) / 2).  Bernoulli and categorical terms
  go through logf / log1pf / expf in fp32: LOGLIK_ULP x u x (|y log p| + |(1 - y) log1p(-p)|), resp. x u x sum_k |y_k| (|f_k - max| + d_out)
  (the sum of d_out exponentials and its log err by about d_out u absolutely), measured and set like XFORM_ULP.  per_net adds the
  issue's n d_out U sum |terms| for the order of the sum; a row of the mixture adds (m + 8) U for the fp64 log-sum-exp of m terms (the
  exponentials, the sum, the log) and 4 U |result| for the final additions.
"""
import math

import numpy as np
import pytest

import forward_ref as fr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
u = 2.0 ** -24
LD = np.longdouble if np.finfo(np.longdouble).eps < 2.0 ** -60 else np.float64

# 4 x the largest error observed on the first green MI355X run ("Ensemble reductions"), in ulp32 of the fp64 value
XFORM_ULP = {"none": 0.0, "exp": 4 * 0.803, "sigmoid": 4 * 2.170, "softmax": 4 * 4.605}
# the same for the fp32 log-likelihood terms, in units of u x the magnitudes named in the module docstring
LOGLIK_ULP = {"bernoulli": 4 * 2.177, "categorical": 4 * 0.890}

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3
LIK_GAUSSIAN, LIK_FIXED_GAUSSIAN, LIK_BERNOULLI, LIK_CATEGORICAL = 0, 1, 2, 3

CASES = {
    # dims, hidden activation, last activation, the handle's likelihood, kernel-name prefix, rows (never a multiple of 16)
    "narrow": ([5, 50, 50, 50, 1], ACT_RELU, ACT_NONE, LIK_FIXED_GAUSSIAN, "fast3<", 1237),
    "tall": ([784, 20, 20, 1], ACT_RELU, ACT_SIGMOID, LIK_BERNOULLI, "tall<", 301),
    "mid2": ([7, 33, 18, 50, 2], ACT_RELU, ACT_NONE, LIK_GAUSSIAN, "mid<", 777),
    "wide": ([10, 200, 200, 200, 1], ACT_RELU, ACT_NONE, LIK_GAUSSIAN, "wide<", 515),
    "wide2": ([3, 20, 36, 2], ACT_TANH, ACT_NONE, LIK_GAUSSIAN, "wide<", 1001),
    "layered10": ([12, 40, 10], ACT_TANH, ACT_NONE, LIK_FIXED_GAUSSIAN, "layered<", 1203),       # no fused family takes 10 outputs here
    "generic4": ([5, 16, 16, 4], ACT_TANH, ACT_NONE, LIK_FIXED_GAUSSIAN, "generic", 517),
}


def layers_for(dims, act, last):
    return [(dims[i], dims[i + 1], act if i < len(dims) - 2 else last, 0) for i in range(len(dims) - 1)]


def make_chain(native, name):
    dims, act, last, lik, prefix, _n = CASES[name]
    kernel = native.KERNEL_GENERIC if prefix == "generic" else native.KERNEL_AUTO
    ch = native.Chain(layers_for(dims, act, last), likelihood=lik, fixed_sd=0.7, kernel=kernel)
    assert ch.kernel_name.startswith(prefix), ch.kernel_name
    return ch


def problem(name, m, seed=0, n=None):
    dims, _a, _l, _lik, _p, rows = CASES[name]
    n = rows if n is None else n
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, dims[0])) / math.sqrt(max(dims[0] / 16.0, 1.0))).astype(np.float32)
    P = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
    thetas = (rng.standard_normal((m, P)) * 0.35).astype(np.float32)
    return X, thetas


def net_weights(m, seed=1):
    w = np.random.default_rng(seed).gamma(0.7, size=m).astype(np.float32)
    if m > 2:
        w[1] = 0.0                                    # a network that drops out
    return w


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def transform64(f, name):
    """fp64 transform of the fp32 predictions f [m, d_out, n]"""
    f = np.asarray(f, dtype=np.float64)
    if name == "exp":
        return np.exp(f)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-f))
    if name == "softmax":
        e = np.exp(f - f.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    return f


def moments_ref(t, w):
    """np.average / weighted population variance of t [m, ...] over axis 0, in LD (module docstring); returned as fp64"""
    t = np.asarray(t, dtype=LD)
    w = np.ones(t.shape[0], dtype=LD) if w is None else np.asarray(w, dtype=LD)
    mean = np.average(t, axis=0, weights=w)
    var = np.average((t - mean) ** 2, axis=0, weights=w)
    return np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)


def check_moments(tag, got_mean, got_var, f, w, xform="none", scale=1.0, shift=0.0):
    """f: fp32 predictions [m, d_out, n].  Prints the figures, then asserts the module docstring's bounds."""
    m = f.shape[0]
    t = transform64(f, xform) * np.float64(np.float32(scale)) + np.float64(np.float32(shift))
    mean, var = moments_ref(t, w)
    span = np.abs(t - t[0]).max(axis=0)
    # error of one transformed value: the transform's ulps, and one rounding each for the product and the sum when scale / shift are set
    # (half an ulp32 each, taken as a whole one: the rounded value may lie in the next binade)
    k = XFORM_ULP[xform]
    x = transform64(f, xform)
    dt = k * ulp32(x) * abs(scale) + (2.0 ** -126 if k else 0.0)
    if scale != 1.0 or shift != 0.0:
        dt = dt + ulp32(x * scale) + ulp32(t)
    dt = dt.max(axis=0)
    tol_mean = 4 * m * U * span + np.spacing(np.abs(mean)) + dt
    tol_var = 4 * m * U * span ** 2 + np.spacing(var) + 2 * span * dt + dt ** 2
    em, ev = np.abs(got_mean - mean), np.abs(got_var - var)
    print(f"[ensemble] {tag}: m={m} mean err max {em.max():.3e} (worst err/tol {np.max(em / tol_mean):.3f}), "
          f"var err max {ev.max():.3e} (worst err/tol {np.max(ev / tol_var):.3f})")
    assert np.all(np.isfinite(got_mean)) and np.all(np.isfinite(got_var))
    assert np.all(em <= tol_mean), (tag, float(np.max(em / tol_mean)))
    assert np.all(ev <= tol_var), (tag, float(np.max(ev / tol_var)))
    assert np.all(got_var >= 0)


# ---------------------------------------------------------------------------------------------------------------- moments, no transform
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("m", [1, 2, 9])
def test_moments_every_family(native, name, m):
    """equal and unequal weights; staged rows of both kinds and explicit X; d_out 1, 2, 4 and 10 over the cases"""
    X, thetas = problem(name, m)
    ch = make_chain(native, name)
    d_out = CASES[name][0][-1]
    Y = np.zeros((X.shape[0], d_out), dtype=np.float32)
    nv = 203
    ch.set_data(X, Y)
    ch.set_validation(X[:nv], Y[:nv])
    f = ch.forward_many(thetas, X=X)
    assert f.shape == (m, d_out, X.shape[0])
    w = net_weights(m)
    for tag, kw, fs in (("explicit X", {"X": X}, f), ("training rows", {"which": 0}, f), ("validation rows", {"which": 1}, f[:, :, :nv])):
        assert np.array_equal(ch.forward_many(thetas, **kw), fs)
        for wt in (None, w):
            mean, var = ch.ensemble_moments(thetas, weights=wt, **kw)
            assert mean.shape == var.shape == (d_out, fs.shape[2]) and mean.dtype == var.dtype == np.float64
            check_moments(f"{name} {tag} {'weighted' if wt is not None else 'equal'}", mean, var, fs, wt)
            if m == 1:
                assert np.array_equal(mean, fs[0].astype(np.float64)) and not var.any()
    mean_only, none = ch.ensemble_moments(thetas, X=X, var=False)
    assert none is None and np.array_equal(mean_only, ch.ensemble_moments(thetas, X=X)[0])
    ch.close()


def test_moments_multi_chain_handle(native):
    """a tbnn_create_multi handle takes explicit thetas like a one-chain handle"""
    dims, act, last, lik, prefix, n = CASES["narrow"]
    X, thetas = problem("narrow", 5)
    grp = native.ChainGroup(layers_for(dims, act, last), 3, likelihood=lik)
    ch = make_chain(native, "narrow")
    want = ch.ensemble_moments(thetas, X=X, weights=net_weights(5))
    mean = np.empty((1, n)); var = np.empty((1, n))
    w = net_weights(5)
    import ctypes as C
    dp = C.POINTER(C.c_double)
    rc = native.lib.tbnn_ensemble_moments(grp._h, native._p(thetas), 5, thetas.shape[1], native._p(w), 0, 1.0, 0.0, 1, native._p(X), n,
                                          mean.ctypes.data_as(dp), var.ctypes.data_as(dp))
    assert rc == 0, native.lib.tbnn_last_error()
    assert np.array_equal(mean, want[0]) and np.array_equal(var, want[1])
    ch.close(); grp.close()


# ---------------------------------------------------------------------------------------------------------------------- chunk carry-over
def test_two_real_chunks(native):
    """Chunks hold 2^28 floats of predictions.  d_out = 10 and n = 1,000,003 rows make one network's predictions 10,000,030 floats, so a
    chunk holds 26 networks and m = 28 runs as 26 + 2: the accumulators and the shift t_ref cross a real chunk boundary, weighted, for the
    moments and for both directions of the log-likelihood (rows checked on a slice to bound the host's work)."""
    m, n = 28, 1_000_003
    X, thetas = problem("layered10", m, seed=3, n=n)
    ch = make_chain(native, "layered10")
    assert (1 << 28) // (10 * n) == 26 < m
    f = ch.forward_many(thetas, X=X)
    # f is cut at the same boundary as everything below: the last network of the first chunk and both of the second against the fp64
    # oracle (tests/forward_ref.py; this problem's fp32 oracle sits at 0.03 of that tolerance, tests/test_forward_ref_host.py)
    nets = [0, 25, 26, 27]
    rows = np.unique(np.concatenate([np.arange(0, n, 97), np.arange(64), np.arange(n - 64, n)]))
    fr.check(f[nets][:, :, rows], fr.reference(fr.spec_of(*CASES["layered10"][:3]), thetas[nets], X, rows), "two real chunks, networks 0, 25 | 26, 27")
    w = net_weights(m, seed=5)
    mean, var = ch.ensemble_moments(thetas, X=X, weights=w)
    for k in range(10):                                                  # one output at a time: the extended-precision copies stay small
        check_moments(f"two chunks, output {k}", mean[k:k + 1], var[k:k + 1], f[:, k:k + 1, :], w)
    Y = np.random.default_rng(9).standard_normal((n, 10)).astype(np.float32)
    sd = np.linspace(0.5, 2.0, m).astype(np.float32)
    per_net, rows = ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=LIK_GAUSSIAN, sd=sd, weights=w)
    want, err, mag = np.zeros(m), np.zeros(m), np.zeros(m)
    for r0 in range(0, n, 100_000):                                      # the fp64 terms of 100,000 rows at a time
        l, e, g = loglik_terms(f[:, :, r0:r0 + 100_000], Y[r0:r0 + 100_000], LIK_GAUSSIAN, sd)
        want += l.sum(axis=1); err += e.sum(axis=1); mag += g
    tol = err + n * 10 * U * mag + np.spacing(np.abs(want))
    print(f"[ensemble] two chunks: per_net worst err/tol {np.max(np.abs(per_net - want) / tol):.3f}")
    assert np.all(np.abs(per_net - want) <= tol)
    sl = slice(0, n, 97)
    check_loglik("two chunks (rows)", None, rows[sl], f[:, :, sl], Y[sl], LIK_GAUSSIAN, sd, w)
    ch.close()


@pytest.mark.parametrize("name", ["narrow", "tall", "layered10", "generic4"])
def test_chunk_override_carries_over(native, monkeypatch, name):
    """TBNN_ENS_CHUNK_FLOATS (read by the two reductions only) cuts 8 networks into chunks of 3, 3 and 2: the sums run in the same
    network order, so every result equals the one-chunk call bit for bit -- and forward_many does not change"""
    m = 8
    X, thetas = problem(name, m, seed=2)
    d_out = CASES[name][0][-1]
    ch = make_chain(native, name)
    rng = np.random.default_rng(4)
    Y = rng.random((X.shape[0], d_out)).astype(np.float32)
    w = net_weights(m)
    lik = LIK_CATEGORICAL if d_out > 1 else LIK_BERNOULLI if name == "tall" else LIK_GAUSSIAN
    xf = native.XFORM_SOFTMAX if d_out > 1 else native.XFORM_EXP
    one = (ch.forward_many(thetas, X=X), ch.ensemble_moments(thetas, X=X, weights=w, xform=xf), ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=lik, weights=w))
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(3 * d_out * X.shape[0] + 5))
    cut = (ch.forward_many(thetas, X=X), ch.ensemble_moments(thetas, X=X, weights=w, xform=xf), ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=lik, weights=w))
    assert np.array_equal(one[0], cut[0])
    for a, b in zip(one[1] + one[2], cut[1] + cut[2]):
        assert np.array_equal(a, b)
    check_moments(f"{name} chunks of 3", cut[1][0], cut[1][1], one[0], w, xform={native.XFORM_SOFTMAX: "softmax", native.XFORM_EXP: "exp"}[xf])
    check_loglik(f"{name} chunks of 3", cut[2][0], cut[2][1], one[0], Y, lik, None, w, fixed_sd=0.7)
    ch.close()


# --------------------------------------------------------------------------------------------------------------------------- transforms
def saturate(thetas, dims, f, peak=80.0):
    """the last layer of every network scaled so that its outputs reach +-peak"""
    th = thetas.copy()
    off = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 2))
    for i in range(th.shape[0]):
        th[i, off:] = (th[i, off:].astype(np.float64) * (peak / np.abs(f[i]).max())).astype(np.float32)
    return th


@pytest.mark.parametrize("name,xform", [("narrow", "exp"), ("narrow", "sigmoid"), ("wide2", "softmax"), ("wide2", "exp"), ("layered10", "softmax"),
                                        ("layered10", "sigmoid"), ("generic4", "softmax"), ("generic4", "exp")])
def test_transforms(native, name, xform):
    """one network: the mean IS the transformed value, so its error in ulp32 is the device function's (printed: the figure XFORM_ULP is
    4 x of); then 7 networks, weighted, with scale and shift; logits scaled to +-80 stay finite; softmax rows sum to 1"""
    code = {"exp": native.XFORM_EXP, "sigmoid": native.XFORM_SIGMOID, "softmax": native.XFORM_SOFTMAX}[xform]
    dims = CASES[name][0]
    d_out = dims[-1]
    X, thetas = problem(name, 7, seed=6)
    ch = make_chain(native, name)
    sat = saturate(thetas, dims, ch.forward_many(thetas, X=X))
    for tag, th in (("moderate", thetas), ("saturated", sat)):
        f = ch.forward_many(th, X=X)
        if tag == "saturated":
            assert 79.0 < np.abs(f).max() < 81.0
        worst = 0.0
        for i in range(th.shape[0]):
            mean, var = ch.ensemble_moments(th[i:i + 1], X=X, xform=code)
            assert np.all(np.isfinite(mean)) and not var.any()
            ref = transform64(f[i:i + 1], xform)[0]
            worst = max(worst, float(np.max(np.maximum(np.abs(mean - ref) - 2.0 ** -126, 0.0) / ulp32(ref))))
            if xform == "softmax":
                assert np.all(np.abs(mean.sum(axis=0) - 1.0) <= d_out * 2.0 ** -23)
        print(f"[ensemble] {name} {xform} {tag}: largest error of one transformed value {worst:.3f} ulp32 (bound {XFORM_ULP[xform]})")
        assert worst <= XFORM_ULP[xform]
        w = net_weights(th.shape[0])
        mean, var = ch.ensemble_moments(th, X=X, weights=w, xform=code)
        check_moments(f"{name} {xform} {tag}", mean, var, f, w, xform=xform)
        if xform == "softmax":
            assert np.all(np.abs(mean.sum(axis=0) - 1.0) <= d_out * 2.0 ** -23)
    mean, var = ch.ensemble_moments(thetas, X=X, weights=w, xform=code, scale=3.25, shift=-1.5)
    check_moments(f"{name} {xform} scaled", mean, var, ch.forward_many(thetas, X=X), w, xform=xform, scale=3.25, shift=-1.5)
    ch.close()


# ---------------------------------------------------------------------------------------------------------------------- log-likelihoods
def loglik_terms(f, Y, lik, sd, fixed_sd=0.7):
    """the package's per-element terms in fp64 from the fp32 predictions f [m, d_out, n] and targets Y [n, d_out]: (rows l [m, n] summed over the
    outputs, their error model [m, n], the sum of |terms| [m])"""
    m, d_out, n = f.shape
    f = f.astype(np.float64)
    y = np.asarray(Y, dtype=np.float32).reshape(n, d_out).T.astype(np.float64)[None]              # [1, d_out, n]
    if lik in (LIK_GAUSSIAN, LIK_FIXED_GAUSSIAN):
        s = np.full(m, fixed_sd, dtype=np.float32) if sd is None else np.asarray(sd, dtype=np.float32)
        sigma = np.clip(s, np.float32(1e-8), np.float32(1e8)).astype(np.float64)[:, None, None]       # layer.py:60-64
        d = (y - f) / sigma
        terms = -np.log(sigma) - 0.5 * d * d - 0.5 * math.log(2 * math.pi)
        err = 8 * U * (np.abs(np.log(sigma)) + 0.5 * d * d + 0.5 * math.log(2 * math.pi))
        return terms.sum(axis=1), err.sum(axis=1), np.abs(terms).sum(axis=(1, 2))
    if lik == LIK_BERNOULLI:
        p = np.clip(f.astype(np.float32), np.float32(1e-8), np.float32(1) - np.float32(1e-7)).astype(np.float64)   # likelihood.py:78-80
        t1 = np.where(y == 0, 0.0, y * np.log(p))
        t2 = np.where(1 - y == 0, 0.0, (1 - y) * np.log1p(-p))
        terms = t1 + t2
        err = LOGLIK_ULP["bernoulli"] * u * (np.abs(t1) + np.abs(t2))
        return terms.sum(axis=1), err.sum(axis=1), np.abs(terms).sum(axis=(1, 2))
    d = f - f.max(axis=1, keepdims=True)                                                             # likelihood.py:86-107
    ls = d - np.log(np.exp(d).sum(axis=1, keepdims=True))
    terms = y * ls
    err = LOGLIK_ULP["categorical"] * u * (np.abs(y) * (np.abs(d) + d_out))
    return terms.sum(axis=1), err.sum(axis=1), np.abs(terms).sum(axis=(1, 2))


def logsumexp_rows(a, w):
    """log sum_i w_i exp(a_i) over axis 0"""
    try:
        from scipy.special import logsumexp
        return logsumexp(a, axis=0, b=w[:, None])
    except ImportError:
        keep = w > 0
        a, lw = a[keep], np.log(w[keep])[:, None]
        mx = (a + lw).max(axis=0)
        return mx + np.log(np.exp(a + lw - mx).sum(axis=0))


def check_loglik(tag, per_net, rows, f, Y, lik, sd, w, fixed_sd=0.7, unit=None):
    m, d_out, n = f.shape
    l, err, mag = loglik_terms(f, Y, lik, sd, fixed_sd)
    if per_net is not None:
        want = l.sum(axis=1)
        tol = err.sum(axis=1) + n * d_out * U * mag + np.spacing(np.abs(want))
        e = np.abs(per_net - want)
        print(f"[ensemble] {tag}: per_net err max {e.max():.3e}, worst err/tol {np.max(e / tol):.3f}")
        assert np.all(np.isfinite(per_net)) and np.all(e <= tol), (tag, float(np.max(e / tol)))
    if rows is not None:
        ww = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
        want = logsumexp_rows(l, ww) - math.log(ww.sum())
        tol = err[ww > 0].max(axis=0) + (m + 8) * U + 4 * U * np.abs(want)
        e = np.abs(rows - want)
        print(f"[ensemble] {tag}: lppd err max {e.max():.3e}, worst err/tol {np.max(e / tol):.3f}")
        assert np.all(np.isfinite(rows)) and np.all(e <= tol), (tag, float(np.max(e / tol)))


def term_error_units(per_net_1row, f, Y, lik):
    """one network, one row: the device's error of that row's terms in units of u x the magnitudes of the module docstring"""
    l, err, _ = loglik_terms(f, Y, lik, None)
    k = LOGLIK_ULP["bernoulli" if lik == LIK_BERNOULLI else "categorical"]
    return abs(per_net_1row - l[0, 0]) / max(err[0, 0] / k, 1e-300)


@pytest.mark.parametrize("name,lik", [("narrow", LIK_GAUSSIAN), ("narrow", LIK_FIXED_GAUSSIAN), ("mid2", LIK_GAUSSIAN), ("tall", LIK_BERNOULLI),
                                      ("wide2", LIK_CATEGORICAL), ("wide2", LIK_BERNOULLI), ("layered10", LIK_CATEGORICAL),
                                      ("layered10", LIK_FIXED_GAUSSIAN), ("generic4", LIK_CATEGORICAL), ("generic4", LIK_BERNOULLI)])
def test_loglik(native, name, lik):
    """all four kinds against the package's terms in fp64; per-network sd, equal and unequal network weights; staged and explicit targets;
    a second call returns the same bits"""
    m = 9
    X, thetas = problem(name, m, seed=7)
    dims = CASES[name][0]
    d_out = dims[-1]
    n = X.shape[0]
    rng = np.random.default_rng(8)
    ch = make_chain(native, name)
    f = ch.forward_many(thetas, X=X)
    if lik == LIK_CATEGORICAL:
        z = rng.standard_normal((n, d_out)) * 2
        Y = (np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)).astype(np.float32)              # soft labels ...
        Y[::3] = np.eye(d_out, dtype=np.float32)[rng.integers(0, d_out, len(Y[::3]))]          # ... and one-hot rows
    elif lik == LIK_BERNOULLI:
        Y = (rng.random((n, d_out)) < 0.5).astype(np.float32)
        Y[::5] = rng.random((len(Y[::5]), d_out)).astype(np.float32)                           # fractional targets take both terms
    else:
        Y = (f[0].T + 0.5 * rng.standard_normal((n, d_out))).astype(np.float32)
    sd = None if lik in (LIK_BERNOULLI, LIK_CATEGORICAL) else (0.2 + rng.random(m)).astype(np.float32)
    if sd is not None:
        sd[0], sd[1] = 1e-12, 3e9                                                             # clipped to 1e-8 and 1e8
    w = net_weights(m)
    ch.set_data(X, Y)
    for wt in (None, w):
        per_net, rows = ch.ensemble_loglik(thetas, which=0, likelihood=lik, sd=sd, weights=wt)          # staged rows and targets
        again = ch.ensemble_loglik(thetas, which=0, likelihood=lik, sd=sd, weights=wt)
        assert np.array_equal(per_net, again[0]) and np.array_equal(rows, again[1])
        explicit = ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=lik, sd=sd, weights=wt)
        assert np.array_equal(per_net, explicit[0]) and np.array_equal(rows, explicit[1])
        check_loglik(f"{name} lik {lik} {'weighted' if wt is not None else 'equal'}", per_net, rows, f, Y, lik, sd, wt)
    if sd is None:
        worst = max(term_error_units(ch.ensemble_loglik(thetas[i:i + 1], Y=Y[r:r + 1], X=X[r:r + 1], likelihood=lik)[0][0],
                                     f[i:i + 1, :, r:r + 1], Y[r:r + 1], lik) for i in range(3) for r in range(0, n, max(n // 40, 1)))
        kind = "bernoulli" if lik == LIK_BERNOULLI else "categorical"
        print(f"[ensemble] {name} {kind}: largest error of one row's terms {worst:.3f} units (bound {LOGLIK_ULP[kind]})")
        assert worst <= LOGLIK_ULP[kind]
    if sd is None:
        per_default = ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=LIK_FIXED_GAUSSIAN)[0]            # sd NULL: the descriptor's fixed_sd
        check_loglik(f"{name} fixed_sd", per_default, None, f, Y, LIK_FIXED_GAUSSIAN, None, None, fixed_sd=0.7)
    ch.close()


def test_loglik_saturated_bernoulli(native):
    """sigmoid outputs driven to exactly 0 and 1: p is clipped to [1e-8, 1 - 1e-7], and a target of exactly 0 or 1 drops its other term"""
    name = "tall"
    m = 6
    X, thetas = problem(name, m, seed=11)
    dims = CASES[name][0]
    ch = make_chain(native, name)
    off = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 2))
    thetas[:4, off:] *= 4000.0
    f = ch.forward_many(thetas, X=X)
    assert np.any(f == 0.0) and np.any(f == 1.0)
    Y = (np.random.default_rng(12).random((X.shape[0], 1)) < 0.5).astype(np.float32)
    w = net_weights(m)
    per_net, rows = ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=LIK_BERNOULLI, weights=w)
    check_loglik("saturated bernoulli", per_net, rows, f, Y, LIK_BERNOULLI, None, w)
    assert per_net.min() < 10 * math.log(1e-8)                       # the clipped terms are there
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_as_it_was(native):
    import ctypes as C
    dp = C.POINTER(C.c_double)
    X, thetas = problem("narrow", 4)
    n, P = X.shape[0], thetas.shape[1]
    ch = make_chain(native, "narrow")
    Y = np.zeros((n, 1), dtype=np.float32)
    before = ch.forward_many(thetas, X=X)
    out = np.empty((1, n)); pn = np.empty(4)
    lib, p = native.lib, native._p

    def moments(w=None, xform=0, stride=P, X_=X, n_=n, which=1):
        return lib.tbnn_ensemble_moments(ch._h, p(thetas), 4, stride, p(w), xform, 1.0, 0.0, which, p(X_), n_, out.ctypes.data_as(dp), None)

    def loglik(w=None, stride=P, X_=X, Y_=Y, n_=n, which=1, lik=0):
        return lib.tbnn_ensemble_loglik(ch._h, p(thetas), 4, stride, lik, None, p(w), which, p(X_), p(Y_), n_, pn.ctypes.data_as(dp), None)

    f32 = lambda *v: np.array(v, dtype=np.float32)
    for call in (moments, loglik):
        for w, msg in ((f32(1, -1, 1, 1), "negative"), (f32(1, np.nan, 1, 1), "not finite"), (f32(1, np.inf, 1, 1), "not finite"),
                       (f32(0, 0, 0, 0), "all weights are zero")):
            assert call(w=w) < 0 and msg in lib.tbnn_last_error().decode(), (call.__name__, msg, lib.tbnn_last_error())
        assert call(stride=P - 1) < 0 and "theta_stride < P" in lib.tbnn_last_error().decode()
        assert call(X_=None, n_=0, which=1) < 0 and "tbnn_set_validation has not been called" in lib.tbnn_last_error().decode()
        assert call(X_=None, n_=0, which=0) < 0 and "tbnn_set_data has not been called" in lib.tbnn_last_error().decode()
        assert call(X_=None, n_=0, which=2) < 0 and "which must be" in lib.tbnn_last_error().decode()
    assert moments(xform=native.XFORM_SOFTMAX) < 0 and "at least 2 outputs" in lib.tbnn_last_error().decode()
    assert moments(xform=4) < 0 and "unknown transform" in lib.tbnn_last_error().decode()
    assert loglik(Y_=None) < 0 and "without their targets" in lib.tbnn_last_error().decode()
    assert loglik(lik=LIK_CATEGORICAL) < 0 and "at least 2 outputs" in lib.tbnn_last_error().decode()
    assert loglik(lik=7) < 0 and "unknown likelihood" in lib.tbnn_last_error().decode()
    with pytest.raises(native.TbnnError, match="negative"):
        ch.ensemble_moments(thetas, X=X, weights=[1, -1, 1, 1])
    with pytest.raises(ValueError):
        ch.ensemble_loglik(thetas, X=X)
    assert np.array_equal(ch.forward_many(thetas, X=X), before)
    assert moments() == 0 and loglik() == 0                          # and the accepted calls still work
    ch.close()


def test_forward_many_unchanged_by_the_reductions(native):
    for name in ("narrow", "layered10", "generic4"):
        X, thetas = problem(name, 5, seed=13)
        ch = make_chain(native, name)
        d_out = CASES[name][0][-1]
        Y = np.random.default_rng(1).random((X.shape[0], d_out)).astype(np.float32)
        before = ch.forward_many(thetas, X=X)
        ch.ensemble_moments(thetas, X=X, weights=net_weights(5), xform=native.XFORM_SIGMOID)
        assert np.array_equal(ch.forward_many(thetas, X=X), before)
        ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=LIK_BERNOULLI)
        assert np.array_equal(ch.forward_many(thetas, X=X), before)
        ch.close()


# ---------------------------------------------------------------------------------------------------------------- predictor, end to end
def test_predictor_end_to_end(tmp_path, monkeypatch, native):
    """a three-class network trained for a few epochs (the set-up of tests/test_gpu_categorical.py): predictMoments returns posterior-mean
    class probabilities -- the softmax-then-average of predict's logits, rows summing to 1 -- and takes reweight's weights; under a
    GaussianLikelihood (the saved networks judged as a regression on the one-hot targets, each with its saved last hyper as sd)
    logPredictiveDensity's per-network values are _data_logprob's"""
    from test_gpu_categorical import blobs, make_net
    from tensorbnn_amd.likelihood import CategoricalLikelihood, GaussianLikelihood
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    X, Y = blobs(600, 1)
    Xv, Yv = blobs(301, 2)
    net = make_net(X, Y, Xv, Yv)
    net.train(30, 2, CategoricalLikelihood(), folderName="blobs", networksPerFile=1, verbose=False)
    p = predictor(str(tmp_path / "blobs") + "/", likelihood=CategoricalLikelihood())
    assert p.numNetworks >= 4
    logits = np.array(p.predict(Xv))                                                   # [m, 3, rows]
    mean, var = p.predictMoments(Xv)
    assert mean.shape == var.shape == (3, 301)
    check_moments("predictor softmax", mean, var, logits, None, xform="softmax")
    assert np.all(np.abs(mean.sum(axis=0) - 1.0) <= 3 * 2.0 ** -23) and np.all(mean >= 0)
    weights = p.reweight(str(tmp_path / "blobs" / "architecture.txt"))
    assert len(weights) == p.numNetworks
    mean_w, var_w = p.predictMoments(Xv, weights=weights)
    check_moments("predictor softmax, reweighted", mean_w, var_w, logits, np.asarray(weights, dtype=np.float32), xform="softmax")
    raw_mean, raw_var = p.predictMoments(Xv, transform="none", sd=2.0, mean=0.5)
    check_moments("predictor logits, de-normalised", raw_mean, raw_var, logits, None, scale=2.0, shift=0.5)
    # every second network under the Gaussian likelihood
    g = GaussianLikelihood(sd=0.1)
    per_net, rows = p.logPredictiveDensity(X, Y, n=2, likelihood=g)
    host = np.array(p._data_logprob(g, X, Y, 2), dtype=np.float64)
    f = np.array(p.predict(X, 2))
    sd = np.array([np.float32(p.hypers[i][-1]) for i in range(0, p.numNetworks, 2)], dtype=np.float32)
    _l, _e, mag = loglik_terms(f, Y, LIK_GAUSSIAN, sd)
    tol = X.shape[0] * u * mag                                                        # what float32 np.sum over n rows allows
    print(f"[ensemble] predictor gaussian: per_network vs _data_logprob worst err/tol {np.max(np.abs(per_net - host) / tol):.3f}")
    assert per_net.shape == host.shape and rows.shape == (600,)
    assert np.all(np.abs(per_net - host) <= tol)
    check_loglik("predictor gaussian", per_net, rows, f, Y, LIK_GAUSSIAN, sd, None)
    # the categorical data term in fp64, and the held-out log predictive density
    per_cat, rows_cat = p.logPredictiveDensity(Xv, Yv)
    check_loglik("predictor categorical", per_cat, rows_cat, logits, Yv, LIK_CATEGORICAL, None, None)
    assert np.all(rows_cat <= 0)
