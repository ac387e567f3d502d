"""GPU: the predictive distribution of a new POSITIVE observation under the Gamma likelihood (tbnn_ensemble_predictive with TBNN_LIK_GAMMA,
predictor.predictiveQuantiles / predictiveInterval / predictiveCDF / predictMoments(noiseVariance=True)) against fp64 SciPy applied to the
fp32 predictions Chain.forward_many returns for the same thetas and rows -- the helpers, shapes and bound of tests/test_gpu_predictive.py,
so the test isolates the mixture CDF and its inversion.  Every test here fails without the feature (the likelihood code is refused).

The mixture: F(y) = sum_i (w_i / W) P(a, a y exp(-f_i)) for y > 0 (0 at and below 0), P the regularised lower incomplete gamma function --
on the device a series or a continued fraction in fp64 (csrc/kernels_ensemble.hpp ens_gamma_p), here scipy.special.gammainc, the sum over
the networks in extended precision where the platform has it.  The bound is test_gpu_predictive's with this term's figure:
      T(m) = (m + 8) U + 4 P_FIG,   U = 2^-53.

P_FIG is the largest |device - scipy.special.gammainc| of one network through the CDF entry point on test_term_accuracy_on_a_grid's grid
(shapes 0.05, 0.5, 1, 2, 10, 37.5, 200 and 5000.3; x / a swept over e^-6 .. e^3 and x within a +- 8 sqrt a), measured on an MI355X; the
test prints it on every run and asserts 4 x the recorded value, the margin for inputs the grid misses, and 1e-9 whatever was recorded.  The
figure holds the rounding of the argument a y exp(-f) on both sides as well (x p(x) times an ulp of x: up to sqrt(a / 2 pi) ulps at
x = a).  Measured: 4.774e-15, at a = 5000.3, x = 4974.35 (a = 0.5: 4.6e-15; a = 200: 1.1e-15); below 1e-3 the device's P agrees with
SciPy's to 1.9e-13 of itself.  The NumPy port of the device's function has 4.2e-15 on the host (tests/test_gamma_host.py).

Quantiles.  The CDF is continuous, so no element is excepted: the device returns the upper end b of a bracket of at most 2 ulp64(b) with
F_dev(a) < p <= F_dev(b), or a point with F_dev == p, and |F_dev - F_ref| <= T gives, per probability,
      F_ref(q) >= p - T   and   F_ref(q - 4 ulp64(q)) <= p + T,
with q > 0 and monotone in p.  Probabilities 0.03, 0.5 and 0.97, and 1e-6 at a = 0.5, where the lower tail must be formed directly (T is
1e-8 of that p).  Closed forms: a = 1 is a mixture of exponentials, F = 1 - sum_i (w_i / W) exp(-y e^-f_i); identical networks give one
Gamma distribution, q* = mu g_p / a with g_p = scipy.special.gammaincinv(a, p), and test_gpu_predictive's conditioning bound restated for
this density: F_dev is known to E(m) = 4 P_FIG + (m + 1) U, and F has the slope d = (a / mu) g_p^(a-1) e^-g_p / Gamma(a) at q*, so
      |q - q*| <= (E(m) + 4 U + |P(a, g_p) - p|) / d + 8 ulp64(q*),
the 4 U and the residual for SciPy's own inversion (the residual of its g_p, evaluated with scipy.special.gammainc, and that evaluation's
rounding) and the last term for the rounding of q* and of q."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.special as sp

from test_gpu_ensemble import CASES, make_chain, problem
from test_gpu_predictive import U, int_weights, mix, setup
from test_gpu_quantiles import ROWS

pytestmark = pytest.mark.gpu

GAMMA = 14
# the largest |device - SciPy| of one term on test_term_accuracy_on_a_grid's grid, measured on an MI355X (module docstring)
P_FIG = 4.774e-15
P_GAM = [0.03, 0.5, 0.97]
MS = [1, 2, 3, 64, 65, 257]
SHAPE = {"narrow": 0.5, "mid2": 2.0, "layered10": 10.0, "generic4": 200.0}
GRID_SHAPES = (0.05, 0.5, 1.0, 2.0, 10.0, 37.5, 200.0, 5000.3)
NET = [1, 16, 16, 1]


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """the two run-time shapes of test_predictor_end_to_end, compiled before any test touches the GPU (cached)"""
    from tensorbnn_amd import jit
    layers = [[NET[i], NET[i + 1], 2 if i < len(NET) - 2 else 0, 0] for i in range(len(NET) - 1)]      # tanh, Cauchy priors
    jobs = [{"layers": layers, "likelihood": lik, "skip": "", "flags": ""} for lik in (GAMMA, 1)]
    assert jit.prebuild(jobs, processes=2) == len(jobs)


def T(m):
    return (m + 8) * U + 4 * P_FIG


def a64(a):
    """the shape as the library holds it: an fp32"""
    return float(np.float32(a))


def gam_terms(y, f, a):
    """P(a, a y exp(-f_i)) per network, 0 for y <= 0: y [d_out, n] (or broadcastable), f fp32 [m, d_out, n]"""
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(over="ignore"):
        x = (a64(a) * np.maximum(y, 0.0))[None] * np.exp(-f.astype(np.float64))
    return np.where(y[None] > 0, sp.gammainc(a64(a), x), 0.0)


def F_gam(y, f, w, a):
    """F(y); networks of weight 0 are left out of the sum (they add nothing, whatever they hold)"""
    if w is not None:
        keep = np.asarray(w) > 0
        f, w = f[keep], np.asarray(w)[keep]
    return mix(gam_terms(y, f, a), w)


def check_gam_quantiles(tag, q, probs, f, w, a):
    m = f.shape[0]
    t = T(m)
    worst = 0.0
    for j, p in enumerate(probs):
        assert np.all(np.isfinite(q[j])) and np.all(q[j] > 0), (tag, p)
        at = F_gam(q[j], f, w, a)
        below = F_gam(q[j] - 4 * np.spacing(q[j]), f, w, a)
        worst = max(worst, float((p - at).max()), float((below - p).max()))
        assert np.all(at >= p - t), (tag, p, float((p - at).max()), t)
        assert np.all(below <= p + t), (tag, p, float((below - p).max()), t)
    print(f"[gamma predictive] {tag}: m={m} a={a:g} quantiles, worst excess over p {worst:.3e} (T {t:.3e})")
    order = np.argsort(probs)
    assert np.all(np.diff(q[order], axis=0) >= 0), tag       # monotone in p


def gam_setup(native, name, m, seed=0):
    ch, X, thetas = setup(native, name, m, seed=seed, rates=True)
    ch.set_lik_df(SHAPE[name])                   # (the handles of tests/test_gpu_ensemble.py are Gaussian ones: a comes from the setter)
    return ch, X, thetas, SHAPE[name]


# --------------------------------------------------------------------------------------------- the per-term figure, measured on a grid
def test_term_accuracy_on_a_grid(native):
    """one network through the CDF entry point, 1,237 rows at each of eight shapes: the device's P against scipy.special.gammainc with
    x / a swept over e^-6 .. e^3 (800 points) and x within a +- 8 sqrt a (437 points).  Prints the largest difference -- P_FIG records it
    -- and asserts 4 x the recorded figure, and 1e-9 whatever was recorded."""
    name = "narrow"
    ch, X, th = setup(native, name, 1, seed=21, rates=True)
    n = X.shape[0]
    assert n == 1237
    fp = ch.forward_many(th, X=X)
    mu = np.exp(fp[0, 0].astype(np.float64))
    worst, where, elements = 0.0, None, 0
    for a in GRID_SHAPES:
        ch.set_lik_df(a)
        aa = a64(a)
        x = np.concatenate([aa * np.exp(np.linspace(-6.0, 3.0, 800)), np.maximum(aa + math.sqrt(aa) * np.linspace(-8.0, 8.0, 437), aa * 1e-3)])
        Y = (x * mu / aa).astype(np.float32)[:, None]
        assert np.all(Y > 0) and np.all(np.isfinite(Y))
        _q, F, Fb = ch.ensemble_predictive(th, Y=Y, X=X, likelihood=GAMMA)
        assert Fb is None and F.shape == (1, n)
        ref = gam_terms(Y.T, fp, a)[0]
        e = np.abs(F - ref)[0]
        i = int(np.argmax(e))
        xi = aa * float(Y[i, 0]) / mu[i]
        low = ref[0] < 1e-3
        rel = float(np.max(e[low & (ref[0] > 1e-30)] / ref[0][low & (ref[0] > 1e-30)], initial=0.0))
        print(f"[gamma predictive] a = {a:g}: max |dev - gammainc| {e.max():.3e} at x = {xi:.6g} (x / a = {xi / aa:.4g}); below 1e-3 the largest "
              f"relative difference {rel:.3e}")
        if e.max() > worst:
            worst, where = float(e.max()), (a, xi)
        elements += n
        assert np.all((F >= 0) & (F <= 1))
    print(f"[gamma predictive] per-term figure over {elements} elements: max |dev - gammainc| {worst:.3e} at (a, x) = {where} (P_FIG {P_FIG:.1e})")
    assert worst <= 1e-9
    assert worst <= 4 * P_FIG
    ch.close()


# ------------------------------------------------------------------------------------------------------------------- every shape, every m
@pytest.mark.parametrize("name,m", [(n_, m_) for n_ in ROWS for m_ in MS])
def test_cdf_and_quantiles_against_scipy(native, name, m):
    """m = 1, 2 (no interior), 3, the wavefront size and one more, 257; d_out 1, 2, 4 and 10 over the cases, a 0.5, 2, 10 and 200; network
    2 a copy of network 0; log-means around 1.5; equal weights and integer weights with zeros; targets at and below 0 give F = 0"""
    d_out = CASES[name][0][-1]
    rng = np.random.default_rng(31)
    ch, X, thetas, a = gam_setup(native, name, m)
    n = X.shape[0]
    f = ch.forward_many(thetas, X=X)
    if m > 2:
        assert np.array_equal(f[0], f[2])
    mu0 = np.exp(f[0].astype(np.float64))
    Yp = np.maximum(rng.gamma(a64(a), mu0 / a64(a)), 1e-30).T.astype(np.float32)
    Yp[0] = 0.0
    Yp[1] = -1.5
    probs = ([1e-6] if a == 0.5 else []) + P_GAM          # the far lower tail where the shape puts mass next to 0: ens_gamma_p's direct side
    # (m = 257 at the two cases of 2,000 and 12,000 elements takes the integer weights alone, as tests/test_gpu_predictive.py does: the
    # reference's 2 n_probs + 1 evaluations of m incomplete gamma functions per element cost seconds there)
    for tag, w in (("equal", None), ("integer weights", int_weights(m)))[m > 65 and name in ("generic4", "layered10"):]:
        q, F, Fb = ch.ensemble_predictive(thetas, probs=probs, Y=Yp, X=X, likelihood=GAMMA, weights=w)
        assert q.shape == (len(probs), d_out, n) and F.shape == (d_out, n) and Fb is None and q.dtype == F.dtype == np.float64
        err = np.abs(F - F_gam(Yp.T, f, w, a))
        print(f"[gamma predictive] {name} {tag}: m={m} a={a:g} CDF err max {err.max():.3e} (T {T(m):.3e})")
        assert np.all(err <= T(m)), (tag, float(err.max()))
        assert not F[:, :2].any() and np.all((F >= 0) & (F <= 1))
        check_gam_quantiles(f"{name} {tag}", q, probs, f, w, a)
    again = ch.ensemble_predictive(thetas, probs=probs, Y=Yp, X=X, likelihood=GAMMA, weights=w)
    assert Fb is None and again[2] is None
    assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(again[:2], (q, F)))
    ch.close()


def test_closed_forms(native):
    """a = 1: the mixture of exponentials, F = 1 - sum_i (w_i / W) exp(-y e^-f_i); one network, five identical networks and the same five
    weighted: one Gamma distribution, q = mu g_p / a within the conditioning bound of the module docstring"""
    name = "mid2"
    ch, X, thetas = setup(native, name, 5, seed=41, rates=True)
    rng = np.random.default_rng(42)
    f = ch.forward_many(thetas, X=X)
    n = X.shape[0]
    ch.set_lik_df(1.0)
    Y = rng.exponential(np.exp(f[0].astype(np.float64))).T.astype(np.float32)
    Y[::9] *= np.float32(1e-6)                                         # the lower tail: 1 - exp(-x) by expm1, not by a difference from 1
    for w in (None, int_weights(5)):
        _q, F, _b = ch.ensemble_predictive(thetas, Y=Y, X=X, likelihood=GAMMA, weights=w)
        keep = np.ones(5, bool) if w is None else w > 0
        want = mix(-np.expm1(-Y.T.astype(np.float64)[None] * np.exp(-f[keep].astype(np.float64))), None if w is None else w[keep])
        err = np.abs(F - want)
        print(f"[gamma predictive] a = 1 against the mixture of exponentials: err max {err.max():.3e} (T {T(5):.3e})")
        assert np.all(err <= T(5))
    probs = [1e-6, 0.03, 0.05, 0.41, 0.5, 0.95, 0.97]
    for a in (0.5, 2.0, 200.0):
        ch.set_lik_df(a)
        g = sp.gammaincinv(a64(a), np.asarray(probs))[:, None, None]
        resid = np.abs(sp.gammainc(a64(a), g) - np.asarray(probs)[:, None, None])          # what SciPy's own g_p misses p by
        dens_g = np.exp((a64(a) - 1.0) * np.log(g) - g - math.lgamma(a64(a)))          # the standard Gamma(a, 1) density at g_p
        for tag, m, w in (("one network", 1, None), ("five identical", 5, None), ("five identical, weighted", 5, int_weights(5))):
            th = np.repeat(thetas[:1], m, axis=0)
            fm = ch.forward_many(th, X=X)
            q, _F, _b = ch.ensemble_predictive(th, probs=probs, X=X, likelihood=GAMMA, weights=w)
            mu = np.exp(fm[0].astype(np.float64))[None]
            want = mu * g / a64(a)
            tol = (4 * P_FIG + (m + 1) * U + 4 * U + resid) / (a64(a) / mu * dens_g) + 8 * np.spacing(want)
            err = np.abs(q - want)
            print(f"[gamma predictive] closed form, a = {a:g}, {tag}: worst err / tol {np.max(err / tol):.3f}, worst err {np.max(err / np.spacing(want)):.1f} ulp64 of q*")
            assert np.all(err <= tol), (a, tag, float(np.max(err / tol)))
    ch.close()


# --------------------------------------------------------------------------------------------------------------------------- row blocks
def test_row_blocks_and_the_handle_s_own_shape(native, monkeypatch):
    """517 rows in blocks of 192 (three blocks, the last of 133 rows), the staged rows and targets, and a Gamma handle whose a is its
    descriptor's: both outputs bit for bit those of the single-block call on the Gaussian handle with the setter"""
    name, m, rb = "generic4", 8, 192
    ch, X, thetas, a = gam_setup(native, name, m, seed=2)
    dims = CASES[name][0]
    d_out = dims[-1]
    n = X.shape[0]
    assert n == 517 and -(-n // rb) == 3
    Y = np.random.default_rng(61).gamma(2.0, 2.0, (n, d_out)).astype(np.float32)
    kw = {"likelihood": GAMMA, "weights": int_weights(m), "probs": P_GAM}
    whole = ch.ensemble_predictive(thetas, Y=Y, X=X, **kw)
    budget = m * d_out * rb + 7
    assert max(64, budget // (m * d_out) // 64 * 64) == rb
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    cut = ch.ensemble_predictive(thetas, Y=Y, X=X, **kw)
    ch.set_data(X, Y)
    staged = ch.ensemble_predictive(thetas, which=0, cdf=True, **kw)
    monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
    own = native.Chain([(dims[i], dims[i + 1], native.ACT_TANH if i < len(dims) - 2 else native.ACT_NONE, 0) for i in range(len(dims) - 1)],
                       likelihood=GAMMA, lik_df=a, kernel=native.KERNEL_GENERIC)
    mine = own.ensemble_predictive(thetas, Y=Y, X=X, weights=kw["weights"], probs=P_GAM)          # likelihood None: the chain's own
    own.close()
    for x, y, z, v in zip(whole[:2], cut[:2], staged[:2], mine[:2]):
        assert x is not None
        for other in (y, z, v):
            assert np.array_equal(x.view(np.uint64), other.view(np.uint64))
    assert whole[2] is None and cut[2] is None and staged[2] is None and mine[2] is None
    # the CDF alone, and the quantiles alone
    assert np.array_equal(ch.ensemble_predictive(thetas, Y=Y, X=X, likelihood=GAMMA, weights=kw["weights"])[1], whole[1])
    only_q = ch.ensemble_predictive(thetas, X=X, **kw)
    assert only_q[1] is None and only_q[2] is None and np.array_equal(only_q[0], whole[0])
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------ probabilities
def test_more_probabilities_than_one_register_group(native):
    """19 probabilities run as groups of 4, 4, 4, 4 and 3: each agrees bit for bit with a call of its own, and they are monotone"""
    m = 9
    ch, X, thetas, a = gam_setup(native, "generic4", m, seed=3)
    w = int_weights(m)
    probs = [(k + 0.37) / 19 for k in range(19)]
    q = ch.ensemble_predictive(thetas, probs=probs, X=X, likelihood=GAMMA, weights=w)[0]
    assert q.shape == (19, 4, X.shape[0]) and np.all(np.diff(q, axis=0) >= 0) and np.all(q > 0)
    for j, p in enumerate(probs):
        one = ch.ensemble_predictive(thetas, probs=[p], X=X, likelihood=GAMMA, weights=w)[0]
        assert np.array_equal(one[0].view(np.uint64), q[j].view(np.uint64)), j
    ch.close()


# ------------------------------------------------------------------------------------------------------------------ NaN and overflow
def test_nan_and_overflow_stay_in_their_element(native):
    """a NaN input row makes that row's predictions NaN under every network; a row scaled up drives a counted network's log-mean past the
    fp64 range of exp (the mean is inf or 0): NaN in those elements only, in every output; a NaN target gives a NaN CDF and leaves the
    quantiles; a network of weight 0 that holds NaN everywhere is not looked at"""
    name, m = "narrow", 5
    ch, X0, thetas, a = gam_setup(native, name, m, seed=51)
    w = int_weights(m)
    counts = w > 0
    assert not counts[0] and counts[1:].any()
    for scale in (4000.0, -4000.0, 40000.0, -40000.0):       # whichever drives a counted network's log-mean out of range (set-up, not a retry)
        X = X0.copy()
        X[7, 0] = np.nan
        X[300] *= np.float32(scale)
        f = ch.forward_many(thetas, X=X)
        nan_el = np.isnan(f).any(axis=0)
        big_el = (np.abs(f[counts].astype(np.float64)) > 750.0).any(axis=0)
        if big_el[0, 300]:
            break
    assert nan_el.sum() == 1 and nan_el[0, 7] and big_el.sum() == 1 and big_el[0, 300] and np.isfinite(f[:, 0, 300]).all()
    Y = np.ones((X.shape[0], 1), dtype=np.float32)
    Y[11, 0] = np.nan
    Y[12, 0] = np.inf                                         # a number: F = 1
    q, F, Fb = ch.ensemble_predictive(thetas, probs=P_GAM, Y=Y, X=X, likelihood=GAMMA, weights=w)
    bad = nan_el | big_el
    for x in (q[0], q[1], q[2]):
        assert np.array_equal(np.isnan(x), bad)
    bad_y = bad.copy()
    bad_y[0, 11] = True
    assert Fb is None and np.array_equal(np.isnan(F), bad_y) and abs(F[0, 12] - 1.0) <= T(m)
    # the network of weight 0 holding NaN: its last bias is NaN, so every prediction of it is; nothing changes
    th = thetas.copy()
    th[0, -1] = np.nan
    assert np.isnan(ch.forward_many(th, X=X)[0]).all()
    q2, F2, _b = ch.ensemble_predictive(th, probs=P_GAM, Y=Y, X=X, likelihood=GAMMA, weights=w)
    assert np.array_equal(q2.view(np.uint64), q.view(np.uint64)) and np.array_equal(F2.view(np.uint64), F.view(np.uint64))
    # ... and with equal weights the same network counts: NaN everywhere
    q3, F3, _b = ch.ensemble_predictive(th, probs=P_GAM, Y=Y, X=X, likelihood=GAMMA)
    assert np.isnan(q3).all() and np.isnan(F3).all()
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_usable(native):
    dp = C.POINTER(C.c_double)
    ch, X, thetas = setup(native, "narrow", 4, rates=True)
    n, Pn = X.shape[0], thetas.shape[1]
    lib, p = native.lib, native._p
    Y = np.ones((n, 1), dtype=np.float32)
    before = ch.forward_many(thetas, X=X)
    qo, Fo, Bo = np.full((3, 1, n), 7.0), np.full((1, n), 7.0), np.full((1, n), 7.0)
    pr = np.asarray(P_GAM, dtype=np.float64)

    def call(q=True, cdf=False, below=False):
        return lib.tbnn_ensemble_predictive(ch._h, p(thetas), 4, Pn, GAMMA, None, None, 1, p(X), p(Y), n, pr.ctypes.data_as(dp), 3,
                                            qo.ctypes.data_as(dp) if q else None, Fo.ctypes.data_as(dp) if cdf else None,
                                            Bo.ctypes.data_as(dp) if below else None)

    err = lambda: lib.tbnn_last_error().decode()
    # no shape on this (Gaussian) handle yet
    assert call() < 0 and "tbnn_set_lik_df" in err() and "TBNN_LIK_GAMMA" in err()
    ch.set_lik_df(2.0)
    assert call(cdf=True, below=True) < 0 and "continuous CDF has no step" in err()
    assert call(q=False) < 0 and "both null" in err()
    assert np.all(qo == 7.0) and np.all(Fo == 7.0) and np.all(Bo == 7.0)          # nothing written
    with pytest.raises(native.TbnnError, match="TBNN_LIK_GAMMA is not built"):
        ch.ensemble_crps(thetas, Y=Y, X=X, likelihood=GAMMA)
    with pytest.raises(native.TbnnError, match="those of a label"):
        ch.ensemble_uncertainty(thetas, X=X, likelihood=GAMMA)
    assert call(cdf=True) == 0 and not np.any(qo == 7.0) and not np.any(Fo == 7.0) and np.all(Bo == 7.0)
    assert np.array_equal(ch.forward_many(thetas, X=X), before)
    ch.close()


# ---------------------------------------------------------------------------------------------------------------- predictor, end to end
def test_predictor_end_to_end(tmp_path, monkeypatch, native):
    """positive targets trained for a few epochs under GammaLikelihood(shape=2), then the saved run: the predictive interval is ordered
    and positive and contains the credible interval of the mean, the PIT is the mixture CDF of the saved networks at y, noiseVariance adds
    E[mu^2] / a to the posterior spread of the mean, and the CRPS is refused"""
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.likelihood import GammaLikelihood
    from tensorbnn_amd.network import network
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    rng = np.random.default_rng(71)
    a = 2.0
    X = rng.uniform(-2, 2, (300, 1)).astype(np.float32)
    mu = np.exp(1.0 + np.sin(2 * X.astype(np.float64)))
    Y = np.maximum(rng.gamma(a, mu / a), 1e-30).astype(np.float32)
    lik = GammaLikelihood(shape=a)
    net = network(np.float32, 1, X, Y, X[:50], Y[:50])
    net.add(DenseLayer(1, 16, seed=1000)); net.add(Tanh())
    net.add(DenseLayer(16, 16, seed=2000)); net.add(Tanh())
    net.add(DenseLayer(16, 1, seed=3000))
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    net.train(30, 2, lik, folderName="gam", networksPerFile=1, verbose=False)
    assert ",gamma;" in net._chain.kernel_name, net._chain.kernel_name
    p = predictor(str(tmp_path / "gam") + "/", likelihood=lik)
    m = p.numNetworks
    assert m >= 4
    lower, median, upper = p.predictiveInterval(X, level=0.9)
    assert lower.shape == median.shape == upper.shape == (1, 300)
    assert np.all(lower > 0) and np.all(lower < median) and np.all(median < upper)
    q = p.predictiveQuantiles(X, [0.05, 0.5, 0.95])
    assert np.array_equal(q[0], lower) and np.array_equal(q[1], median) and np.array_equal(q[2], upper)
    assert np.array_equal(p.predictiveQuantiles(X, 0.5), median)
    f = np.array(p.predict(X))
    check_gam_quantiles("predictor", q, [0.05, 0.5, 0.95], f, None, a)
    c_lo, _c_med, c_hi = p.predictInterval(X, level=0.9)                                # the mean's credible interval (exp by default)
    assert np.all(lower <= c_lo) and np.all(c_hi <= upper)
    F = p.predictiveCDF(X, Y)
    yt = Y.T.astype(np.float64)
    assert isinstance(F, np.ndarray) and np.all(np.abs(F - F_gam(yt, f, None, a)) <= T(m))
    inside = float(np.mean((yt >= lower) & (yt <= upper)))
    print(f"[gamma predictive] predictor: {m} networks; share of the training targets inside the 90 % predictive interval {inside:.3f}")
    mean, var = p.predictMoments(X)
    mean2, tot = p.predictMoments(X, noiseVariance=True)
    assert np.array_equal(mean, mean2) and np.array_equal(tot, var + (var + mean * mean) / a) and np.all(tot > var)
    # every second network, reweighted; Gamma targets take no de-normalisation
    w = np.arange(1, len(range(0, m, 2)) + 1, dtype=np.float32)
    q2 = p.predictiveQuantiles(X, [0.25, 0.75], n=2, weights=w)
    check_gam_quantiles("predictor, every second network", q2, [0.25, 0.75], f[::2], w, a)
    with pytest.raises(ValueError, match="GammaLikelihood"):
        p.predictiveQuantiles(X, [0.5], sd=2.0)
    with pytest.raises(ValueError, match="not built for a GammaLikelihood"):
        p.crps(X, Y)
    with pytest.raises(ValueError, match="GammaLikelihood"):
        p.predictUncertainty(X)
    per_net, per_row = p.logPredictiveDensity(X, Y)
    assert per_net.shape == (m,) and np.all(np.isfinite(per_row))
