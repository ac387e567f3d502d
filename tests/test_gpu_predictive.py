"""GPU: the predictive distribution of a new observation over an ensemble (tbnn_ensemble_predictive, Chain.ensemble_predictive,
predictor.predictiveQuantiles / predictiveInterval / predictiveCDF) against fp64 NumPy / SciPy applied to the fp32 predictions
Chain.forward_many returns for the same thetas and rows.  The forward kernels are shared, so both sides start from the same bits and the
test isolates the mixture CDF and its inversion.  Every test here fails without the entry point (it does not exist before this module's
feature).

The bound T (U = 2^-53).  The device forms F = sum_i (w_i / W) term_i in network order, term_i = Phi((y - f_i) / s_i) or Q(k + 1, lambda_i),
every term in [0, 1]:
  * the sequential fp64 sum of m products carries at most (m - 1) U times the sum of their magnitudes (Higham, Accuracy and Stability of
    Numerical Algorithms, eq. 4.4), which is at most 1; the rounded quotients w_i / W and the m products add 2 U of the same sum;
    the reference divides once more and the comparison rounds: together (m + c) U with c = 8.  The reference's own sum is taken in extended
    precision where the platform has it (LD below), so that this term is the device's alone;
  * each term differs from the reference's by the error of the device's erfc (and of its argument (y - f) / (s sqrt 2)) or of its
    incomplete gamma function plus the error of SciPy's: the per-term figures PHI_FIG and Q_FIG are the largest differences
    test_term_accuracy_on_a_grid finds on its grid on an MI355X (it prints them on every run and asserts 4 x the recorded ones; they are
    also in DESIGN.md section 4.6), taken times a margin of 4 for inputs the grid missed.  The weights w_i / W sum to 1, so the terms'
    errors enter F at most once.
      T(m, kind) = (m + 8) U + 4 FIG(kind)
Both figures hold the reference's error too: scipy.special.gammaincc is itself off by up to 2.8e-11 at isolated points near k = 1e6
(DESIGN.md section 4.6), so Q_FIG is mostly SciPy's; the other tests use rates of a few hundred at the most, where the two agree to 1e-14.
Whatever the grid gives, a Q figure above 1e-9 fails the test: the implementation would not be good enough.

Gaussian quantiles.  The device returns the upper end b of a bracket a < b of at most 2 ulp64 with F_dev(a) < p <= F_dev(b), or a point
with F_dev == p.  |F_dev - F_ref| <= T gives F_ref(b) >= p - T, and a >= b - 2 ulp64(b) >= b - 4 ulp64(b) with F_ref monotone gives
F_ref(b - 4 ulp64(b)) <= F_ref(a) <= p + T: the criterion the tests assert, which holds whatever the slope of F -- also where the mixture is
flat between separated modes.  Closed forms (one network, or all networks identical: F is one Gaussian's CDF and q* = f + s z_p).  Here
F_dev is a sum of m equal terms: E(m) = 4 PHI_FIG + (m + 1) U bounds its error (the term; m - 1 additions, the quotients w_i / W and the
products).  The bracket puts q within 2 ulp64 of a point where |F - p| <= E, and F has the slope phi(z_p) / s there (over a distance of
1e-13 s the slope does not change in its first ten digits), so
      |q - q*| <= E(m) s / phi(z_p) + 4 ulp64(q) + 4 ulp64(|f| + s |z_p|),
the last term for the rounding of q* itself with SciPy's z_p.  The first term is the conditioning of the problem, not slack: F is known
to E only, and at p = 1/2 with f near 0 it is E s / 0.4 = 1e-15 s however small |f| + s |z_p| and its ulp are; at the six probabilities
of the test it is 3 to 16 E s.  A search that stopped early by more than that fails.

Poisson quantiles are integers and must equal the reference's, except where the reference's own decision is closer to p than T:
min(|F_ref(k*) - p|, |F_ref(k* - 1) - p|) < T, where k* +- 1 is accepted -- for at most 0.1 % of a test's elements (the count is printed).
"""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.special as sp
import scipy.stats as st

from test_gpu_ensemble import CASES, make_chain, net_weights, problem
from test_gpu_quantiles import ROWS

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble if np.finfo(np.longdouble).eps < 2.0 ** -60 else np.float64
# the largest |device - SciPy| of one term on test_term_accuracy_on_a_grid's grid, measured on an MI355X (module docstring)
PHI_FIG = 2.220e-16
Q_FIG = 1.593e-14
GAUSS, FIXED, POISSON = 0, 1, 5

P_GAUSS = [0.05, 0.5, 0.95]
P_POIS = [0.03, 0.41, 0.97]            # none a multiple of 1 / W for the small m: no exact ties between a flat CDF and p
SMALL_M = [1, 2, 3, 64, 65]


def T(m, kind):
    return (m + 8) * U + 4 * (Q_FIG if kind == POISSON else PHI_FIG)


def setup(native, name, m, seed=0, rates=False):
    """network 2 a copy of network 0.  rates: the last layer of every network rescaled so that the outputs, read as log-rates, have mean
    about 1.5 and standard deviation 1.2 over the ensemble and the rows (rates of a few counts, a few hundred at the most)"""
    X, thetas = problem(name, m, seed=seed, n=ROWS[name])
    if m > 2:
        thetas[2] = thetas[0]
    ch = make_chain(native, name)
    if rates:
        dims = CASES[name][0]
        d_out, last = dims[-1], dims[-2] * dims[-1] + dims[-1]       # theta ends with the last layer's weights, then its biases
        f = ch.forward_many(thetas, X=X).astype(np.float64)
        scale = 1.2 / f.std()
        thetas[:, -last:] = (thetas[:, -last:].astype(np.float64) * scale).astype(np.float32)
        thetas[:, -d_out:] += np.float32(1.5 - scale * f.mean())
    return ch, X, thetas


def sds(m, seed=2):
    """per-network standard deviations spread over two decades"""
    s = 10.0 ** np.linspace(-1.5, 0.5, m) if m > 1 else np.array([0.4])
    return np.random.default_rng(seed).permutation(s).astype(np.float32)


def int_weights(m, seed=1):
    """0 .. 3, with zeros and at least one positive"""
    w = np.random.default_rng(seed).integers(0, 4, m).astype(np.float32)
    w[0] = 0.0 if m > 1 else 2.0
    w[-1] = 2.0
    return w


def mix(terms, w):
    """sum_i w_i terms_i / W over axis 0, the sum in LD"""
    w = np.ones(terms.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    wl = w.astype(LD).reshape((-1,) + (1,) * (terms.ndim - 1))
    return np.asarray((wl * terms.astype(LD)).sum(axis=0) / w.astype(LD).sum(), dtype=np.float64)


def clip_sd(sd):
    return np.clip(np.asarray(sd, dtype=np.float32), np.float32(1e-8), np.float32(1e8)).astype(np.float64)


def F_gauss(y, f, sd, w):
    """y [d_out, n] (or broadcastable), f fp32 [m, d_out, n]"""
    s = clip_sd(sd)[:, None, None]
    return mix(sp.ndtr((np.asarray(y, dtype=np.float64)[None] - f.astype(np.float64)) / s), w)


def F_pois(k, f, w):
    """F(k) at integer-valued k [d_out, n]; 0 below 0"""
    k = np.asarray(k, dtype=np.float64)
    lam = np.exp(f.astype(np.float64))
    return np.where(k < 0, 0.0, mix(st.poisson.cdf(np.maximum(k, 0.0)[None], lam), w))


def pois_quantile_ref(p, f, w):
    """the smallest integer k >= 0 with F_pois(k) >= p: a bracket around the components' quantiles in the normal approximation, pushed
    outward until F_pois itself says F(lo) < p <= F(hi) (lo = -1: F = 0), then bisection"""
    lam = np.exp(f.astype(np.float64))
    keep = np.ones(f.shape[0], bool) if w is None else np.asarray(w) > 0
    guess = lam[keep] + sp.ndtri(p) * np.sqrt(lam[keep])
    lo, hi = np.maximum(np.floor(guess.min(axis=0)) - 3.0, -1.0), np.ceil(guess.max(axis=0)) + 3.0
    step = 2.0
    while True:
        up, down = F_pois(hi, f, w) < p, (lo >= 0) & (F_pois(lo, f, w) >= p)
        if not up.any() and not down.any():
            break
        hi, lo = np.where(up, hi + step, hi), np.where(down, np.maximum(lo - step, -1.0), lo)
        step *= 2
    while np.any(hi - lo > 1):
        mid = np.floor((lo + hi) / 2)
        ge = F_pois(mid, f, w) >= p
        act = hi - lo > 1
        hi, lo = np.where(act & ge, mid, hi), np.where(act & ~ge, mid, lo)
    return hi


def check_gauss_quantiles(tag, q, probs, f, sd, w):
    m = f.shape[0]
    t = T(m, GAUSS)
    worst = 0.0
    for j, p in enumerate(probs):
        at = F_gauss(q[j], f, sd, w)
        below = F_gauss(q[j] - 4 * np.spacing(np.abs(q[j])), f, sd, w)
        worst = max(worst, float((p - at).max()), float((below - p).max()))
        assert np.all(np.isfinite(q[j])), (tag, p)
        assert np.all(at >= p - t), (tag, p, float((p - at).max()), t)
        assert np.all(below <= p + t), (tag, p, float((below - p).max()), t)
    print(f"[predictive] {tag}: m={m} Gaussian quantiles, worst excess over p {worst:.3e} (T {t:.3e})")
    order = np.argsort(probs)
    assert np.all(np.diff(q[order], axis=0) >= 0), tag       # monotone in p


def check_pois_quantiles(tag, q, probs, f, w):
    m = f.shape[0]
    t = T(m, POISSON)
    used = total = 0
    for j, p in enumerate(probs):
        ks = pois_quantile_ref(p, f, w)
        margin = np.minimum(np.abs(F_pois(ks, f, w) - p), np.abs(F_pois(ks - 1, f, w) - p))
        diff = q[j] != ks
        ok = ~diff | ((margin < t) & (np.abs(q[j] - ks) <= 1))
        assert ok.all(), (tag, p, q[j][~ok][:5], ks[~ok][:5])
        assert np.array_equal(q[j], np.floor(q[j])) and np.all(q[j] >= 0)
        used += int(diff.sum()); total += diff.size
    print(f"[predictive] {tag}: m={m} Poisson quantiles, {used} of {total} elements within T of a tie took the exception")
    assert used <= 0.001 * total, (tag, used, total)


# --------------------------------------------------------------------------------------------- the per-term figures, measured on a grid
def test_term_accuracy_on_a_grid(native):
    """one network through the CDF entry point: the device's Phi against scipy.special.ndtr at targets swept over +-38 sd, its Q against
    scipy.special.gammaincc at counts 0 .. 2^20 and rates up to 2^20 (around k = lambda, where Q moves, and far from it).  Prints the largest
    differences -- PHI_FIG and Q_FIG record these figures -- and asserts 4 x the recorded ones, and 1e-9 for Q whatever was recorded."""
    name = "narrow"
    X, thetas = problem(name, 1, seed=21, n=40009)
    ch = make_chain(native, name)
    n = X.shape[0]
    f = ch.forward_many(thetas, X=X)
    sd = np.array([1.3], dtype=np.float32)
    z = np.linspace(-38.0, 38.0, n)
    Y = (f[0, 0].astype(np.float64) + z * float(sd[0])).astype(np.float32)[:, None]
    _q, F, _b = ch.ensemble_predictive(thetas, Y=Y, X=X, likelihood=GAUSS, sd=sd)
    ref = sp.ndtr((Y.T.astype(np.float64) - f[0].astype(np.float64)) / float(sd[0]))
    e_phi = float(np.abs(F - ref).max())
    tail = (ref < 1e-3) & (ref > 1e-290)
    rel = float(np.max(np.abs(F - ref)[tail] / ref[tail]))
    assert np.array_equal(F, ch.ensemble_predictive(thetas, Y=Y, X=X, likelihood=FIXED, sd=sd)[1])
    # log-rates from log 0.05 to log 2^20: the last layer rescaled (theta ends with its 50 weights and its bias)
    f0 = f[0, 0].astype(np.float64)
    alpha = (math.log(2.0 ** 20) - math.log(0.05)) / (f0.max() - f0.min())
    th = thetas.copy()
    th[0, -51:] = (th[0, -51:].astype(np.float64) * alpha).astype(np.float32)
    th[0, -1] += np.float32(math.log(0.05) - alpha * f0.min())
    fp = ch.forward_many(th, X=X)
    lam = np.exp(fp[0, 0].astype(np.float64))
    assert lam.min() < 0.1 and 2.0 ** 19 < lam.max() <= 2.0 ** 20 * 1.01
    rng = np.random.default_rng(22)
    k = np.floor(lam + np.sqrt(lam) * rng.uniform(-7, 7, n))
    k[::5] = np.floor(2.0 ** rng.uniform(0, 20, len(k[::5])))
    k[::11] = rng.integers(0, 40, len(k[::11]))
    k = np.clip(k, 0, 2.0 ** 20)
    k[:3] = [0, 2.0 ** 20, 31]
    Yp = k.astype(np.float32)[:, None]
    assert np.array_equal(Yp[:, 0].astype(np.float64), k)
    _q, Fp, Fb = ch.ensemble_predictive(th, Y=Yp, X=X, likelihood=POISSON)
    ref_at = sp.gammaincc(k + 1, lam)
    ref_below = np.where(k >= 1, sp.gammaincc(np.maximum(k, 1), lam), 0.0)
    e_q = float(max(np.abs(Fp[0] - ref_at).max(), np.abs(Fb[0] - ref_below).max()))
    print(f"[predictive] per-term figures: Phi max |dev - ndtr| {e_phi:.3e} (PHI_FIG {PHI_FIG:.1e}; below 1e-3 the largest relative "
          f"difference {rel:.3e}), Q max |dev - gammaincc| {e_q:.3e} (Q_FIG {Q_FIG:.1e})")
    assert e_q <= 1e-9
    assert e_phi <= 4 * PHI_FIG and e_q <= 4 * Q_FIG
    assert np.all((Fp >= 0) & (Fp <= 1)) and np.all(Fb <= Fp)
    ch.close()


# ------------------------------------------------------------------------------------------------------- both kinds, every shape
@pytest.mark.parametrize("name,m", [(n_, m_) for n_ in ROWS for m_ in SMALL_M + [257]])
def test_cdf_and_quantiles_against_scipy(native, name, m):
    """m = 1, 2 (no interior), 3, the wavefront size and one more, 257; d_out 1, 2, 4 and 10 over the cases; network 2 a copy of network 0;
    per-network sd's over two decades; equal weights, real weights with a zero and integer weights with zeros"""
    d_out = CASES[name][0][-1]
    rng = np.random.default_rng(31)
    # Gaussian
    ch, X, thetas = setup(native, name, m)
    n = X.shape[0]
    f = ch.forward_many(thetas, X=X)
    if m > 2:
        assert np.array_equal(f[0], f[2])
    sd = sds(m)
    Y = (f[rng.integers(0, m, n), :, np.arange(n)] + 1.5 * float(sd.max()) * rng.standard_normal((n, d_out))).astype(np.float32)
    for tag, w in (("equal", None), ("weighted", net_weights(m)), ("integer weights", int_weights(m))):
        q, F, Fb = ch.ensemble_predictive(thetas, probs=P_GAUSS, Y=Y, X=X, likelihood=GAUSS, sd=sd, weights=w)
        assert q.shape == (3, d_out, n) and F.shape == (d_out, n) and Fb is None and q.dtype == F.dtype == np.float64
        err = np.abs(F - F_gauss(Y.T, f, sd, w))
        print(f"[predictive] {name} {tag}: m={m} Gaussian CDF err max {err.max():.3e} (T {T(m, GAUSS):.3e})")
        assert np.all(err <= T(m, GAUSS)), (tag, float(err.max()))
        if m == 1:
            pit = sp.ndtr((Y.T.astype(np.float64) - f[0].astype(np.float64)) / float(clip_sd(sd)[0]))
            assert np.all(np.abs(F - pit) <= 4 * PHI_FIG)
        check_gauss_quantiles(f"{name} {tag}", q, P_GAUSS, f, sd, w)
    again = ch.ensemble_predictive(thetas, probs=P_GAUSS, Y=Y, X=X, likelihood=GAUSS, sd=sd, weights=w)
    assert np.array_equal(again[0].view(np.uint64), q.view(np.uint64)) and np.array_equal(again[1].view(np.uint64), F.view(np.uint64))
    # Poisson: log-rates around 1.5
    ch.close()
    ch, X, thetas = setup(native, name, m, rates=True)
    f = ch.forward_many(thetas, X=X)
    assert np.exp(f.astype(np.float64)).max() < 2.0 ** 20
    Yp = rng.poisson(np.exp(f[0].astype(np.float64))).T.astype(np.float32)
    Yp[::7] += np.float32(0.5)                                 # read at floor(y)
    Yp[0] = 0.0
    # (m = 257 at the two cases of 2,000 elements: the reference's search costs 3 s per set of weights there, so they take the integer
    # weights alone; narrow and mid2 run both at 257 too)
    for tag, w in (("equal", None), ("integer weights", int_weights(m)))[m > 65 and name in ("generic4", "layered10"):]:
        q, F, Fb = ch.ensemble_predictive(thetas, probs=P_POIS, Y=Yp, X=X, likelihood=POISSON, weights=w)
        k = np.floor(Yp.T.astype(np.float64))
        e_at, e_below = np.abs(F - F_pois(k, f, w)), np.abs(Fb - F_pois(k - 1, f, w))
        print(f"[predictive] {name} {tag}: m={m} Poisson CDF err max {e_at.max():.3e}, below {e_below.max():.3e} (T {T(m, POISSON):.3e})")
        assert np.all(e_at <= T(m, POISSON)) and np.all(e_below <= T(m, POISSON))
        assert not Fb[:, 0].any() and np.all(Fb <= F)
        check_pois_quantiles(f"{name} {tag}", q, P_POIS, f, w)
    again = ch.ensemble_predictive(thetas, probs=P_POIS, Y=Yp, X=X, likelihood=POISSON, weights=w)
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(again, (q, F, Fb)))
    ch.close()


def test_gaussian_closed_forms(native):
    """one network, five identical networks and the same five weighted: the mixture is one Gaussian and q = f + s z_p (module docstring);
    separated modes: two networks 40 sd apart, where F is flat at 1/2 between them and the criterion still holds"""
    name = "mid2"
    probs = [0.03, 0.05, 0.41, 0.5, 0.95, 0.97]
    ch, X, thetas = setup(native, name, 1, seed=41)
    z = sp.ndtri(probs)[:, None, None]
    s32 = np.float32(0.37)
    s = float(s32)
    for tag, m, w in (("one network", 1, None), ("five identical", 5, None), ("five identical, weighted", 5, int_weights(5))):
        th = np.repeat(thetas, m, axis=0)
        f = ch.forward_many(th, X=X)
        q, _F, _b = ch.ensemble_predictive(th, probs=probs, X=X, likelihood=GAUSS, sd=np.full(m, s32), weights=w)
        f64 = f[0].astype(np.float64)[None]
        want = f64 + s * z
        tol = (4 * PHI_FIG + (m + 1) * U) * s / st.norm.pdf(z) + 4 * np.spacing(np.abs(q)) + 4 * np.spacing(np.abs(f64) + s * np.abs(z))
        err = np.abs(q - want)
        print(f"[predictive] closed form, {tag}: worst err / tol {np.max(err / tol):.3f}, worst err {np.max(err / np.spacing(np.abs(f64) + s * np.abs(z))):.1f} ulp64 of |f| + s |z_p|")
        assert np.all(err <= tol), (tag, float(np.max(err / tol)))
    th = np.repeat(thetas, 2, axis=0)
    th[1, -2:] += np.float32(40 * s)                          # the second network's two output biases
    f = ch.forward_many(th, X=X)
    sd = np.full(2, s32)
    q, _F, _b = ch.ensemble_predictive(th, probs=[0.25, 0.5, 0.75], X=X, likelihood=GAUSS, sd=sd)
    check_gauss_quantiles("separated modes", q, [0.25, 0.5, 0.75], f, sd, None)
    assert np.all(q[0] < f[0] + 1.0) and np.all(q[2] > f[1] - 1.0)
    ch.close()


def test_nan_and_absurd_rates_stay_in_their_element(native):
    """a NaN input row makes that row's predictions NaN under every network; a row scaled up drives some network's log-rate past log 2^30:
    NaN in those elements only, in all three outputs, whatever the other networks say"""
    name, m = "narrow", 5
    ch, X0, thetas = setup(native, name, m, seed=51, rates=True)
    w = int_weights(m)
    counts = w > 0
    for scale in (400.0, -400.0, 4000.0, -4000.0):           # whichever drives a counted network's log-rate up (set-up, not a retry)
        X = X0.copy()
        X[7, 0] = np.nan
        X[300] *= np.float32(scale)
        f = ch.forward_many(thetas, X=X)
        with np.errstate(over="ignore"):
            lam = np.exp(f.astype(np.float64))
        nan_el = np.isnan(f).any(axis=0)
        big_el = (lam[counts] > 2.0 ** 30).any(axis=0)
        if big_el[0, 300]:
            break
    assert nan_el.sum() == 1 and nan_el[0, 7] and big_el.sum() == 1 and big_el[0, 300] and np.isfinite(f[:, 0, 300]).all()
    Y = np.ones((X.shape[0], 1), dtype=np.float32)
    q, F, Fb = ch.ensemble_predictive(thetas, probs=P_POIS, Y=Y, X=X, likelihood=POISSON, weights=w)
    bad = nan_el | big_el
    for a in (q[0], q[1], q[2], F, Fb):
        assert np.array_equal(np.isnan(a), bad)
    q, F, _b = ch.ensemble_predictive(thetas, probs=P_GAUSS, Y=Y, X=X, likelihood=GAUSS, sd=sds(m), weights=w)
    for a in (q[0], q[1], q[2], F):
        assert np.array_equal(np.isnan(a), nan_el)            # a large finite prediction is a number to the Gaussian kinds
    ch.close()


# --------------------------------------------------------------------------------------------------------------------------- row blocks
def test_row_blocks(native, monkeypatch):
    """517 rows in blocks of 192: three blocks, the last of 133 rows (the driver's rule: rb = floor(budget / (m d_out)) rounded down to a
    multiple of 64).  The generic kernel runs a row per thread, so a row's forward bits do not depend on its block; both outputs, both
    kinds, are bit for bit those of the single-block call.  The staged rows and targets give the bits of the explicit ones."""
    name, m, rb = "generic4", 8, 192
    ch, X, thetas = setup(native, name, m, seed=2, rates=True)
    d_out = CASES[name][0][-1]
    n = X.shape[0]
    assert n == 517 and -(-n // rb) == 3
    rng = np.random.default_rng(61)
    Y = rng.poisson(3.0, (n, d_out)).astype(np.float32)
    sd, w = sds(m), int_weights(m)
    calls = ({"likelihood": GAUSS, "sd": sd, "weights": w, "probs": P_GAUSS}, {"likelihood": POISSON, "weights": w, "probs": P_POIS})
    whole = [ch.ensemble_predictive(thetas, Y=Y, X=X, **kw) for kw in calls]
    budget = m * d_out * rb + 7
    assert max(64, budget // (m * d_out) // 64 * 64) == rb
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    cut = [ch.ensemble_predictive(thetas, Y=Y, X=X, **kw) for kw in calls]
    ch.set_data(X, Y)
    staged = [ch.ensemble_predictive(thetas, which=0, cdf=True, **kw) for kw in calls]
    monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
    for a, b, c in zip(whole, cut, staged):
        for x, y, z in zip(a, b, c):
            if x is None:
                assert y is None and z is None
            else:
                assert np.array_equal(x.view(np.uint64), y.view(np.uint64)) and np.array_equal(x.view(np.uint64), z.view(np.uint64))
    assert whole[1][2] is not None and whole[0][2] is None
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------ probabilities
def test_more_probabilities_than_one_register_group(native):
    """19 probabilities run as groups of 4, 4, 4, 4 and 3: each agrees bit for bit with a call of its own, and they are monotone"""
    m = 9
    ch, X, thetas = setup(native, "generic4", m, seed=3, rates=True)
    sd, w = sds(m), int_weights(m)
    probs = [(k + 0.37) / 19 for k in range(19)]
    for kw in ({"likelihood": GAUSS, "sd": sd, "weights": w}, {"likelihood": POISSON, "weights": w}):
        q = ch.ensemble_predictive(thetas, probs=probs, X=X, **kw)[0]
        assert q.shape == (19, 4, X.shape[0]) and np.all(np.diff(q, axis=0) >= 0)
        for j, p in enumerate(probs):
            one = ch.ensemble_predictive(thetas, probs=[p], X=X, **kw)[0]
            assert np.array_equal(one[0].view(np.uint64), q[j].view(np.uint64)), (kw["likelihood"], j)
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_usable(native):
    dp = C.POINTER(C.c_double)
    ch, X, thetas = setup(native, "narrow", 4)
    n, Pn = X.shape[0], thetas.shape[1]
    lib, p = native.lib, native._p
    Y = np.ones((n, 1), dtype=np.float32)
    before = ch.forward_many(thetas, X=X)
    qo, Fo, Bo = np.full((65, 1, n), 7.0), np.full((1, n), 7.0), np.full((1, n), 7.0)

    def call(probs=(0.5,), n_probs=None, w=None, lik=GAUSS, sd=None, probs_null=False, q=True, cdf=False, below=False, X_=X, Y_=Y, n_=n,
             which=1, stride=Pn, m=4):
        pr = np.asarray(probs, dtype=np.float64)
        return lib.tbnn_ensemble_predictive(ch._h, p(thetas), m, stride, lik, p(sd), p(w), which, p(X_), p(Y_), n_,
                                            None if probs_null else pr.ctypes.data_as(dp), len(pr) if n_probs is None else n_probs,
                                            qo.ctypes.data_as(dp) if q else None, Fo.ctypes.data_as(dp) if cdf else None,
                                            Bo.ctypes.data_as(dp) if below else None)

    f32 = lambda *v: np.array(v, dtype=np.float32)
    err = lambda: lib.tbnn_last_error().decode()
    assert call(q=False) < 0 and "both null" in err()
    assert call(probs_null=True) < 0 and "null probs" in err()
    assert call(cdf=True, Y_=None) < 0 and "without their targets" in err()
    assert call(below=True, lik=POISSON) < 0 and "without cdf_out" in err()
    assert call(cdf=True, below=True) < 0 and "TBNN_LIK_POISSON" in err()
    assert call(n_probs=0) < 0 and "n_probs" in err()
    assert call(probs=[0.5] * 65) < 0 and "n_probs" in err()
    for bad in (0.0, 1.0, -0.25, 1.5, np.nan):
        assert call(probs=(0.5, bad)) < 0 and "not in (0, 1)" in err(), bad
    assert call(lik=native.LIK_BERNOULLI) < 0 and "tbnn_ensemble_moments" in err()
    assert call(lik=native.LIK_CATEGORICAL) < 0 and "tbnn_ensemble_moments" in err()
    assert call(lik=4) < 0 and "unknown likelihood" in err()
    assert call(lik=7) < 0 and "unknown likelihood" in err()
    assert call(w=f32(1, -1, 1, 1)) < 0 and "negative" in err()
    assert call(w=f32(0, 0, 0, 0)) < 0 and "all weights are zero" in err()
    assert call(w=f32(1, np.nan, 1, 1)) < 0 and "not finite" in err()
    assert call(sd=f32(1, np.nan, 1, 1)) < 0 and "not a number" in err()
    assert call(stride=Pn - 1) < 0 and "theta_stride < P" in err()
    assert call(m=0) < 0 and "m < 1" in err()
    assert call(X_=None, n_=0, which=1) < 0 and "tbnn_set_validation has not been called" in err()
    assert call(X_=None, n_=0, which=2) < 0 and "which must be" in err()
    ch.set_data(X, Y)
    assert call(cdf=True, X_=None, Y_=Y, n_=n - 1, which=0) < 0 and "does not match" in err()
    assert np.all(qo == 7.0) and np.all(Fo == 7.0) and np.all(Bo == 7.0)          # nothing written
    # m d_out 64 > 2^28 is refused before anything is staged (the thetas are not read)
    assert call(m=(1 << 22) + 1) < 0 and "block budget" in err()
    with pytest.raises(native.TbnnError, match="not in"):
        ch.ensemble_predictive(thetas, probs=[1.0], X=X)
    with pytest.raises(native.TbnnError, match="tbnn_ensemble_moments"):
        ch.ensemble_predictive(thetas, probs=[0.5], X=X, likelihood=native.LIK_BERNOULLI)
    with pytest.raises(ValueError, match="targets"):
        ch.ensemble_predictive(thetas, X=X, cdf=True)
    assert call(probs=[(k + 0.5) / 64 for k in range(64)], cdf=True) == 0      # 64 probabilities, and both outputs at once
    assert call(q=False, probs_null=True, cdf=True, below=True, lik=POISSON, n_probs=2 ** 31 - 1) == 0     # the CDF alone: probs and n_probs are not read
    assert not np.any(qo[:64] == 7.0) and not np.any(Fo == 7.0) and np.all(qo[64] == 7.0)
    assert np.array_equal(ch.forward_many(thetas, X=X), before)
    ch.close()


# ---------------------------------------------------------------------------------------------------------------- predictor, end to end
def test_predictor_end_to_end(tmp_path, monkeypatch, native):
    """a small noisy regression trained for a few epochs under a GaussianLikelihood whose sd is sampled: the predictive interval is
    ordered, contains the credible interval of the network's output, and covers more of the training targets than it; the PIT values lie in
    [0, 1] and are the mixture CDF of the saved networks with their saved sd's"""
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.likelihood import GaussianLikelihood
    from tensorbnn_amd.network import network
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(71)
    X = rng.uniform(-2, 2, (300, 1)).astype(np.float32)
    Y = (np.sin(2 * X) + 0.3 * rng.standard_normal(X.shape)).astype(np.float32)
    net = network(np.float32, 1, X, Y, X[:50], Y[:50])
    net.add(DenseLayer(1, 16, seed=1000)); net.add(Tanh())
    net.add(DenseLayer(16, 16, seed=2000)); net.add(Tanh())
    net.add(DenseLayer(16, 1, seed=3000))
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    net.train(30, 2, GaussianLikelihood(sd=0.5), folderName="reg", networksPerFile=1, verbose=False)
    p = predictor(str(tmp_path / "reg") + "/", likelihood=GaussianLikelihood(sd=0.5))
    m = p.numNetworks
    assert m >= 4 and len(p.hypers) == m
    lower, median, upper = p.predictiveInterval(X, level=0.9)
    assert lower.shape == median.shape == upper.shape == (1, 300)
    assert np.all(lower < median) and np.all(median < upper)
    q = p.predictiveQuantiles(X, [0.05, 0.5, 0.95])
    assert np.array_equal(q[0], lower) and np.array_equal(q[1], median) and np.array_equal(q[2], upper)
    assert np.array_equal(p.predictiveQuantiles(X, 0.5), median)
    f = np.array(p.predict(X))
    sd = np.array([np.float32(h[-1]) for h in p.hypers], dtype=np.float32)
    check_gauss_quantiles("predictor", q, [0.05, 0.5, 0.95], f, sd, None)
    c_lo, _c_med, c_hi = p.predictInterval(X, level=0.9)
    assert np.all(lower <= c_lo) and np.all(c_hi <= upper)                               # the noise only widens the interval
    yt = Y.T.astype(np.float64)
    inside_pred, inside_cred = np.mean((yt >= lower) & (yt <= upper)), np.mean((yt >= c_lo) & (yt <= c_hi))
    print(f"[predictive] predictor: {m} networks, sd {clip_sd(sd).min():.3f} .. {clip_sd(sd).max():.3f}; share of the training targets inside "
          f"the 90 % predictive interval {inside_pred:.3f}, inside the credible interval {inside_cred:.3f}")
    assert inside_pred > inside_cred
    pit = p.predictiveCDF(X, Y)
    assert pit.shape == (1, 300) and np.all((pit >= 0) & (pit <= 1))
    assert np.all(np.abs(pit - F_gauss(yt, f, sd, None)) <= T(m, GAUSS))
    # every second network, reweighted and de-normalised on the host
    w = np.arange(1, len(range(0, m, 2)) + 1, dtype=np.float32)
    q2 = p.predictiveQuantiles(X, [0.25, 0.75], n=2, weights=w, sd=2.0, mean=0.5)
    raw = p._chain.ensemble_predictive(np.stack(p.vectors[::2]), probs=[0.25, 0.75], X=X, likelihood=native.LIK_GAUSSIAN, sd=sd[::2], weights=w)[0]
    assert np.array_equal(q2, raw * 2.0 + 0.5)
    check_gauss_quantiles("predictor, every second network", raw, [0.25, 0.75], f[::2], sd[::2], w)
