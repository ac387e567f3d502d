"""GPU: the predictive distribution of a new COUNT under the negative binomial (tbnn_ensemble_predictive with TBNN_LIK_NEG_BINOMIAL,
predictor.predictiveQuantiles / predictiveInterval / predictiveCDF / predictMoments(countVariance=True)) against fp64 SciPy applied to the
fp32 predictions Chain.forward_many returns for the same thetas and rows -- the helpers, shapes and bound of tests/test_gpu_predictive.py.
Every test here fails without the feature (the likelihood code is refused).

The mixture: F(k) = sum_i (w_i / W) I_{q_i}(r, k + 1) for integer k >= 0 (0 below), q_i = r / (r + exp(f_i)) = sigmoid(log r - f_i), I the
regularised incomplete beta function -- on the device a continued fraction in fp64 (csrc/kernels_ensemble.hpp ens_betainc), here
scipy.special.betainc.  The bound is test_gpu_predictive's with this term's figure:  T(m) = (m + 8) U + 4 NB_FIG.

NB_FIG is the largest |device - SciPy| of one term on test_term_accuracy_on_a_grid's grid (40,028 elements: r in {0.3, 3.7, 50, 1e4}, rates
from 0.05 to 2^20, k within 7 sd of the mean, far from it, at 0 and at the ceiling 2^20), measured on an MI355X; the test prints it on every
run and asserts 4 x the recorded value, the margin for inputs the grid misses, and 1e-9 whatever was recorded.  SciPy agrees with 40-digit
mpmath to 1e-15 at points up to k = 2^20, so the figure (1.608e-11, at r = 0.3, rate 218,651, k = 2^20) is the device's: it comes from the continued fraction's first step
1 - (a + b) x / (a + 1), which cancels to 2 / (a + b) of itself next to the switch of sides (a + b ~ 1e6: 5e-11 relative), not from the
prefactor, which is formed without cancellation (3e-16 against mpmath).

Quantiles are integers and must equal the reference's smallest k with F(k) >= p -- the k with F_ref(k - 1) < p <= F_ref(k), F_ref being
monotone -- except where the reference's own decision is within T of p (min(|F_ref(k*) - p|, |F_ref(k* - 1) - p|) < T), where k* +- 1 is
accepted, for at most 0.1 % of a test's elements (the count is printed).  nb_quantile_ref states the search itself (outward, then
bisection); check_nb_quantiles uses the two-sided characterisation, which is the same statement at 2 evaluations of F_ref per probability,
and test_quantile_characterisation_equals_the_search runs both.  The reference's count of such near-ties on these inputs, evaluated on the
CPU with the oracle's forward for the same thetas before any GPU run: 0 at every (case, m, weights) with the probabilities
[0.03, 0.41, 0.97] and the seeds used here."""
import math

import numpy as np
import pytest
import scipy.special as sp

from test_gpu_ensemble import CASES, problem, make_chain
from test_gpu_predictive import U, int_weights, mix, setup
from test_gpu_quantiles import ROWS

pytestmark = pytest.mark.gpu

NEGBIN = 10
KMAX = 2.0 ** 20                       # csrc/kernels_ensemble.hpp ENS_NB_MAX: the ceiling on the rate and on k
# the largest |device - SciPy| of one term on test_term_accuracy_on_a_grid's grid, measured on an MI355X (module docstring)
NB_FIG = 1.608e-11
P_NB = [0.03, 0.41, 0.97]
MS = [1, 2, 3, 64, 65, 257]
DISP = {"narrow": 0.5, "mid2": 2.5, "layered10": 30.0, "generic4": 1e4}


def T(m):
    return (m + 8) * U + 4 * NB_FIG


def r64(r):
    """the dispersion as the library holds it: an fp32"""
    return float(np.float32(r))


def nb_terms(k, f, r):
    """I_{q_i}(r, k + 1) per network: k [d_out, n] integer-valued and >= 0, f fp32 [m, d_out, n]"""
    q = sp.expit(math.log(r64(r)) - f.astype(np.float64))
    return sp.betainc(r64(r), np.asarray(k, dtype=np.float64)[None] + 1.0, q)


def F_nb(k, f, w, r):
    """F(k) at integer-valued k [d_out, n]; 0 below 0.  Networks of weight 0 are left out of the sum (they add nothing)"""
    k = np.asarray(k, dtype=np.float64)
    if w is not None:
        keep = np.asarray(w) > 0
        f, w = f[keep], np.asarray(w)[keep]
    return np.where(k < 0, 0.0, mix(nb_terms(np.maximum(k, 0.0), f, r), w))


def nb_quantile_ref(p, f, w, r):
    """the smallest integer k >= 0 with F_nb(k) >= p: a bracket around the components' quantiles in the normal approximation, pushed
    outward until F_nb itself says F(lo) < p <= F(hi) (lo = -1: F = 0), then bisection"""
    lam = np.exp(f.astype(np.float64))
    keep = np.ones(f.shape[0], bool) if w is None else np.asarray(w) > 0
    guess = lam[keep] + sp.ndtri(p) * np.sqrt(lam[keep] + lam[keep] ** 2 / r64(r))
    lo, hi = np.maximum(np.floor(guess.min(axis=0)) - 3.0, -1.0), np.maximum(np.ceil(guess.max(axis=0)) + 3.0, 0.0)
    step = 2.0
    while True:
        up, down = F_nb(hi, f, w, r) < p, (lo >= 0) & (F_nb(lo, f, w, r) >= p)
        if not up.any() and not down.any():
            break
        hi, lo = np.where(up, hi + step, hi), np.where(down, np.maximum(lo - step, -1.0), lo)
        step *= 2
    while np.any(hi - lo > 1):
        mid = np.floor((lo + hi) / 2)
        ge = F_nb(mid, f, w, r) >= p
        act = hi - lo > 1
        hi, lo = np.where(act & ge, mid, hi), np.where(act & ~ge, mid, lo)
    return hi


def check_nb_quantiles(tag, q, probs, f, w, r):
    """q[j] is the reference's smallest k with F_ref(k) >= p_j: F_ref(q - 1) < p <= F_ref(q).  Where it is not, k* is q + 1 (F_ref(q) < p
    <= F_ref(q + 1)) or q - 1 (F_ref(q - 2) < p <= F_ref(q - 1)) and the reference's decision there is within T of p; anything else fails"""
    m = f.shape[0]
    t = T(m)
    used = total = 0
    for j, p in enumerate(probs):
        qj = q[j]
        assert np.all(np.isfinite(qj)) and np.array_equal(qj, np.floor(qj)) and np.all(qj >= 0), (tag, p)
        at, below = F_nb(qj, f, w, r), F_nb(qj - 1, f, w, r)
        exact = (below < p) & (at >= p)
        low = ~exact & (at < p)                      # the device stopped one short: k* = q + 1, and F_ref(k* - 1) = at is within T of p
        high = ~exact & ~low                         # one too far: k* = q - 1, and F_ref(k*) = below is within T of p
        ok = exact.copy()
        if low.any():
            ok |= low & (p - at < t) & (F_nb(qj + 1, f, w, r) >= p)
        if high.any():
            ok |= high & (below - p < t) & (F_nb(qj - 2, f, w, r) < p)
        assert ok.all(), (tag, p, qj[~ok][:5], at[~ok][:5], below[~ok][:5])
        used += int((~exact).sum()); total += exact.size
    print(f"[negbin predictive] {tag}: m={m} quantiles, {used} of {total} elements within T of a tie took the exception")
    assert used <= 0.001 * total, (tag, used, total)
    order = np.argsort(probs)
    assert np.all(np.diff(q[order], axis=0) >= 0), tag       # monotone in p


def near_ties(probs, f, w, r):
    """the reference's own count of elements whose decision is within T of p (the condition on the exception's 0.1 % cap)"""
    t, cnt = T(f.shape[0]), 0
    for p in probs:
        ks = nb_quantile_ref(p, f, w, r)
        cnt += int((np.minimum(np.abs(F_nb(ks, f, w, r) - p), np.abs(F_nb(ks - 1, f, w, r) - p)) < t).sum())
    return cnt


def nb_setup(native, name, m, seed=0):
    ch, X, thetas = setup(native, name, m, seed=seed, rates=True)
    ch.set_lik_df(DISP[name])                    # (the handles of tests/test_gpu_ensemble.py are Gaussian ones: r comes from the setter)
    return ch, X, thetas, DISP[name]


# --------------------------------------------------------------------------------------------- the per-term figure, measured on a grid
def grid_counts(lam, r, rng):
    """k within 7 sd of the mean, every 5th far from it (2^U(0, 20)), every 11th small, then 0, the ceiling and 31"""
    n = lam.size
    k = np.floor(lam + np.sqrt(lam + lam * lam / r) * rng.uniform(-7, 7, n))
    k[::5] = np.floor(2.0 ** rng.uniform(0, 20, len(k[::5])))
    k[::11] = rng.integers(0, 40, len(k[::11]))
    k = np.clip(k, 0, KMAX)
    k[:3] = [0, KMAX, 31]
    return k


def test_term_accuracy_on_a_grid(native):
    """one network through the CDF entry point, 10,007 rows at each of four dispersions: the device's I against scipy.special.betainc at
    rates from 0.05 to 2^20 and counts 0 .. 2^20.  Prints the largest difference -- NB_FIG records it -- and asserts 4 x the recorded
    figure, and 1e-9 whatever was recorded."""
    name = "narrow"
    X, thetas = problem(name, 1, seed=21, n=10007)
    ch = make_chain(native, name)
    n = X.shape[0]
    f0 = ch.forward_many(thetas, X=X)[0, 0].astype(np.float64)
    # log-rates from log 0.05 to log 2^20: the last layer rescaled (theta ends with its 50 weights and its bias)
    alpha = (math.log(0.999 * KMAX) - math.log(0.05)) / (f0.max() - f0.min())
    th = thetas.copy()
    th[0, -51:] = (th[0, -51:].astype(np.float64) * alpha).astype(np.float32)
    th[0, -1] += np.float32(math.log(0.05) - alpha * f0.min())
    fp = ch.forward_many(th, X=X)
    lam = np.exp(fp[0, 0].astype(np.float64))
    inside = lam <= KMAX
    assert lam.min() < 0.1 and 2.0 ** 19 < lam.max() and inside.all()
    rng = np.random.default_rng(22)
    worst, where, elements = 0.0, None, 0
    for r in (0.3, 3.7, 50.0, 1e4):
        ch.set_lik_df(r)
        k = grid_counts(lam, r64(r), rng)
        Y = k.astype(np.float32)[:, None]
        assert np.array_equal(Y[:, 0].astype(np.float64), k)
        _q, F, Fb = ch.ensemble_predictive(th, Y=Y, X=X, likelihood=NEGBIN)
        assert np.array_equal(np.isnan(F[0]), ~inside) and np.array_equal(np.isnan(Fb[0]), ~inside)
        ref_at = nb_terms(k[None], fp, r)[0, 0]
        ref_below = np.where(k >= 1, nb_terms(np.maximum(k - 1, 0.0)[None], fp, r)[0, 0], 0.0)
        e = np.maximum(np.abs(F[0] - ref_at), np.abs(Fb[0] - ref_below))[inside]
        i = int(np.argmax(e))
        print(f"[negbin predictive] r = {r:g}: max |dev - betainc| {e.max():.3e} at rate {lam[inside][i]:.6g}, k {k[inside][i]:.0f}")
        if e.max() > worst:
            worst, where = float(e.max()), (r, float(lam[inside][i]), float(k[inside][i]))
        elements += int(inside.sum())
        assert np.all((F[0][inside] >= 0) & (F[0][inside] <= 1)) and np.all(Fb[0][inside] <= F[0][inside])
    print(f"[negbin predictive] per-term figure over {elements} elements: max |dev - betainc| {worst:.3e} at (r, rate, k) = {where} (NB_FIG {NB_FIG:.1e})")
    assert worst <= 1e-9
    assert worst <= 4 * NB_FIG
    ch.close()


# ------------------------------------------------------------------------------------------------------------------- every shape, every m
@pytest.mark.parametrize("name,m", [(n_, m_) for n_ in ROWS for m_ in MS])
def test_cdf_and_quantiles_against_scipy(native, name, m):
    """m = 1, 2 (no interior), 3, the wavefront size and one more, 257; d_out 1, 2, 4 and 10 over the cases, r 0.5, 2.5, 30 and 1e4; network
    2 a copy of network 0; log-rates around 1.5; equal weights and integer weights with zeros; targets read at floor(y)"""
    d_out = CASES[name][0][-1]
    rng = np.random.default_rng(31)
    ch, X, thetas, r = nb_setup(native, name, m)
    n = X.shape[0]
    f = ch.forward_many(thetas, X=X)
    if m > 2:
        assert np.array_equal(f[0], f[2])
    lam0 = np.exp(f[0].astype(np.float64))
    assert np.exp(f.astype(np.float64)).max() < KMAX
    Yp = rng.poisson(rng.gamma(r64(r), lam0 / r64(r))).T.astype(np.float32)
    Yp[::7] += np.float32(0.5)                                 # read at floor(y)
    Yp[0] = 0.0
    for tag, w in (("equal", None), ("integer weights", int_weights(m))):
        q, F, Fb = ch.ensemble_predictive(thetas, probs=P_NB, Y=Yp, X=X, likelihood=NEGBIN, weights=w)
        assert q.shape == (3, d_out, n) and F.shape == Fb.shape == (d_out, n) and q.dtype == F.dtype == Fb.dtype == np.float64
        k = np.floor(Yp.T.astype(np.float64))
        e_at, e_below = np.abs(F - F_nb(k, f, w, r)), np.abs(Fb - F_nb(k - 1, f, w, r))
        print(f"[negbin predictive] {name} {tag}: m={m} r={r:g} CDF err max {e_at.max():.3e}, below {e_below.max():.3e} (T {T(m):.3e})")
        assert np.all(e_at <= T(m)) and np.all(e_below <= T(m))
        assert not Fb[:, 0].any() and np.all(Fb <= F)
        check_nb_quantiles(f"{name} {tag}", q, P_NB, f, w, r)
    again = ch.ensemble_predictive(thetas, probs=P_NB, Y=Yp, X=X, likelihood=NEGBIN, weights=w)
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(again, (q, F, Fb)))
    ch.close()


def test_quantile_characterisation_equals_the_search(native):
    """the reference's search (nb_quantile_ref) and the two-sided characterisation check_nb_quantiles asserts name the same k, and the
    device returns it: m = 3 and m = 65 on the four-output case; the reference's own count of near-ties is printed"""
    for m in (3, 65):
        ch, X, thetas, r = nb_setup(native, "generic4", m, seed=5)
        f = ch.forward_many(thetas, X=X)
        w = int_weights(m)
        q = ch.ensemble_predictive(thetas, probs=P_NB, X=X, likelihood=NEGBIN, weights=w)[0]
        ties = near_ties(P_NB, f, w, r)
        print(f"[negbin predictive] m={m}: the reference's own near-ties: {ties} of {q.size}")
        assert ties <= 0.001 * q.size
        for j, p in enumerate(P_NB):
            ks = nb_quantile_ref(p, f, w, r)
            assert np.all((F_nb(ks - 1, f, w, r) < p) & (F_nb(ks, f, w, r) >= p))
            if ties == 0:
                assert np.array_equal(q[j], ks)
        ch.close()


# --------------------------------------------------------------------------------------------------------------------------- row blocks
def test_row_blocks_and_the_handle_s_own_dispersion(native, monkeypatch):
    """517 rows in blocks of 192 (three blocks, the last of 133 rows), the staged rows and targets, and a negative-binomial handle whose r
    is its descriptor's: all three outputs bit for bit those of the single-block call on the Gaussian handle with the setter"""
    name, m, rb = "generic4", 8, 192
    ch, X, thetas, r = nb_setup(native, name, m, seed=2)
    dims = CASES[name][0]
    d_out = dims[-1]
    n = X.shape[0]
    assert n == 517 and -(-n // rb) == 3
    Y = np.random.default_rng(61).poisson(3.0, (n, d_out)).astype(np.float32)
    kw = {"likelihood": NEGBIN, "weights": int_weights(m), "probs": P_NB}
    whole = ch.ensemble_predictive(thetas, Y=Y, X=X, **kw)
    budget = m * d_out * rb + 7
    assert max(64, budget // (m * d_out) // 64 * 64) == rb
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    cut = ch.ensemble_predictive(thetas, Y=Y, X=X, **kw)
    ch.set_data(X, Y)
    staged = ch.ensemble_predictive(thetas, which=0, cdf=True, **kw)
    monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
    own = native.Chain([(dims[i], dims[i + 1], native.ACT_TANH if i < len(dims) - 2 else native.ACT_NONE, 0) for i in range(len(dims) - 1)],
                       likelihood=NEGBIN, lik_df=r, kernel=native.KERNEL_GENERIC)
    mine = own.ensemble_predictive(thetas, Y=Y, X=X, weights=kw["weights"], probs=P_NB)          # likelihood None: the chain's own
    own.close()
    for x, y, z, v in zip(whole, cut, staged, mine):
        assert x is not None
        for other in (y, z, v):
            assert np.array_equal(x.view(np.uint64), other.view(np.uint64))
    # the CDF alone, and the quantiles alone
    assert np.array_equal(ch.ensemble_predictive(thetas, Y=Y, X=X, likelihood=NEGBIN, weights=kw["weights"])[1], whole[1])
    only_q = ch.ensemble_predictive(thetas, X=X, **kw)
    assert only_q[1] is None and only_q[2] is None and np.array_equal(only_q[0], whole[0])
    ch.close()


# ------------------------------------------------------------------------------------------------------------------ NaN and the ceilings
def test_nan_and_ceilings_stay_in_their_element(native):
    """a NaN input row makes that row's predictions NaN under every network; a row scaled up drives some counted network's rate past 2^20:
    NaN in those elements only, in all outputs; a target above 2^20 makes that element's CDF and CDF-below NaN and leaves its quantiles; a
    probability whose quantile lies past k = 2^20 is NaN alone, the others of its element are numbers"""
    name, m = "narrow", 5
    ch, X0, thetas, r = nb_setup(native, name, m, seed=51)
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
        big_el = (lam[counts] > KMAX).any(axis=0)
        if big_el[0, 300]:
            break
    assert nan_el.sum() == 1 and nan_el[0, 7] and big_el.sum() == 1 and big_el[0, 300] and np.isfinite(f[:, 0, 300]).all()
    Y = np.ones((X.shape[0], 1), dtype=np.float32)
    Y[11, 0] = np.float32(KMAX + 2.0)                         # past the ceiling on k
    Y[12, 0] = np.float32(KMAX)                               # at it: a number
    Y[13, 0] = np.inf
    q, F, Fb = ch.ensemble_predictive(thetas, probs=P_NB, Y=Y, X=X, likelihood=NEGBIN, weights=w)
    bad = nan_el | big_el
    for a in (q[0], q[1], q[2]):
        assert np.array_equal(np.isnan(a), bad)
    bad_y = bad.copy()
    bad_y[0, 11] = bad_y[0, 13] = True
    for a in (F, Fb):
        assert np.array_equal(np.isnan(a), bad_y)
    assert F[0, 12] == 1.0 or abs(F[0, 12] - 1.0) <= T(m)
    ch.close()
    # one network at a constant rate of 9e5 and r = 0.3: the 0.97 quantile lies past 2^20, the 0.03 and 0.41 quantiles do not
    ch, X, th = setup(native, name, 1, seed=52)
    ch.set_lik_df(0.3)
    th = th.copy()
    th[0, -51:-1] = 0.0
    th[0, -1] = np.float32(math.log(9e5))
    f = ch.forward_many(th, X=X)
    assert np.all(f == f[0, 0, 0]) and np.exp(float(f[0, 0, 0])) < KMAX
    q = ch.ensemble_predictive(th, probs=P_NB, X=X, likelihood=NEGBIN)[0]
    assert F_nb(np.full((1, 1), KMAX), f[:, :, :1], None, 0.3)[0, 0] < 0.97
    assert np.all(np.isnan(q[2])) and np.all(np.isfinite(q[0])) and np.all(np.isfinite(q[1])) and np.all(q[1] <= KMAX)
    check_nb_quantiles("constant rate", q[:2], P_NB[:2], f, None, 0.3)
    ch.close()


# ---------------------------------------------------------------------------------------------------------------- predictor, end to end
def test_predictor_end_to_end(tmp_path, monkeypatch, native):
    """over-dispersed counts trained for a few epochs under NegativeBinomialLikelihood(dispersion=2): the predictive interval is ordered
    and integer, contains the credible interval of the rate, the PIT pair is the mixture CDF of the saved networks at y - 1 and y, and
    countVariance adds E[rate^2] / r to the Poisson total"""
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.likelihood import NegativeBinomialLikelihood
    from tensorbnn_amd.network import network
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(71)
    r = 2.0
    X = rng.uniform(-2, 2, (300, 1)).astype(np.float32)
    mu = np.exp(1.5 + np.sin(2 * X.astype(np.float64)))
    Y = rng.poisson(rng.gamma(r, mu / r)).astype(np.float32)
    lik = NegativeBinomialLikelihood(dispersion=r)
    net = network(np.float32, 1, X, Y, X[:50], Y[:50])
    net.add(DenseLayer(1, 16, seed=1000)); net.add(Tanh())
    net.add(DenseLayer(16, 16, seed=2000)); net.add(Tanh())
    net.add(DenseLayer(16, 1, seed=3000))
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    net.train(30, 2, lik, folderName="nb", networksPerFile=1, verbose=False)
    assert "neg-binomial" in net._chain.kernel_name, net._chain.kernel_name
    p = predictor(str(tmp_path / "nb") + "/", likelihood=lik)
    m = p.numNetworks
    assert m >= 4
    lower, median, upper = p.predictiveInterval(X, level=0.9)
    assert lower.shape == median.shape == upper.shape == (1, 300)
    assert np.all(lower <= median) and np.all(median <= upper) and np.all(lower < upper)
    q = p.predictiveQuantiles(X, [0.05, 0.5, 0.95])
    assert np.array_equal(q[0], lower) and np.array_equal(q[1], median) and np.array_equal(q[2], upper)
    assert np.array_equal(p.predictiveQuantiles(X, 0.5), median)
    f = np.array(p.predict(X))
    check_nb_quantiles("predictor", q, [0.05, 0.5, 0.95], f, None, r)
    c_lo, _c_med, c_hi = p.predictInterval(X, level=0.9)                                # the rate's credible interval (exp by default)
    assert np.all(lower <= c_lo) and np.all(np.ceil(c_hi) <= upper + 1)
    below, at = p.predictiveCDF(X, Y)
    yt = Y.T.astype(np.float64)
    assert np.all(np.abs(at - F_nb(yt, f, None, r)) <= T(m)) and np.all(np.abs(below - F_nb(yt - 1, f, None, r)) <= T(m))
    inside = float(np.mean((yt >= lower) & (yt <= upper)))
    print(f"[negbin predictive] predictor: {m} networks; share of the training targets inside the 90 % predictive interval {inside:.3f}")
    mean, var = p.predictMoments(X)
    mean2, tot = p.predictMoments(X, countVariance=True)
    assert np.array_equal(mean, mean2) and np.array_equal(tot, mean + var + (var + mean * mean) / r) and np.all(tot > mean + var)
    # every second network, reweighted; counts take no de-normalisation
    w = np.arange(1, len(range(0, m, 2)) + 1, dtype=np.float32)
    q2 = p.predictiveQuantiles(X, [0.25, 0.75], n=2, weights=w)
    check_nb_quantiles("predictor, every second network", q2, [0.25, 0.75], f[::2], w, r)
    with pytest.raises(ValueError, match="NegativeBinomialLikelihood"):
        p.predictiveQuantiles(X, [0.5], sd=2.0)
    per_net, per_row = p.logPredictiveDensity(X, Y)
    assert per_net.shape == (m,) and np.all(np.isfinite(per_row))
