"""GPU: Pareto-smoothed leave-one-out cross-validation and WAIC over an ensemble (tbnn_ensemble_loo, Chain.ensemble_loo, predictor.loo / waic
/ compareLoo) against tests/psis_ref.py, the fp64 NumPy restatement of the definition in include/tbnn.h.  Every test here fails without the
entry point (it does not exist before this module's feature).

Comparison rule.  The device's own `pointwise` matrix l[m][rows] is fed to psis_ref, so both sides smooth the same doubles: which values
form the tail and whether a row is smoothed at all are comparisons of identical values, and +inf and NaN must stand in the same places.
What is left differs by libm against the device's exp / log / log1p / expm1 and by the order of fp64 sums (the device carries the fit's
weights as running sums, NumPy forms them after a log-sum-exp).  MEASURED is the largest such difference over all cases of this module on an
MI355X -- absolute for pareto_k and p_waic, relative for elpd_loo and lppd: 2.787e-11, a k of 62 in test_predictor_loo_waic_compare's
categorical rows when the whole suite runs (there the predictor's forward kernel is the run-time mid-width one; 2.8e-14 on the layered
kernel of a run of this module alone).  Those rows' l_i lie within a few fp32 quanta of 0, about 1e-7, so the definition's
y_j = exp(v) - exp(c) cancels seven digits of an ulp's difference between the two exp.  Every other case stays below 2.180e-13 (the k of one
row of test_ties' pairs of equal networks); p_waic: 0.0; elpd_loo and lppd: 8.2e-14 at the most.  The bound is 16 x the largest, the margin tests/test_gpu_diagnostics.py
gives the same kind of gap, and never above 1e-8: a larger gap would mean a formula differs, not rounding.  DESIGN.md section 4.6 records
the figure.

The matrix itself is checked twice: against the package's terms in fp64 from Chain.forward_many's predictions under the error model of
tests/test_gpu_ensemble.py (Poisson: that of tests/test_gpu_poisson.py), and against the existing entry point bit for bit -- lppd is
tbnn_ensemble_loglik's lppd_rows, and the matrix summed over the rows in the order k_ens_loglik sums them (the wavefront's shuffle tree, the
four waves, the workgroups) is its per_net."""
import ctypes as C
import math

import numpy as np
import pytest

from psis_ref import psis_ref, tail_length
from test_gpu_diagnostics import gen3_chain, rows_for, walks
from test_gpu_ensemble import CASES, U, layers_for, loglik_terms, make_chain

pytestmark = pytest.mark.gpu

MEASURED = 2.787e-11
TOL = min(16 * MEASURED, 1e-8)
ROWS = 70                                                    # one ragged wavefront
LIK_GAUSSIAN, LIK_FIXED_GAUSSIAN, LIK_BERNOULLI, LIK_CATEGORICAL, LIK_POISSON = 0, 1, 2, 3, 5
KEYS = ("elpd_loo", "pareto_k", "lppd", "p_waic")


def compare(tag, got, r_eff=1.0, keys=KEYS):
    """got: Chain.ensemble_loo(..., pointwise=True).  Prints the figures, then asserts the module docstring's rule for `keys`; returns the
    reference."""
    pw = got["pointwise"]
    ref = psis_ref(pw, r_eff)
    worst = {}
    for key in keys:
        g, w = got[key], ref[key]
        assert g.shape == w.shape == (pw.shape[1],) and g.dtype == np.float64, (tag, key)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, key, "NaN positions")
        assert np.array_equal(np.isposinf(g), np.isposinf(w)) and np.array_equal(np.isneginf(g), np.isneginf(w)), (tag, key, "inf positions")
        fin = np.isfinite(w)
        d = np.abs(g[fin] - w[fin])
        if key in ("elpd_loo", "lppd"):                     # (a reference of exactly 0 -- a row every network predicts with certainty -- is to be met exactly)
            d = np.where(w[fin] != 0, d / np.where(w[fin] != 0, np.abs(w[fin]), 1.0), np.where(d == 0, 0.0, np.inf))
        worst[key] = float(d.max(initial=0.0))
    k = ref["pareto_k"]
    kf = k[np.isfinite(k)]
    print(f"[loo] {tag}: m={pw.shape[0]} M={tail_length(pw.shape[0], r_eff)} rows {pw.shape[1]} (k=inf {int(np.isposinf(k).sum())}, NaN {int(np.isnan(k).sum())}), "
          f"k {kf.min(initial=np.inf):.3f} .. {kf.max(initial=-np.inf):.3f}, diff " + " ".join(f"{key} {worst[key]:.3e}" for key in keys)
          + f" -> largest {max(worst.values()):.3e}")
    assert max(worst.values()) <= TOL, (tag, worst)
    return ref


def device_row_sums(l):
    """l [m, n] summed over the rows as k_ens_loglik sums them: per workgroup of 256 rows the lanes of each wavefront by the tree of wave_sum
    (lane i += lane i + o, o = 32 .. 1; rows past n add 0), the four waves in order, then the workgroups in order"""
    m, n = l.shape
    nblk = -(-n // 256)
    v = np.zeros((m, nblk * 256))
    v[:, :n] = l
    v = v.reshape(m, nblk, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
    w = v[..., 0]
    blk = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    out = np.zeros(m)
    for b in range(nblk):
        out += blk[:, b]
    return out


def check_matrix(tag, ch, got, thetas, X, Y, lik, sd, fixed_sd=0.7):
    """the two checks of the module docstring's last paragraph"""
    pw = got["pointwise"]
    f = ch.forward_many(thetas, X=X)
    if lik == LIK_POISSON:
        from scipy.special import gammaln
        f64 = f.astype(np.float64)
        y = np.asarray(Y, dtype=np.float32).reshape(X.shape[0], -1).T.astype(np.float64)[None]
        t1, t2, t3 = y * f64, np.exp(f64), gammaln(y + 1.0) + 0 * f64
        l, err = (t1 - t2 - t3).sum(axis=1), (8 * U * (np.abs(t1) + t2 + np.abs(t3))).sum(axis=1)
    else:
        l, err, _mag = loglik_terms(f, Y, lik, sd, fixed_sd)
    tol = err + np.spacing(np.abs(l))
    e = np.abs(pw - l)
    print(f"[loo] {tag}: matrix against the fp64 terms, err max {e.max():.3e}, worst err/tol {np.max(e / tol):.3f}")
    assert np.all(np.isfinite(pw)) and np.all(e <= tol), (tag, float(np.max(e / tol)))
    per_net, rows = ch.ensemble_loglik(thetas, Y=Y, X=X, likelihood=lik, sd=sd)
    assert np.array_equal(got["lppd"].view(np.uint64), rows.view(np.uint64)), tag
    assert np.array_equal(device_row_sums(pw).view(np.uint64), per_net.view(np.uint64)), tag


def targets_for(f, lik, rng):
    """f [m, d_out, n] -> Y [n, d_out] the first network roughly fits"""
    n, d_out = f.shape[2], f.shape[1]
    if lik == LIK_BERNOULLI:
        return (rng.random((n, d_out)) < f[0].T).astype(np.float32)
    if lik == LIK_CATEGORICAL:
        return np.eye(d_out, dtype=np.float32)[np.argmax(f[0].T + rng.gumbel(size=(n, d_out)), axis=1)]
    if lik == LIK_POISSON:
        return rng.poisson(np.exp(np.clip(f[0].T.astype(np.float64), -3.0, 3.0))).astype(np.float32)
    return (f[0].T + 0.5 * rng.standard_normal((n, d_out))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name,m,r_eff,lik,per_net_sd", [
    ("narrow", 20, 1.0, LIK_FIXED_GAUSSIAN, False), ("narrow", 25, 1.0, LIK_FIXED_GAUSSIAN, False), ("narrow", 64, 1.0, LIK_FIXED_GAUSSIAN, False),
    ("narrow", 256, 1.0, LIK_FIXED_GAUSSIAN, False), ("narrow", 256, 0.5, LIK_FIXED_GAUSSIAN, False), ("tall", 64, 1.0, LIK_BERNOULLI, False),
    ("gen3", 64, 1.0, LIK_CATEGORICAL, False), ("narrow", 64, 1.0, LIK_POISSON, False), ("mid2", 64, 1.0, LIK_GAUSSIAN, True)])
def test_against_the_restatement(native, name, m, r_eff, lik, per_net_sd):
    """m = 20: M = 4, no smoothing; 25: the smallest tail that is smoothed; 64: M = 13 from 0.2 m; 256: M = 48 from 3 sqrt m, and 52 at
    r_eff = 0.5.  The fixed Gaussian on the narrow MFMA kernels, Bernoulli on the tall family, the categorical likelihood over three outputs
    of the generic kernel, Poisson with count targets, per-network sd over two outputs.  The thetas are small walks around one base, so the
    ratios have a real but light tail.  70 rows."""
    ch = gen3_chain(native) if name == "gen3" else make_chain(native, name)
    X = rows_for(name)
    thetas = walks(ch.P, 1, m, seed=m + lik)
    rng = np.random.default_rng(m)
    Y = targets_for(ch.forward_many(thetas, X=X), lik, rng)
    sd = (0.4 + rng.random(m)).astype(np.float32) if per_net_sd else None
    got = ch.ensemble_loo(thetas, Y=Y, X=X, likelihood=lik, sd=sd, r_eff=r_eff, pointwise=True)
    assert got["pointwise"].shape == (m, ROWS)
    ref = compare(f"{name} lik {lik} r_eff {r_eff}", got, r_eff)
    check_matrix(f"{name} lik {lik}", ch, got, thetas, X, Y, lik, sd)
    assert np.all(np.isposinf(ref["pareto_k"])) if m == 20 else np.all(np.isfinite(ref["pareto_k"]))
    assert np.all(got["elpd_loo"] <= got["lppd"]) and np.all(got["p_waic"] >= 0)
    # staged rows and targets give the same bits, and so does leaving the matrix out
    ch.set_data(X, Y)
    staged = ch.ensemble_loo(thetas, which=0, likelihood=lik, sd=sd, r_eff=r_eff)
    assert "pointwise" not in staged
    waic_only = ch.ensemble_loo(thetas, Y=Y, X=X, likelihood=lik, sd=sd, psis=False)               # no smoothing kernel: the other two unchanged
    assert sorted(waic_only) == ["lppd", "p_waic"]
    for key in waic_only:
        assert np.array_equal(waic_only[key].view(np.uint64), got[key].view(np.uint64)), key
    for key in KEYS:
        assert np.array_equal(staged[key].view(np.uint64), got[key].view(np.uint64)), key
    ch.close()


def test_outliers_span_the_range_of_k(native):
    """256 networks on a SEGMENT of parameter space (a bounded spread of predictions: short tails, k < 0) and targets planted from 1/4 to 16
    noise-sd's away in seven rows (the further, the heavier the tail of the ratios): both ends of the scale occur"""
    ch = make_chain(native, "narrow")
    X = rows_for("narrow", seed=2)
    rng = np.random.default_rng(21)
    base, direction = rng.standard_normal(ch.P) * 0.35, rng.standard_normal(ch.P)
    thetas = (base + 0.03 * rng.uniform(-1.0, 1.0, (256, 1)) * direction).astype(np.float32)
    Y = targets_for(ch.forward_many(thetas, X=X), LIK_FIXED_GAUSSIAN, rng)
    Y[3:70:10, 0] += (0.7 * 2.0 ** np.arange(-2, 5)).astype(np.float32)
    got = ch.ensemble_loo(thetas, Y=Y, X=X, pointwise=True)
    ref = compare("planted outliers", got)
    k = ref["pareto_k"]
    print("[loo] planted outliers: k of the planted rows " + " ".join(f"{v:.2f}" for v in k[3:70:10]))
    assert np.all(np.isfinite(k)) and k.min() < 0.0 and k.max() > 0.7
    ch.close()


def test_ties(native):
    """all networks identical: nothing to smooth, k = +inf and elpd_loo = lppd = the row's l (two roundings at |l| + log m: the log-sum-exp
    adds log m and the subtraction takes it off).  Every second network a copy of its neighbour: with M = 13 the pairs straddle the cutoff"""
    ch = make_chain(native, "narrow")
    X = rows_for("narrow", seed=3)
    thetas = walks(ch.P, 1, 64, seed=31)
    Y = targets_for(ch.forward_many(thetas, X=X), LIK_FIXED_GAUSSIAN, np.random.default_rng(32))
    same = np.repeat(thetas[:1], 64, axis=0)
    got = ch.ensemble_loo(same, Y=Y, X=X, pointwise=True)
    compare("identical networks", got)
    l = got["pointwise"][0]
    assert np.all(got["pointwise"] == l) and np.all(np.isposinf(got["pareto_k"]))
    assert np.all(got["p_waic"] <= 2 * (64 * U * np.abs(l)) ** 2)          # the mean of 64 equal values is rounded: up to 64 U |l| from them
    for key in ("elpd_loo", "lppd"):
        assert np.all(np.abs(got[key] - l) <= 2 * U * 2 * (np.abs(l) + math.log(64))), key
    pairs = thetas.copy()
    pairs[1::2] = pairs[0::2]
    got = ch.ensemble_loo(pairs, Y=Y, X=X, pointwise=True)
    assert np.array_equal(got["pointwise"][1::2], got["pointwise"][0::2])
    ref = compare("pairs of equal networks", got)
    assert np.all(np.isfinite(ref["pareto_k"]))
    ch.close()


def test_a_nan_target_undoes_its_row_alone(native):
    ch = make_chain(native, "narrow")
    X = rows_for("narrow", seed=4)
    thetas = walks(ch.P, 1, 64, seed=41)
    Y = targets_for(ch.forward_many(thetas, X=X), LIK_FIXED_GAUSSIAN, np.random.default_rng(42))
    clean = ch.ensemble_loo(thetas, Y=Y, X=X, pointwise=True)
    Y2 = Y.copy()
    Y2[5, 0] = np.nan
    got = ch.ensemble_loo(thetas, Y=Y2, X=X, pointwise=True)
    compare("a NaN target", got)
    others = np.arange(ROWS) != 5
    for key in KEYS:
        assert np.isnan(got[key][5]), key
        assert np.array_equal(got[key][others].view(np.uint64), clean[key][others].view(np.uint64)), key
    assert np.all(np.isnan(got["pointwise"][:, 5])) and np.array_equal(got["pointwise"][:, others], clean["pointwise"][:, others])
    ch.close()


# --------------------------------------------------------------------------------------------------------------------------- row blocks
def test_row_blocks_and_a_second_call(native, monkeypatch):
    """200 rows in blocks of 64, 64, 64 and 8: the budget counts the matrix and the tail beside the predictions, 4 m d_out + 8 m + 16 M bytes
    per row.  The bits of the one-block call, matrix included; a second call returns the same bits"""
    ch = make_chain(native, "narrow")
    n, m = 200, 64
    X = rows_for("narrow", n=n, seed=5)
    thetas = walks(ch.P, 1, m, seed=51)
    Y = targets_for(ch.forward_many(thetas, X=X), LIK_FIXED_GAUSSIAN, np.random.default_rng(52))
    whole = ch.ensemble_loo(thetas, Y=Y, X=X, pointwise=True)
    again = ch.ensemble_loo(thetas, Y=Y, X=X, pointwise=True)
    per_row = m * ch.d_out + 2 * m + 4 * tail_length(m)                # in floats
    budget = per_row * 64 + 5
    assert max(64, budget // per_row // 64 * 64) == 64 and budget // (m * ch.d_out) // 64 * 64 > 64      # the extra bytes are what cuts
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    cut = ch.ensemble_loo(thetas, Y=Y, X=X, pointwise=True)
    monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
    for key in KEYS + ("pointwise",):
        assert np.array_equal(whole[key].view(np.uint64), again[key].view(np.uint64)), key
        assert np.array_equal(whole[key].view(np.uint64), cut[key].view(np.uint64)), key
    compare("row blocks", cut)
    ch.close()


def test_a_multi_chain_handle_and_single_outputs(native):
    """a tbnn_create_multi handle takes explicit thetas like a one-chain handle; any output alone is the one of the full call"""
    dp = C.POINTER(C.c_double)
    dims, act, last, lik, _prefix, _n = CASES["narrow"]
    ch = make_chain(native, "narrow")
    X = rows_for("narrow", seed=6)
    thetas = walks(ch.P, 1, 64, seed=61)
    Y = targets_for(ch.forward_many(thetas, X=X), LIK_FIXED_GAUSSIAN, np.random.default_rng(62))
    want = ch.ensemble_loo(thetas, Y=Y, X=X, pointwise=True)
    grp = native.ChainGroup(layers_for(dims, act, last), 3, likelihood=lik, fixed_sd=0.7)
    outs = [np.empty(ROWS) for _ in range(4)] + [np.empty((64, ROWS))]
    args = (native._p(thetas), 64, thetas.shape[1], LIK_FIXED_GAUSSIAN, None, 1, native._p(X), native._p(Y), ROWS, 1.0)
    rc = native.lib.tbnn_ensemble_loo(grp._h, *args, *[o.ctypes.data_as(dp) for o in outs])
    assert rc == 0, native.lib.tbnn_last_error()
    for key, o in zip(KEYS + ("pointwise",), outs):
        assert np.array_equal(o.view(np.uint64), want[key].view(np.uint64)), key
    grp.close()
    for j, key in enumerate(KEYS + ("pointwise",)):
        one = np.full(want[key].shape, 7.0)
        ptrs = [None] * 5
        ptrs[j] = one.ctypes.data_as(dp)
        assert native.lib.tbnn_ensemble_loo(ch._h, *args, *ptrs) == 0, native.lib.tbnn_last_error()
        assert np.array_equal(one.view(np.uint64), want[key].view(np.uint64)), key
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(native):
    dp = C.POINTER(C.c_double)
    ch = make_chain(native, "narrow")
    X = rows_for("narrow")
    thetas = walks(ch.P, 1, 25, seed=7)
    n, Pn = X.shape[0], thetas.shape[1]
    Y = np.zeros((n, 1), dtype=np.float32)
    lib, p = native.lib, native._p
    before = ch.ensemble_loo(thetas, Y=Y, X=X, pointwise=True)
    outs = [np.full(n, 7.0) for _ in range(4)] + [np.full((25, n), 7.0)]

    def call(m=25, stride=Pn, lik=LIK_FIXED_GAUSSIAN, sd=None, which=1, X_=X, Y_=Y, n_=n, r_eff=1.0, null=False):
        return lib.tbnn_ensemble_loo(ch._h, p(thetas), m, stride, lik, p(sd), which, p(X_), p(Y_), n_, r_eff,
                                     *[None if null else o.ctypes.data_as(dp) for o in outs])

    err = lambda: lib.tbnn_last_error().decode()
    assert call(null=True) < 0 and "every output is null" in err()
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert call(r_eff=bad) < 0 and "r_eff" in err(), bad
    assert call(m=1) < 0 and "fewer than 2" in err()
    assert call(m=0) < 0 and "fewer than 2" in err()
    assert call(Y_=None) < 0 and "without their targets" in err()
    assert call(lik=7) < 0 and "unknown likelihood" in err()
    assert call(lik=4) < 0 and "unknown likelihood" in err()
    assert call(lik=LIK_CATEGORICAL) < 0 and "at least 2 outputs" in err()
    sd = np.full(25, 0.5, dtype=np.float32)
    sd[7] = np.nan
    assert call(lik=LIK_GAUSSIAN, sd=sd) < 0 and "sd 7 is not a number" in err()
    assert call(stride=Pn - 1) < 0 and "theta_stride < P" in err()
    assert call(X_=None, Y_=None, n_=0, which=1) < 0 and "tbnn_set_validation has not been called" in err()
    assert call(X_=None, Y_=None, n_=0, which=2) < 0 and "which must be" in err()
    ch.set_data(X, Y)
    assert call(X_=None, n_=n - 1, which=0) < 0 and "does not match" in err()
    # 64 rows of all m networks, their matrix and tails past the block budget: refused before anything is read
    assert call(m=1_500_000) < 0 and "block budget" in err()
    assert all(np.all(o == 7.0) for o in outs)                   # nothing written
    with pytest.raises(native.TbnnError, match="r_eff"):
        ch.ensemble_loo(thetas, Y=Y, X=X, r_eff=0.0)
    with pytest.raises(ValueError):
        ch.ensemble_loo(thetas, X=X)
    assert call() == 0                                           # and the accepted call still works
    for key, o in zip(KEYS + ("pointwise",), outs):
        assert np.array_equal(o.view(np.uint64), before[key].view(np.uint64)), key
    ch.close()


# ---------------------------------------------------------------------------------------------------------------- predictor, end to end
def test_predictor_loo_waic_compare(tmp_path, monkeypatch, native):
    """a three-class network trained for a few epochs (the set-up of tests/test_gpu_categorical.py), its saved networks read back: the sums
    are the row arrays', a model compared with itself differs by nothing, and every second network is another (smaller) model over the same
    rows.  Under the predictor's own categorical likelihood lppd is logPredictiveDensity's, bit for bit, and pareto_k and p_waic meet the
    restatement under the absolute rule.  elpd_loo and lppd are compared with it where the relative rule is well-posed: the networks judged
    under a FixedGaussianLikelihood of sd 40, as a regression of the logits on the one-hot targets.  (Rows the classifier is certain of have
    an lppd of 1e-9 and less; the definition's own subtraction of log m leaves 1e-16 absolutely on either side, which says nothing
    relative to such a value.)"""
    from test_gpu_categorical import blobs, make_net
    from tensorbnn_amd.likelihood import CategoricalLikelihood, FixedGaussianLikelihood
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    X, Y = blobs(600, 1)
    Xv, Yv = blobs(ROWS, 2)
    Xv = (Xv + 1.2 * np.random.default_rng(3).standard_normal(Xv.shape)).astype(np.float32)      # held-out rows near and across the class borders
    net = make_net(X, Y, Xv, Yv)
    net.train(44, 1, CategoricalLikelihood(), folderName="blobs", networksPerFile=8, verbose=False)
    p = predictor(str(tmp_path / "blobs") + "/", likelihood=CategoricalLikelihood())
    m = p.numNetworks
    assert m >= 25
    for lik in (None, FixedGaussianLikelihood(sd=40.0)):
        res = p.loo(Xv, Yv, likelihood=lik, pointwise=True)
        w = p.waic(Xv, Yv, likelihood=lik)
        assert res["pointwise"].shape == (m, ROWS) and np.isfinite(res["pareto_k"]).any()
        assert res["elpd_loo"] == res["elpd_loo_rows"].sum() and res["looic"] == -2.0 * res["elpd_loo"]
        assert res["se"] == math.sqrt(ROWS * np.var(res["elpd_loo_rows"], ddof=1)) and res["p_loo"] == np.sum(res["lppd_rows"] - res["elpd_loo_rows"])
        assert res["k_threshold"] == min(1.0 - 1.0 / math.log10(m), 0.7) and res["n_bad_k"] == int(np.sum(res["pareto_k"] > res["k_threshold"]))
        assert np.array_equal(w["lppd_rows"], res["lppd_rows"]) and np.array_equal(w["elpd_waic_rows"], w["lppd_rows"] - w["p_waic_rows"])
        assert w["elpd_waic"] == w["elpd_waic_rows"].sum() and w["waic"] == -2.0 * w["elpd_waic"] and w["p_waic"] == np.sum(w["p_waic_rows"])
        _per_net, rows = p.logPredictiveDensity(Xv, Yv, likelihood=lik)
        assert np.array_equal(rows.view(np.uint64), res["lppd_rows"].view(np.uint64))
        assert predictor.compareLoo(res, res) == {"elpd_diff": 0.0, "se_diff": 0.0}
        half = p.loo(Xv, Yv, n=2, likelihood=lik)
        d = predictor.compareLoo(res, half)
        assert d["elpd_diff"] == np.sum(res["elpd_loo_rows"] - half["elpd_loo_rows"]) and d["se_diff"] > 0
        assert predictor.compareLoo(half, res)["elpd_diff"] == -d["elpd_diff"]
        if lik is None:
            compare("predictor categorical", {"pareto_k": res["pareto_k"], "p_waic": w["p_waic_rows"], "pointwise": res["pointwise"]},
                    keys=("pareto_k", "p_waic"))
    compare("predictor, judged as a regression", {"elpd_loo": res["elpd_loo_rows"], "pareto_k": res["pareto_k"], "lppd": res["lppd_rows"],
                                                  "p_waic": w["p_waic_rows"], "pointwise": res["pointwise"]})
