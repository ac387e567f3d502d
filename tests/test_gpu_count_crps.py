"""GPU: the CRPS of a predictive mixture of count distributions (tbnn_ensemble_count_crps, Chain.ensemble_count_crps, predictor.countCrps)
against the SciPy restatement of its definition (tests/count_crps_ref.py) applied to the fp32 log-rates Chain.forward_many returns for
the same rows: only the reduction is judged.  Networks: 2-4-d_out, weights 0, the last biases the log-rates: a case's rows differ by their targets.
The band, per element:  |got - ref| <= REF_FIG max(1, |ref|) + 8 (n_k + m) 2^-53 max(1, error_ref),  n_k the values of k the reference
sums over: the second term is the worst case of summing that many terms >= 0 in any order, the first the reference's own error.
REF_FIG = 4 x the largest relative difference between count_crps_ref and the same sums in 50-digit mpmath over the first six rows (one
per kind of target) of every case of test_against_reference, as `python tools/count_crps_ref_fig.py` prints it."""
import numpy as np
import pytest

import count_crps_ref as cc
from count_crps_ref import NEGB, POIS

pytestmark = pytest.mark.gpu

REF_FIG = 4 * 5.906e-13     # `python tools/count_crps_ref_fig.py`: the largest of its lines, at r = 0.5 (Poisson 8.7e-14, r = 50 9.9e-15)
KEYS = ("crps", "error", "spread")
# (likelihood, r, m, d_out, rows, weighted).  LARGE: four networks near rate 2^17 (the anchor's Stirling branch, windows of some 9,000 values)
LARGE = (np.log(2.0 ** 17) + np.array([[-0.01], [0.0], [0.004], [0.012]])).astype(np.float32)
CASES = [(POIS, None, 1, 1, 33, False), (POIS, None, 7, 3, 67, True), (POIS, None, 8, 1, 33, False), (POIS, None, 9, 1, 67, True),
         (POIS, None, 17, 3, 33, False), (NEGB, 50.0, 1, 1, 33, False), (NEGB, 50.0, 8, 1, 67, True), (NEGB, 50.0, 17, 3, 33, False),
         (NEGB, 0.5, 7, 1, 33, True), (NEGB, 0.5, 9, 1, 67, False), (POIS, None, "large", 1, 8, False)]


def weights(m, weighted):
    return np.where(np.arange(m) % 3 == 1, 0, 1 + np.arange(m) % 4).astype(np.float32) if weighted and m > 1 else None


def run(native, lik, r, f, rows, w=None, Y=None):
    """a chain whose predictions are the log-rates f [m, d_out] on every row: (the three planes, forward_many's output, the targets)"""
    ch = native.Chain([(2, 4, native.ACT_TANH, 0), (4, f.shape[1], native.ACT_NONE, 0)], likelihood=lik, kernel=native.KERNEL_GENERIC,
                      lik_df=0.0 if r is None else r)
    thetas = np.zeros((f.shape[0], ch.P), dtype=np.float32)
    thetas[:, -f.shape[1]:] = f
    X = np.random.default_rng(3).uniform(-1, 1, (rows, 2)).astype(np.float32)
    Y = cc.targets(f, rows) if Y is None else Y
    got = ch.ensemble_count_crps(thetas, Y=Y, X=X, weights=w)
    fm = ch.forward_many(thetas, X=X)
    ch.close()
    return got, fm, Y


def check_band(tag, got, fm, Y, lik, r, w):
    m, d_out, n = fm.shape
    w = np.ones(m) if w is None else w
    for j in range(d_out):
        assert np.all(fm[:, j, :] == fm[:, j, :1])                      # (one set of rates per output: one reference sweep)
        ref = cc.count_crps_ref(fm[:, j, 0], w, Y[:, j], lik, r)
        tol = lambda v, sel=slice(None): REF_FIG * np.maximum(1, np.abs(v)) + 8 * (ref[3] + m) * 2.0 ** -53 * np.maximum(1, ref[1][sel])
        for k, v in zip(KEYS, ref):
            d = np.abs(got[k][j] - v)
            print(f"[count crps] {tag} output {j} {k}: worst {d.max():.3e} (band there {tol(v)[d.argmax()]:.3e}), n_k {ref[3]}")
            assert np.all(np.isfinite(got[k][j])) and np.all(d <= tol(v)), (tag, j, k)
        assert np.all(np.abs(got["crps"][j] - (got["error"][j] - got["spread"][j])) <= tol(ref[0]))
        if lik == POIS:
            ok = (Y[:, j] >= 0) & (Y[:, j] == np.floor(Y[:, j]))
            closed = np.array([cc.poisson_error_closed(fm[:, j, 0], w, float(y)) for y in Y[ok, j]])
            assert np.all(np.abs(got["error"][j][ok] - closed) <= tol(closed, ok))


@pytest.mark.parametrize("lik,r,m,d_out,rows,weighted", CASES)
def test_against_reference(native, lik, r, m, d_out, rows, weighted):
    f, w = (LARGE, None) if m == "large" else (cc.log_rates(m, d_out), weights(m, weighted))
    got, fm, Y = run(native, lik, r, f, rows, w)
    check_band(f"lik {lik} r {r} m {m}", got, fm, Y, lik, r, w)


def test_row_blocks_and_repeatability(native, monkeypatch):
    """517 rows in three blocks (the driver's rule with the sweep's scratch in the budget): the one-block call's bits, which a second call repeats"""
    m, rows, rb = 9, 517, 192
    f, w = cc.log_rates(m, 1), weights(m, True)
    whole, _fm, Y = run(native, NEGB, 50.0, f, rows, w)
    again, _fm, _Y = run(native, NEGB, 50.0, f, rows, w)
    budget = 11 * m * rb + 7
    assert max(64, budget // (11 * m) // 64 * 64) == rb and -(-rows // rb) == 3
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    cut, _fm, _Y = run(native, NEGB, 50.0, f, rows, w)
    for k in KEYS:
        assert np.array_equal(whole[k].view(np.uint64), cut[k].view(np.uint64)) and np.array_equal(whole[k].view(np.uint64), again[k].view(np.uint64)), k


def test_nan_and_ceilings(native):
    """only the marked elements are NaN, in all three planes; the others keep the bits of the clean run"""
    m, rows = 9, 33
    f, w = cc.log_rates(m, 1), weights(m, True)
    clean, _fm, Y = run(native, POIS, None, f, rows, w)

    def expect(got, bad_rows):
        bad = np.zeros((1, rows), dtype=bool)
        bad[0, bad_rows] = True
        for k in KEYS:
            assert np.array_equal(np.isnan(got[k]), bad), k
            assert np.array_equal(got[k][~bad].view(np.uint64), clean[k][~bad].view(np.uint64)), k

    Yb = Y.copy()
    Yb[3], Yb[5] = np.nan, 2.0 ** 20 + 1
    expect(run(native, POIS, None, f, rows, w, Yb)[0], [3, 5])
    # a NaN under weight 0 (w[1] = 0); a rate past the ceiling that counts, and under weight 0, where it is not looked at
    for net, value, every in ((1, np.nan, True), (0, np.log(2.0 ** 20) + 0.1, True), (1, np.log(2.0 ** 20) + 0.1, False)):
        fb = f.copy()
        fb[net] = value
        expect(run(native, POIS, None, fb, rows, w, Y)[0], list(range(rows)) if every else [])
    got = run(native, NEGB, 0.05, np.full((2, 1), np.log(2.0 ** 20) - 0.01, dtype=np.float32), 3)[0]      # the range exceeds the cap
    assert all(np.isnan(got[k]).all() for k in KEYS)


def test_refusals_and_predictor(tmp_path, monkeypatch, native):
    ch = native.Chain([(2, 4, native.ACT_TANH, 0), (4, 1, native.ACT_NONE, 0)], likelihood=POIS, kernel=native.KERNEL_GENERIC)
    thetas = np.zeros((4, ch.P), dtype=np.float32)
    X, Y = np.zeros((5, 2), dtype=np.float32), np.ones((5, 1), dtype=np.float32)
    outs = [np.full((1, 5), 7.0) for _ in range(3)]
    call = lambda lik, o=True: native.lib.tbnn_ensemble_count_crps(ch._h, native._p(thetas), 4, ch.P, lik, None, 1, native._p(X), native._p(Y), 5,
                                                                   *[native._pd(a) if o else None for a in outs])
    for lik, name in zip((0, 1, 2, 3, 8, 12, 14, 16), "GAUSSIAN FIXED_GAUSSIAN BERNOULLI CATEGORICAL STUDENT_T HETERO_GAUSSIAN GAMMA WEIBULL".split()):
        assert call(lik) < 0 and f"TBNN_LIK_{name} is not a count likelihood" in native.lib.tbnn_last_error().decode()
    assert call(POIS, o=False) < 0 and "every output is null" in native.lib.tbnn_last_error().decode()
    assert all(np.all(a == 7.0) for a in outs)
    assert call(POIS) == 0 and np.all(outs[0] >= 0)                      # the handle stays usable
    with pytest.raises(native.TbnnError, match="dispersion"):
        ch.ensemble_count_crps(thetas, Y=Y, X=X, likelihood=NEGB)
    ch.close()
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.likelihood import NegativeBinomialLikelihood, PoissonLikelihood
    from tensorbnn_amd.network import network
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    res, rng = {}, np.random.default_rng(5)
    X = rng.uniform(-1, 1, (60, 1)).astype(np.float32)
    Y = rng.poisson(np.exp(1.0 + X)).astype(np.float32)
    for name, lik in (("pois", PoissonLikelihood()), ("negb", NegativeBinomialLikelihood(dispersion=3.0))):
        net = network(np.float32, 1, X, Y, X[:20], Y[:20])
        net.add(DenseLayer(1, 16, seed=1000)); net.add(Tanh())
        net.add(DenseLayer(16, 16, seed=2000)); net.add(Tanh()); net.add(DenseLayer(16, 1, seed=3000))
        net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                      leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
        net.train(30, 2, lik, folderName=name, networksPerFile=1, verbose=False)
        p = predictor(str(tmp_path / name) + "/", likelihood=lik)
        res[name] = p.countCrps(X, Y)
        assert set(res[name]) == set(KEYS) | {"mean_crps", "se", "n_bad"} and res[name]["n_bad"] == 0 and res[name]["mean_crps"][0] > 0
        with pytest.raises(ValueError, match="count"):
            p.crps(X, Y)
    c = predictor.compareCrps(res["pois"], res["negb"])
    assert np.isfinite(c["crps_diff"][0]) and c["se_diff"][0] > 0
