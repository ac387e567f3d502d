"""GPU: Harrell's concordance index of a survival ensemble (tbnn_ensemble_concordance, Chain.ensemble_concordance, predictor.concordance)
against the pair definition in plain NumPy (tests/concordance_ref.py) applied to the fp32 scores Chain.forward_many returns for the same
rows and to the returned fp64 mean score: only the reduction is judged, and every count is compared with ==.
Networks: 2-4-d_out tanh under KERNEL_GENERIC with random weights (scores differ by row); one case on the fused narrow 5-50-50-50-1.
T is the kernel's i-tile (and j-tile): 1024 sorted rows."""
import numpy as np
import pytest

import concordance_ref as cr

pytestmark = pytest.mark.gpu

T = 1024
KEYS = ("comparable", "concordant", "tied", "mean_concordant", "mean_tied", "mean_score")
# (rows, networks, d_out, kind, weighted).  ties: times from about n / 6 values, 40 % censored; events: all events at distinct times;
# censored: no event; quantised: a saturated first layer leaves a handful of score values; fused: the narrow family's chunk layout
CASES = [(1, 1, 1, "ties", False), (2, 5, 2, "ties", False), (T - 1, 1, 2, "ties", False), (T, 5, 1, "ties", True), (T + 1, 5, 2, "ties", False),
         (2 * T + 37, 5, 2, "ties", True), (2 * T + 37, 1, 1, "events", False), (T + 1, 5, 1, "censored", False),
         (T + 1, 5, 1, "quantised", False), (2 * T + 37, 5, 1, "fused", False)]


def problem(native, n, m, d_out, kind="ties", weighted=False):
    """(chain, thetas [m, P], X, signed targets Y [n, d_out], weights or None)"""
    if kind == "fused":
        ch = native.Chain([(5, 50, native.ACT_RELU, 0), (50, 50, native.ACT_RELU, 0), (50, 50, native.ACT_RELU, 0), (50, 1, native.ACT_NONE, 0)],
                          likelihood=native.LIK_FIXED_GAUSSIAN)
        assert ch.kernel_name.startswith("fast3<"), ch.kernel_name
    else:
        ch = native.Chain([(2, 4, native.ACT_TANH, 0), (4, d_out, native.ACT_NONE, 0)], likelihood=native.LIK_WEIBULL, kernel=native.KERNEL_GENERIC,
                          lik_df=1.5)
    rng = np.random.default_rng(31 * n + m)
    X = rng.uniform(-1, 1, (n, ch.d_in)).astype(np.float32)
    thetas = (0.5 * rng.standard_normal((m, ch.P))).astype(np.float32)
    if kind == "quantised":
        thetas[:, :12] *= np.float32(1e4)
    t = rng.integers(1, max(2, n // 6) + 1, (n, d_out)) * 0.25
    if kind == "events":
        t = np.stack([rng.permutation(n) + 1.0 for _ in range(d_out)], axis=1)
    ev = np.full((n, d_out), kind == "events") if kind in ("events", "censored") else rng.random((n, d_out)) >= 0.4
    w = np.where(np.arange(m) == 1, 0, 1 + np.arange(m) % 3).astype(np.float32) if weighted else None
    return ch, thetas, X, np.where(ev, t, -t).astype(np.float32), w


def check(ch, thetas, X, Y, w, res):
    """every count of res against the reference on forward_many's scores and on the mean score, which is ensemble_moments' bit for bit"""
    fm = ch.forward_many(thetas, X=X)
    mean = ch.ensemble_moments(thetas, X=X, weights=w, var=False)[0]
    assert np.array_equal(res["mean_score"].view(np.uint64), mean.view(np.uint64))
    for o in range(Y.shape[1]):
        assert (int(res["comparable"][o]), int(res["mean_concordant"][o]), int(res["mean_tied"][o])) == cr.concordance_ref(Y[:, o], mean[o]), o
        for k in range(thetas.shape[0]):
            assert (int(res["comparable"][o]), int(res["concordant"][k, o]), int(res["tied"][k, o])) == cr.concordance_ref(Y[:, o], fm[k, o]), (k, o)


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint64) if k == "mean_score" else a[k], b[k].view(np.uint64) if k == "mean_score" else b[k]) for k in KEYS)


@pytest.mark.parametrize("n,m,d_out,kind,weighted", CASES)
def test_against_reference(native, n, m, d_out, kind, weighted):
    ch, thetas, X, Y, w = problem(native, n, m, d_out, kind, weighted)
    res = ch.ensemble_concordance(thetas, Y=Y, X=X, weights=w)
    assert res["concordant"].shape == res["tied"].shape == (m, d_out) and res["mean_score"].shape == (d_out, n)
    check(ch, thetas, X, Y, w, res)
    if kind == "events":
        assert res["comparable"][0] == n * (n - 1) // 2
    if kind == "censored":
        assert res["comparable"][0] == 0 and not res["concordant"].any() and not res["tied"].any()
    if kind == "quantised":
        assert np.all(res["tied"] > 0) and np.all(res["concordant"] > 0)
    ch.close()


def test_staged_rows_and_targets(native):
    """X = None, Y = None: the rows and the targets staged with set_validation, the targets copied back to the host for its sort; one row
    past a tile edge with two columns, so the padded perm and its per-column offsets too"""
    ch, thetas, X, Y, _w = problem(native, T + 1, 2, 2)
    ch.set_validation(X, Y)
    res = ch.ensemble_concordance(thetas)
    assert res["concordant"].shape == (2, 2) and res["mean_score"].shape == (2, T + 1)
    check(ch, thetas, X, Y, None, res)
    ch.close()


def test_constant_score_and_nan(native):
    """a network whose weights are 0 ties every comparable pair (C = 1/2); a NaN bias gives that network -1 and leaves the others their counts"""
    ch, thetas, X, Y, _w = problem(native, T + 1, 5, 1)
    thetas[0, :-1] = 0
    clean = ch.ensemble_concordance(thetas, Y=Y, X=X)
    comp = int(clean["comparable"][0])
    assert comp > 0 and clean["tied"][0, 0] == comp and clean["concordant"][0, 0] == 0 and cr.c_index(comp, 0, comp) == 0.5
    check(ch, thetas, X, Y, None, clean)
    bad = thetas.copy()
    bad[2, -1] = np.nan
    res = ch.ensemble_concordance(bad, Y=Y, X=X)
    keep = [0, 1, 3, 4]
    four = ch.ensemble_concordance(thetas[keep], Y=Y, X=X)
    assert res["concordant"][2, 0] == res["tied"][2, 0] == -1 and res["mean_concordant"][0] == res["mean_tied"][0] == -1
    assert np.array_equal(res["concordant"][keep], four["concordant"]) and np.array_equal(res["tied"][keep], four["tied"])
    assert np.array_equal(four["concordant"], clean["concordant"][keep]) and res["comparable"][0] == comp
    ch.close()


def test_chunks_and_repeatability(native, monkeypatch):
    """5 networks in 3 chunks (half of the budget holds the predictions of 2): the one-chunk call's outputs, which a second call repeats"""
    n, m, d_out = 2 * T + 37, 5, 2
    ch, thetas, X, Y, w = problem(native, n, m, d_out, weighted=True)
    whole = ch.ensemble_concordance(thetas, Y=Y, X=X, weights=w)
    assert same(whole, ch.ensemble_concordance(thetas, Y=Y, X=X, weights=w))
    budget = 4 * n * d_out
    assert (budget // 2) // (n * d_out) == 2
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    assert same(whole, ch.ensemble_concordance(thetas, Y=Y, X=X, weights=w))
    ch.close()


def test_refusals(native):
    ch, thetas, X, Y, _w = problem(native, 5, 3, 1)
    pl = lambda a: a.ctypes.data_as(native.C.POINTER(native.C.c_int64))
    outs = [np.full(1, 7, dtype=np.int64), np.full((3, 1, 2), 7, dtype=np.int64), np.full((1, 2), 7, dtype=np.int64)]
    call = lambda Yb, n, Xb: native.lib.tbnn_ensemble_concordance(ch._h, native._p(thetas), 3, ch.P, None, 1, native._p(Xb), native._p(Yb), n,
                                                                  *[pl(a) for a in outs], None)
    for value in (0.0, np.nan, np.inf):
        Yb = Y.copy()
        Yb[3, 0] = value
        assert call(Yb, 5, X) < 0 and "not a finite, nonzero time" in native.lib.tbnn_last_error().decode()
    ch.set_validation(X, Y)
    assert call(Y[:4], 4, None) < 0 and "does not match the 5 staged rows" in native.lib.tbnn_last_error().decode()
    assert all(np.all(a == 7) for a in outs)
    assert call(None, 5, None) == 0 and outs[0][0] == cr.concordance_ref(Y[:, 0], np.zeros(5))[0]      # the staged targets; the handle stays usable
    ch.close()


def test_predictor(tmp_path, monkeypatch, native):
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.likelihood import GaussianLikelihood, WeibullLikelihood
    from tensorbnn_amd.network import network
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(71)
    X = rng.uniform(-2, 2, (120, 1)).astype(np.float32)
    lam = np.exp(1.0 + np.sin(2 * X.astype(np.float64)))
    t_ev, t_ce = lam * rng.weibull(1.5, (120, 1)), 1.3 * lam * rng.weibull(1.5, (120, 1))
    Y = WeibullLikelihood.encode(np.minimum(t_ev, t_ce), t_ev <= t_ce)
    lik = WeibullLikelihood(shape=1.5)
    net = network(np.float32, 1, X, Y, X[:20], Y[:20])
    net.add(DenseLayer(1, 16, seed=1000)); net.add(Tanh())
    net.add(DenseLayer(16, 16, seed=2000)); net.add(Tanh()); net.add(DenseLayer(16, 1, seed=3000))
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    net.train(30, 2, lik, folderName="wei", networksPerFile=1, verbose=False)
    p = predictor(str(tmp_path / "wei") + "/", likelihood=lik)
    m = p.numNetworks
    res = p.concordance(X, Y)
    ch, picked = p._ensure_chain(), np.stack(p.vectors)
    fm, mean = ch.forward_many(picked, X=X), ch.ensemble_moments(picked, X=X, var=False)[0]
    assert res["c_index"][0] == cr.c_index(*cr.concordance_ref(Y[:, 0], mean[0]))
    assert np.array_equal(res["per_network"][:, 0], [cr.c_index(*cr.concordance_ref(Y[:, 0], fm[k, 0])) for k in range(m)])
    assert res["per_network"].shape == (m, 1) and all(res[k].shape == (1,) for k in ("c_index", "mean", "sd", "q05", "q50", "q95", "comparable"))
    assert res["n_bad"] == 0 and res["q05"][0] <= res["q50"][0] <= res["q95"][0] and res["n_events"][0] + res["n_censored"][0] == 120
    wres = p.concordance(X, Y, weights=np.arange(m, dtype=np.float32))
    assert np.array_equal(wres["per_network"], res["per_network"]) and wres["q50"][0] in res["per_network"][1:, 0]
    none = p.concordance(X, -np.abs(Y))
    assert none["comparable"][0] == 0 and np.isnan(none["c_index"][0]) and none["n_bad"] == m and np.isnan(none["mean"][0])
    with pytest.raises(ValueError, match="needs a WeibullLikelihood"):
        p.concordance(X, Y, likelihood=GaussianLikelihood(sd=0.1))
