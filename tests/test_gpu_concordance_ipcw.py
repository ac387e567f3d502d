"""GPU: Uno's IPCW concordance index of a survival ensemble on a time grid (tbnn_ensemble_concordance_ipcw, Chain.ensemble_concordance_ipcw,
predictor.concordanceIpcw) against the pair definition in fp64 NumPy (tests/concordance_ipcw_ref.py).  The reference is fed what the
device compares: per network the fp32 predictions of Chain.forward_many, for the mean score Chain.ensemble_moments' mean; the weights are
tbnn_ipcw_weights' squared.  Every compare is therefore on identical bits and only the weighted sums may differ.
Band (derived, tests/test_gpu_auc.py's): a numerator is a sum of at most n non-negative terms omega_i x integer, any fp64 summation order
of which is within (n + 8) U relative of the exact sum, and so is D_g: |C - ref| <= 2 (n + 8) U ref.  NaN patterns equal, the cases ==.
Problems: tests/test_gpu_brier.problem.  Sizes around the kernel's tile of 1024 sorted positions (cases in registers, partners in LDS):
1023 / 1024 / 1025 rows; 1500 rows with 150 equal times across position 1024 and every second row of X a copy of its neighbour (masked
boundary tiles, score ties); 2085 rows: three tiles, one network per chunk under TBNN_ENS_CHUNK_FLOATS; 200001 rows, one event in 256, the
grid at the median and the 90 % quantile of the times: 196 tiles, the 177 that hold a case with up to 25 work items each (spans of 8
partner tiles), about 2400 items over the 1024 workgroups: every workgroup adds a second item to its slab.
Measured on an MI355X: the largest error over all cases was 5.7 % of the band (63 rows x 9 networks)."""
import numpy as np
import pytest

import concordance_ipcw_ref as cr
from test_gpu_brier import K, NAN_NET, close, problem
from test_gpu_predictive import U

pytestmark = pytest.mark.gpu
# (rows, networks, d_out, times, kind): the kinds of tests/test_gpu_brier.py, and edges: a grid time below every row's time and one above
# all of them; ties: equal times across a tile edge and duplicated rows of X; large: few events
CASES = [(1, 1, 1, 1, "plain"), (2, 1, 1, 2, "plain"), (63, 9, 2, 9, "plain"), (64, 24, 1, 9, "weights"), (65, 9, 2, 9, "nan"), (63, 9, 2, 2, "nan0"),
         (1023, 1, 1, 9, "edges"), (1024, 9, 1, 33, "weights"), (1025, 9, 1, 9, "events"), (257, 1, 1, 9, "censored"), (257, 24, 1, 33, "gy"),
         (1500, 9, 1, 33, "ties"), (2085, 9, 2, 33, "chunks"), (257, 9, 1, 33, "fused"), (200001, 1, 1, 2, "large")]


def check(res, f, sbar, Y, times, GY, native):
    m, d_out, n = f.shape
    omega = native.ipcw_weights(Y, times, GY)[0] ** 2
    worst = 0.0
    for o in range(d_out):
        ref, D, cases = cr.concordance_ipcw(Y[:, o], sbar[o], times, omega[o])
        assert np.array_equal(res["n_cases"][o], cases) and close(res["pair_weight"][o], D, (n + 8) * U * D), o
        refs, gots = [ref] + [cr.concordance_ipcw(Y[:, o], f[i, o], times, omega[o])[0] for i in range(m)], [res["c_index"][o]] + list(res["per_network"][:, o])
        for got, r in zip(gots, refs):
            tol = 2 * (n + 8) * U * r
            worst = max(worst, np.max(np.abs(got - r) / tol, initial=0.0, where=np.isfinite(r) & (r > 0)))
            assert close(got, r, tol), o
    print(f"[concordance_ipcw] n={n} m={m} T={len(times)}: error at most {worst:.2e} of the band")


@pytest.mark.parametrize("n,m,d_out,nt,kind", CASES)
def test_against_reference(native, monkeypatch, n, m, d_out, nt, kind):
    ch, thetas, X, Y, times, w, GY, f = problem(native, n, m, d_out, nt, kind)
    if kind in ("edges", "events"):
        times = np.concatenate([[0.5 * np.abs(Y).min()], times, [2.0 * np.abs(Y).max()]])
    if kind == "ties":
        run = np.argsort(np.abs(Y[:, 0]), kind="stable")[880:1030]
        Y[run, 0] = np.sign(Y[run, 0]) * np.abs(Y[run[0], 0])
        X[1::2] = X[:-1:2]
    if kind == "large":
        Y[:, 0] = np.where(np.arange(n) % 256 == 0, Y[:, 0], -np.abs(Y[:, 0]))
        times = np.quantile(np.abs(Y[:, 0]).astype(np.float64), [0.5, 0.9])
    if kind in ("ties", "large"):
        f = ch.forward_many(thetas, X=X)
    kw = dict(Y=Y, X=X, weights=w, censoringY=GY)
    if kind == "chunks":
        monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(2 * n * d_out))                             # one network per chunk
    res = ch.ensemble_concordance_ipcw(thetas, times, **kw)
    nt = len(times)
    assert res["c_index"].shape == (d_out, nt) and res["per_network"].shape == (m, d_out, nt) and res["n_cases"].dtype == np.int64
    check(res, f, ch.ensemble_moments(thetas, X=X, weights=w, var=False)[0], Y, times, GY, native)
    again = ch.ensemble_concordance_ipcw(thetas, times, **kw)
    assert all(np.array_equal(res[k].view(np.uint64), again[k].view(np.uint64)) for k in res)       # the same bits from run to run
    only = ch.ensemble_concordance_ipcw(thetas, times, per_network=False, **kw)
    assert "per_network" not in only and np.array_equal(only["c_index"].view(np.uint64), res["c_index"].view(np.uint64))
    if kind == "chunks":
        monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
        whole = ch.ensemble_concordance_ipcw(thetas, times, **kw)
        assert all(np.array_equal(res[k].view(np.uint64), whole[k].view(np.uint64)) for k in res)   # ... and whatever the chunks
    if kind in ("edges", "events"):                                                                  # no case at the first time
        assert np.isnan(res["c_index"][:, 0]).all() and np.isnan(res["per_network"][:, :, 0]).all() and not np.isnan(res["c_index"][:, 1:]).any()
        assert np.all(res["n_cases"][:, 0] == 0) and np.all(res["pair_weight"][:, 0] == 0) and res["n_cases"][0, -1] == np.sum(Y[:, 0] > 0)
    if kind == "events":                                                                             # omega == 1, tau above all times: Harrell's C
        har = ch.ensemble_concordance(thetas, Y=Y, X=X, weights=w)
        comp = har["comparable"].astype(np.float64)
        assert np.array_equal(res["pair_weight"][:, -1], comp) and np.array_equal(res["c_index"][:, -1], (har["mean_concordant"] + 0.5 * har["mean_tied"]) / comp)
        assert np.array_equal(res["per_network"][:, :, -1], (har["concordant"] + 0.5 * har["tied"]) / comp)
    if kind == "censored":
        assert np.isnan(res["c_index"]).all() and np.isnan(res["per_network"]).all() and np.all(res["n_cases"] == 0)
    if kind in NAN_NET:                                                                              # whatever the NaN network's weight
        bad = np.arange(d_out) == d_out - 1                                                          # the column of the NaN bias
        some = res["pair_weight"] > 0
        assert np.array_equal(np.isnan(res["per_network"]), ((np.arange(m)[:, None] == NAN_NET[kind]) & bad)[:, :, None] | ~some[None])
        assert np.array_equal(np.isnan(res["c_index"]), bad[:, None] | ~some)
    ch.close()


def test_predictor(tmp_path, monkeypatch, native):
    from tensorbnn_amd import activationFunctions as af, layer as ly, network as nw, predictor as pr
    from tensorbnn_amd.likelihood import GaussianLikelihood, WeibullLikelihood
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(71)
    X = rng.uniform(-2, 2, (120, 1)).astype(np.float32)
    lam = np.exp(1.0 + np.sin(2 * X.astype(np.float64)))
    t_ev, t_ce = lam * rng.weibull(K, (120, 1)), 1.3 * lam * rng.weibull(K, (120, 1))
    Y, lik = WeibullLikelihood.encode(np.minimum(t_ev, t_ce), t_ev <= t_ce), WeibullLikelihood(shape=K)
    net = nw.network(np.float32, 1, X, Y, X[:20], Y[:20])
    for layer in (ly.DenseLayer(1, 16, seed=1000), af.Tanh(), ly.DenseLayer(16, 1, seed=3000)):
        net.add(layer)
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    net.train(20, 2, lik, folderName="wei", networksPerFile=1, verbose=False)
    p = pr.predictor(str(tmp_path / "wei") + "/", likelihood=lik)
    res = p.concordanceIpcw(X, Y)
    ts, m = res["times"], p.numNetworks
    assert ts.shape == (32,) and np.array_equal(ts, p.brierScore(X, Y)["times"]) and res["n_bad"] == 0
    assert res["c_index"].shape == (1, 32) and res["per_network"].shape == (m, 1, 32) and all(res[k].shape == (1, 32) for k in ("mean", "sd", "q05", "q50", "q95"))
    direct = p._ensure_chain().ensemble_concordance_ipcw(np.stack(p.vectors), ts, Y=Y, X=X)
    assert all(np.array_equal(res[k].view(np.uint64), direct[k].view(np.uint64)) for k in direct)
    assert np.all((0 < res["c_index"]) & (res["c_index"] <= 1)) and np.all(res["q05"] <= res["q50"]) and np.all(res["q50"] <= res["q95"])
    with pytest.raises(ValueError, match="needs a WeibullLikelihood"):
        p.concordanceIpcw(X, Y, likelihood=GaussianLikelihood(sd=0.1))


def test_refusals(native):
    """a bad grid and a zero / NaN target in Y and in G_Y are refused with nothing written, and the handle works afterwards"""
    ch = native.Chain([(2, 4, native.ACT_TANH, 0), (4, 1, native.ACT_NONE, 0)], likelihood=native.LIK_FIXED_GAUSSIAN, kernel=native.KERNEL_GENERIC)
    th, X, Y, out = np.zeros((2, ch.P), dtype=np.float32), np.ones((3, 2), dtype=np.float32), np.float32([[1], [-2], [3]]), np.full(2, 7.0)
    cases = np.full(2, 7, dtype=np.int64)

    def call(ts=np.float64([1, 2]), Yb=Y, gy=None, o=out):
        return native.lib.tbnn_ensemble_concordance_ipcw(ch._h, native._p(th), 2, ch.P, None, 1, native._p(X), native._p(Yb), 3, native._p(gy),
                                                         0 if gy is None else len(gy), native._pd(ts), 2, native._pd(o), None, None,
                                                         cases.ctypes.data_as(native.C.POINTER(native.C.c_int64)))

    for why, kw in [("not above its predecessor", dict(ts=np.float64([2, 1]))), ("not finite, not > 0", dict(ts=np.float64([0, 1]))),
                    ("not a finite, nonzero time", dict(Yb=np.float32([[1], [0], [3]]))), ("not a finite, nonzero time", dict(Yb=np.float32([[1], [np.nan], [3]]))),
                    ("(G_Y): target 1 is not a finite", dict(gy=np.float32([[1], [0]]))), ("(G_Y): target 0 is not a finite", dict(gy=np.float32([[np.inf], [2]]))),
                    ("without their targets", dict(Yb=None))]:
        rc = call(**kw)
        assert rc < 0 and why in native.lib.tbnn_last_error().decode() and np.all(out == 7.0) and np.all(cases == 7), (why, rc, native.lib.tbnn_last_error())
    assert call() == 0 and np.array_equal(cases, [0, 1]) and np.isnan(out[0]) and out[1] == 0.5      # thetas 0: the one pair at tau = 2 is a tie
    ch.close()
