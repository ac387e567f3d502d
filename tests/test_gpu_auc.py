"""GPU: the cumulative/dynamic time-dependent AUC of a survival ensemble (tbnn_ensemble_auc, Chain.ensemble_auc, predictor.timeDependentAuc)
against the pair definition in fp64 NumPy (tests/auc_ref.py).  The reference is fed what the device compares: per network the fp32
predictions of Chain.forward_many, for the mixture the curves Chain.ensemble_brier returns for the same call; the case weights are
tbnn_ipcw_weights' (tests/test_brier_host.py).  Every compare is therefore on identical bits and only the weighted sums may differ.
Band (derived): a numerator is a sum of at most n non-negative terms omega_i x integer, any fp64 summation order of which is within
(n + 8) U relative of the exact sum, and so is W_g: |auc - ref| <= 2 (n + 8) U ref.  NaN patterns equal, the controls ==.
Problems: tests/test_gpu_brier.problem.  Sizes around the kernel's tile of 1024 sorted positions (cases in registers, controls in LDS):
1023 / 1024 / 1025 rows; 1500 rows with 150 equal times across position 1024 and every second row of X a copy of its neighbour;
2085 rows: three control tiles, and one network per chunk under TBNN_ENS_CHUNK_FLOATS; 200001 rows, one event in 256, the grid at
the median and the 90 % quantile of the times: 196 tiles, the 98 below the median with 13 work items each (98 control tiles in spans of
8), so more than the 1024 workgroups: the first ones add a second item to their slabs."""
import numpy as np
import pytest

import auc_ref as ar
from test_gpu_brier import K, NAN_NET, close, problem
from test_gpu_predictive import U

pytestmark = pytest.mark.gpu
# (rows, networks, d_out, times, kind): the kinds of tests/test_gpu_brier.py, and edges: a grid time below every row's time and one above
# all of them; ties: equal times across a tile edge and duplicated rows of X; large: few events
CASES = [(1, 1, 1, 1, "plain"), (2, 1, 1, 2, "plain"), (63, 9, 2, 9, "plain"), (64, 24, 1, 9, "weights"), (65, 9, 2, 9, "nan"), (63, 9, 2, 2, "nan0"),
         (1023, 1, 1, 9, "edges"), (1024, 9, 1, 33, "weights"), (1025, 9, 1, 9, "events"), (257, 1, 1, 9, "censored"), (257, 24, 1, 33, "gy"),
         (1500, 9, 1, 33, "ties"), (2085, 9, 2, 33, "chunks"), (257, 9, 1, 33, "fused"), (200001, 1, 1, 2, "large")]


def check(res, f, curves, Y, times, GY, native):
    m, d_out, n = f.shape
    omega = native.ipcw_weights(Y, times, GY)[0]
    worst = 0.0
    for o in range(d_out):
        ref, W, C = ar.auc(Y[:, o], curves[:, o], times, omega[o])
        assert np.array_equal(res["n_controls"][o], C) and close(res["case_weight"][o], W, (n + 8) * U * W), o
        refs, gots = [ref] + [ar.auc(Y[:, o], f[i, o], times, omega[o])[0] for i in range(m)], [res["auc"][o]] + list(res["per_network"][:, o])
        for got, r in zip(gots, refs):
            tol = 2 * (n + 8) * U * r
            worst = max(worst, np.max(np.abs(got - r) / tol, initial=0.0, where=np.isfinite(r) & (r > 0)))
            assert close(got, r, tol), o
    print(f"[auc] n={n} m={m} T={len(times)}: error at most {worst:.2e} of the band")
    return worst


@pytest.mark.parametrize("n,m,d_out,nt,kind", CASES)
def test_against_reference(native, monkeypatch, n, m, d_out, nt, kind):
    ch, thetas, X, Y, times, w, GY, f = problem(native, n, m, d_out, nt, kind)
    if kind == "edges":
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
    kw = dict(Y=Y, X=X, likelihood=native.LIK_WEIBULL, weights=w, censoringY=GY)
    if kind == "chunks":
        monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(512 * m * d_out))                           # one network per chunk, row blocks of 512
    res = ch.ensemble_auc(thetas, times, **kw)
    nt = len(times)
    assert res["auc"].shape == (d_out, nt) and res["per_network"].shape == (m, d_out, nt) and res["n_controls"].dtype == np.int64
    curves = ch.ensemble_brier(thetas, times, per_network=False, curves=True, **kw)["curves"]
    check(res, f, curves, Y, times, GY, native)
    again = ch.ensemble_auc(thetas, times, **kw)
    assert all(np.array_equal(res[k].view(np.uint64), again[k].view(np.uint64)) for k in res)       # the same bits from run to run
    only = ch.ensemble_auc(thetas, times, per_network=False, **kw)
    assert "per_network" not in only and np.array_equal(only["auc"].view(np.uint64), res["auc"].view(np.uint64))
    if kind == "chunks":
        monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
        whole = ch.ensemble_auc(thetas, times, **kw)
        assert all(np.array_equal(res[k].view(np.uint64), whole[k].view(np.uint64)) for k in res)   # ... and whatever the chunks
    if kind == "edges":                                                                              # no case at the first time, no control at the last
        assert np.isnan(res["auc"][:, [0, -1]]).all() and np.isnan(res["per_network"][:, :, [0, -1]]).all() and not np.isnan(res["auc"][:, 1:-1]).any()
        assert res["case_weight"][0, 0] == 0 and res["n_controls"][0, 0] == n and res["n_controls"][0, -1] == 0
    if kind in ("censored", "events"):
        assert np.isnan(res["auc"]).all() == (kind == "censored")
    if kind in NAN_NET:                                                                              # whatever the NaN network's weight
        bad = np.arange(d_out) == d_out - 1                                                          # the column of the NaN bias
        some = (res["case_weight"] > 0) & (res["n_controls"] > 0)
        assert np.array_equal(np.isnan(res["per_network"]), ((np.arange(m)[:, None] == NAN_NET[kind]) & bad)[:, :, None] | ~some[None])
        assert np.array_equal(np.isnan(res["auc"]), bad[:, None] | ~some)
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
    res = p.timeDependentAuc(X, Y)
    ts, m = res["times"], p.numNetworks
    assert ts.shape == (32,) and res["auc"].shape == (32, 1) and res["per_network"].shape == (m, 32, 1) and res["iauc_per_network"].shape == (m, 1)
    assert np.array_equal(ts, p.brierScore(X, Y)["times"])
    ch, th = p._ensure_chain(), np.stack(p.vectors)
    curves = ch.ensemble_brier(th, ts, Y=Y, X=X, likelihood=native.LIK_WEIBULL, per_network=False, curves=True)["curves"]
    check({"auc": res["auc"].T, "per_network": res["per_network"].transpose(0, 2, 1), "case_weight": res["case_weight"].T, "n_controls": res["n_controls"].T},
          ch.forward_many(th, X=X), curves, Y, ts, None, native)
    assert 0 < res["iauc"][0] <= 1 and res["n_bad"] == 0 and res["q05"][0] <= res["q50"][0] <= res["q95"][0]
    assert np.isclose(res["iauc"][0], np.sum(0.5 * (res["auc"][1:, 0] + res["auc"][:-1, 0]) * np.diff(ts)) / (ts[-1] - ts[0]), rtol=1e-14, atol=0)
    with pytest.raises(ValueError, match="needs a WeibullLikelihood"):
        p.timeDependentAuc(X, Y, likelihood=GaussianLikelihood(sd=0.1))


def test_refusals(native):
    """what tbnn_ensemble_auc refuses beyond the grid's and the targets' refusals (tests/test_brier_host.py), with nothing written"""
    ch = native.Chain([(2, 4, native.ACT_TANH, 0), (4, 1, native.ACT_NONE, 0)], likelihood=native.LIK_FIXED_GAUSSIAN, kernel=native.KERNEL_GENERIC)
    th, X, Y, ts, out = np.zeros((4097, ch.P), dtype=np.float32), np.ones((3, 2), dtype=np.float32), np.float32([[1], [-2], [3]]), np.float64([1, 2]), np.full(2, 7.0)

    def refused(why, m=2, lik=native.LIK_WEIBULL, Yb=Y, gy=None, o=out, n=3, T=2):
        rc = native.lib.tbnn_ensemble_auc(ch._h, native._p(th), m, ch.P, lik, None, 1, native._p(X), native._p(Yb), n, native._p(gy), 0,
                                          native._pd(ts), T, native._pd(o), None, None, None)
        assert rc < 0 and why in native.lib.tbnn_last_error().decode() and np.all(out == 7.0), (why, rc, native.lib.tbnn_last_error())

    refused("needs the shape")
    ch.set_lik_df(K)
    for why, kw in [("every output is null", dict(o=None)), ("without their targets", dict(Yb=None)), ("no survival function", dict(lik=native.LIK_POISSON)),
                    ("exceeds 4096 networks", dict(m=4097)), ("G_Y with n_g < 1", dict(gy=Y)), ("T must be", dict(T=257)),
                    ("not a finite, nonzero time", dict(Yb=np.float32([[1], [0], [3]]))),
                    ("more than 4194304 rows", dict(Yb=np.ones((2 ** 22 + 1, 1), dtype=np.float32), n=2 ** 22 + 1))]:
        refused(why, **kw)
    ch.close()
