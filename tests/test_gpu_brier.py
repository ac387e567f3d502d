"""GPU: the IPCW Brier score of a survival ensemble over a time grid (tbnn_ensemble_brier, Chain.ensemble_brier, predictor.brierScore)
against the definition in fp64 NumPy (tests/brier_ref.py) applied to the fp32 predictions Chain.forward_many returns for the same rows.
Networks: 2-4-d_out tanh under KERNEL_GENERIC, shape 1.5, targets drawn around the networks' own log-scales, about 35 % censored; one case
on the fused narrow 5-50-50-50-1.  Bands: the curves within T(m) of tests/test_gpu_gamma_predictive.py (the Weibull mixture CDF's); a row's
term (I - S)^2 moves by at most 2 T(m) and any fp64 summation order over n rows adds (n + 8) U relative, so the scores within
(2 T(m) + (n + 8) U) x the mean weight.  Sizes around the kernel's 64-row tile, its tile of 8 times and its batch of 8 networks, and
65601 rows: 1026 row tiles over the grid's 1024 workgroups, so that the first two workgroups add a second tile to their slabs, the last of one row."""
import numpy as np
import pytest

import brier_ref as br
from test_gpu_gamma_predictive import T as band
from test_gpu_predictive import U, mix

pytestmark = pytest.mark.gpu
K = 1.5
# (rows, networks, d_out, times, kind): weights: network weights with a zero; nan: one network's last bias NaN; nan0: both, the NaN network
# the one of weight 0; events / censored: no censored row / no event; gy: the censoring distribution from other targets; chunks: 2085 rows
# in blocks of 512; fused: the narrow family
CASES = [(1, 1, 1, 1, "plain"), (63, 9, 2, 7, "plain"), (64, 24, 1, 8, "weights"), (65, 9, 2, 9, "nan"), (63, 9, 2, 7, "nan0"),
         (257, 24, 2, 33, "weights"), (257, 9, 1, 8, "events"), (257, 1, 1, 9, "censored"), (257, 24, 1, 33, "gy"), (2085, 9, 2, 33, "chunks"),
         (257, 9, 1, 33, "fused"), (65601, 1, 1, 1, "plain"), (65601, 9, 1, 9, "weights")]
NAN_NET = {"nan": 2, "nan0": 1}


def problem(native, n, m, d_out, nt, kind):
    """(chain, thetas, X, Y, times, weights or None, G_Y or None, f = forward_many's predictions)"""
    if kind == "fused":
        ch = native.Chain([(5, 50, native.ACT_RELU, 0), (50, 50, native.ACT_RELU, 0), (50, 50, native.ACT_RELU, 0), (50, 1, native.ACT_NONE, 0)],
                          likelihood=native.LIK_FIXED_GAUSSIAN)
        assert ch.kernel_name.startswith("fast3<"), ch.kernel_name
        ch.set_lik_df(K)
    else:
        ch = native.Chain([(2, 4, native.ACT_TANH, 0), (4, d_out, native.ACT_NONE, 0)], likelihood=native.LIK_WEIBULL, kernel=native.KERNEL_GENERIC, lik_df=K)
    rng = np.random.default_rng(31 * n + m)
    X = rng.uniform(-1, 1, (n, ch.d_in)).astype(np.float32)
    thetas = ((0.1 if kind == "fused" else 0.5) * rng.standard_normal((m, ch.P))).astype(np.float32)
    lam = np.exp(ch.forward_many(thetas, X=X).astype(np.float64).mean(axis=0).T)                 # [n, d_out]
    t_ev, t_ce = lam * rng.weibull(K, (n, d_out)), 1.5 * lam * rng.weibull(K, (n, d_out))
    Y = (t_ev if kind == "events" else -t_ce if kind == "censored" else np.where(t_ev <= t_ce, t_ev, -t_ce)).astype(np.float32)
    GY = (Y[::2] * np.float32(1.25)).astype(np.float32) if kind == "gy" else None
    # the grid: from the 10 % to the 90 % quantile of the times, and one row's own time
    own = float(abs(Y[n // 2, 0]))
    times = np.unique(np.append(np.linspace(*np.quantile(np.abs(Y).astype(np.float64), [0.1, 0.9]), nt - 1), own)) if nt > 1 else np.array([own])
    assert times.size == nt
    if kind in NAN_NET:
        thetas[NAN_NET[kind], -1] = np.nan
    w = np.where(np.arange(m) == 1, 0, 1 + np.arange(m) % 3).astype(np.float32) if kind in ("weights", "nan0") else None
    return ch, thetas, X, Y, times, w, GY, ch.forward_many(thetas, X=X)


def close(got, ref, tol):
    ok = ~np.isnan(ref)
    return np.array_equal(np.isnan(got), ~ok) and np.all(np.abs(got - ref)[ok] <= np.broadcast_to(tol, ref.shape)[ok])


def check(res, f, Y, times, w, GY):
    m, d_out, n = f.shape
    S = br.survival(f, K, times)                                                                    # [m, d_out, T, n]
    keep = np.ones(m, dtype=bool) if w is None else w > 0
    Sbar = mix(S[keep], None if w is None else w[keep])
    Sbar[np.isnan(S).any(axis=0)] = np.nan                                                           # whatever the network's weight
    assert close(res["curves"], Sbar.transpose(1, 0, 2), band(m))
    for o in range(d_out):
        gy = None if GY is None else GY[:, o]
        ref_net, mw = br.brier(Y[:, o], S[:, o], times, gy)
        tol = (2 * band(m) + (n + 8) * U) * mw
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = np.max(np.abs(res["per_network"][:, o] - ref_net) / tol, initial=0.0, where=np.isfinite(ref_net) & (tol > 0))
        print(f"[brier] n={n} m={m} T={len(times)} o={o}: per-network error at most {worst:.2e} of the band")
        assert close(res["mean_weight"][o], mw, (n + 8) * U * mw) and close(res["per_network"][:, o], ref_net, tol), o
        assert close(res["brier"][o], br.brier(Y[:, o], Sbar[o], times, gy)[0], tol), o


@pytest.mark.parametrize("n,m,d_out,nt,kind", CASES)
def test_against_reference(native, monkeypatch, n, m, d_out, nt, kind):
    ch, thetas, X, Y, times, w, GY, f = problem(native, n, m, d_out, nt, kind)
    score = lambda **kw: ch.ensemble_brier(thetas, times, Y=Y, X=X, likelihood=native.LIK_WEIBULL, weights=w, censoringY=GY, **kw)
    if kind == "chunks":
        monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(512 * m * d_out))                           # blocks of 512 rows, a ragged last one
    res = score(curves=True)
    assert res["brier"].shape == (d_out, nt) and res["per_network"].shape == (m, d_out, nt) and res["curves"].shape == (nt, d_out, n)
    check(res, f, Y, times, w, GY)
    again = score(curves=True)
    assert all(np.array_equal(res[k].view(np.uint64), again[k].view(np.uint64)) for k in res)       # the same bits from run to run
    assert np.all(np.diff(res["curves"], axis=0)[~np.isnan(res["curves"][1:])] <= 0)                 # a survival curve does not rise
    only = score(per_network=False)                                                                  # the kernel without the per-network sums
    assert set(only) == {"brier", "mean_weight"} and close(only["brier"], res["brier"], 0.0)
    if kind == "chunks":
        monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
        check(score(curves=True), f, Y, times, w, GY)                                               # one block: the same within the band
    if kind in NAN_NET:                                                                              # whatever the NaN network's weight
        bad = np.arange(d_out) == d_out - 1                                                          # the column of the NaN bias
        assert np.array_equal(np.isnan(res["per_network"]), np.broadcast_to((np.arange(m)[:, None] == NAN_NET[kind]) & bad, (nt, m, d_out)).transpose(1, 2, 0))
        assert np.array_equal(np.isnan(res["brier"]), np.broadcast_to(bad[:, None], (d_out, nt)))
        assert np.array_equal(np.isnan(res["curves"]), np.broadcast_to(bad[None, :, None], (nt, d_out, n)))
    ch.close()


def test_predictor(tmp_path, monkeypatch, native):
    from tensorbnn_amd import activationFunctions as af, layer as ly, network as nw, predictor as pr
    from tensorbnn_amd.likelihood import WeibullLikelihood
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(71)
    X = rng.uniform(-2, 2, (120, 1)).astype(np.float32)
    lam = np.exp(1.0 + np.sin(2 * X.astype(np.float64)))
    t_ev, t_ce = lam * rng.weibull(1.5, (120, 1)), 1.3 * lam * rng.weibull(1.5, (120, 1))
    Y, lik = WeibullLikelihood.encode(np.minimum(t_ev, t_ce), t_ev <= t_ce), WeibullLikelihood(shape=1.5)
    net = nw.network(np.float32, 1, X, Y, X[:20], Y[:20])
    for layer in (ly.DenseLayer(1, 16, seed=1000), af.Tanh(), ly.DenseLayer(16, 16, seed=2000), af.Tanh(), ly.DenseLayer(16, 1, seed=3000)):
        net.add(layer)
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    net.train(30, 2, lik, folderName="wei", networksPerFile=1, verbose=False)
    p = pr.predictor(str(tmp_path / "wei") + "/", likelihood=lik)
    res = p.brierScore(X, Y, curves=True)
    ts, m = res["times"], p.numNetworks
    assert ts.shape == (32,) and res["brier"].shape == (32, 1) and res["per_network"].shape == (m, 32, 1) and res["ibs_per_network"].shape == (m, 1)
    check({"curves": res["curves"], "brier": res["brier"].T, "per_network": res["per_network"].transpose(0, 2, 1), "mean_weight": res["mean_weight"].T},
          p._ensure_chain().forward_many(np.stack(p.vectors), X=X), Y, ts, None, None)
    assert 0 < res["ibs"][0] < 0.25 and res["n_bad"] == 0 and res["q05"][0] <= res["q50"][0] <= res["q95"][0]
    assert np.isclose(res["ibs"][0], np.sum(0.5 * (res["brier"][1:, 0] + res["brier"][:-1, 0]) * np.diff(ts)) / (ts[-1] - ts[0]), rtol=1e-14, atol=0)


def test_refusals(native):
    """what tbnn_ensemble_brier itself refuses (the grid's and the targets' refusals: tests/test_brier_host.py), with nothing written"""
    ch = native.Chain([(2, 4, native.ACT_TANH, 0), (4, 1, native.ACT_NONE, 0)], likelihood=native.LIK_FIXED_GAUSSIAN, kernel=native.KERNEL_GENERIC)
    th, X, Y, ts, out = np.zeros((4097, ch.P), dtype=np.float32), np.ones((3, 2), dtype=np.float32), np.float32([[1], [-2], [3]]), np.float64([1, 2]), np.full(2, 7.0)

    def refused(why, m=2, lik=native.LIK_WEIBULL, Yb=Y, gy=None, o=out):
        rc = native.lib.tbnn_ensemble_brier(ch._h, native._p(th), m, ch.P, lik, None, 1, native._p(X), native._p(Yb), 3, native._p(gy), 0,
                                            native._pd(ts), 2, native._pd(o), None, None, None)
        assert rc < 0 and why in native.lib.tbnn_last_error().decode() and np.all(out == 7.0), (why, rc, native.lib.tbnn_last_error())

    refused("needs the shape")
    ch.set_lik_df(K)
    for why, kw in [("every output is null", dict(o=None)), ("without their targets", dict(Yb=None)), ("no survival function", dict(lik=native.LIK_POISSON)),
                    ("exceeds 4096 networks", dict(m=4097)), ("G_Y with n_g < 1", dict(gy=Y))]:
        refused(why, **kw)
    ch.close()
