"""CPU: the host half of the IPCW Brier score -- tbnn_ipcw_weights (the Kaplan-Meier estimate of the censoring time, include/tbnn.h
tbnn_ensemble_brier) against tests/brier_ref.py with ==: both multiply the factors 1 - c / r in ascending time, so the bits agree -- and
predictor.brierScore's grid default, refusals and IBS on a stub chain."""
import numpy as np
import pytest

import brier_ref as br
from test_predictive_host import HYPERS, X as SX, stub_predictor
from test_weibull_host import WeibullStubChain

TIES = [2, -2, 3, -3, -3, 5, 1, -1, 4, -6, 3]        # events and censored rows at 1, 2 and 3; the last time censored: G reaches 0
# name: (Y columns, grid, G_Y columns or None)
CASES = {"ties_and_grid_on_rows": ([TIES, TIES[::-1]], [0.5, 1, 2, 3, 4.5, 6, 7], None), "all_events": ([[1, 2, 2, 4]], [1, 3], None),
         "all_censored": ([[-1, -2, -2, -4]], [0.5, 2, 4, 5], None),
         "separate_G": ([TIES, TIES[::-1]], [1, 2.5, 6], [[-1, 2, -2, -2, 7, -8], [3, -3, 1, -0.5, 9, 9]])}


@pytest.mark.parametrize("name", list(CASES))
def test_ipcw_weights(native, name):
    cols, times, gcols = CASES[name]
    Y, times = np.asarray(cols, dtype=np.float32).T, np.asarray(times, dtype=np.float64)
    GY = None if gcols is None else np.asarray(gcols, dtype=np.float32).T
    row, tim = native.ipcw_weights(Y, times, GY)
    assert row.shape == (Y.shape[1], Y.shape[0]) and tim.shape == (Y.shape[1], len(times))
    for o in range(Y.shape[1]):
        gy = None if GY is None else GY[:, o]
        t = np.abs(Y[:, o].astype(np.float64))
        km = br.censoring_km(Y[:, o] if gy is None else gy)
        assert np.array_equal(row[o], br.g_inv(km, t, True), equal_nan=True) and np.array_equal(tim[o], br.g_inv(km, times, False), equal_nan=True), o
        # the weights the kernel selects from the two arrays are the reference's
        w = np.where(t[None] > times[:, None], tim[o][:, None], np.where(Y[None, :, o] > 0, row[o][None], 0.0))
        assert np.array_equal(w, br.weights(Y[:, o], times, gy)[0], equal_nan=True), o
    if name == "all_events":
        assert np.all(row == 1.0) and np.all(tim == 1.0)
    if name == "all_censored":                                            # G(4) = 0: NaN in the array, needed by nobody here
        g2 = (1.0 - 1.0 / 4.0) * (1.0 - 2.0 / 3.0)
        assert np.isnan(tim[0, 2]) and np.isnan(tim[0, 3]) and tim[0, 0] == 1.0 and tim[0, 1] == 1.0 / g2 and row[0, 3] == 1.0 / g2
    if name == "ties_and_grid_on_rows":                                   # the event at 2 leaves first: G(2) = (1 - 1/10)(1 - 1/8)
        assert tim[0, 2] == 1.0 / ((1.0 - 1.0 / 10.0) * (1.0 - 1.0 / 8.0)) and np.isnan(tim[0, 5]) and np.isfinite(row[0, 9])
        assert np.mean(br.weights(Y[:, 0], times[:5])[0], axis=1) == pytest.approx(1.0, abs=1e-14)


def test_ipcw_refusals(native):
    Y = np.asarray([TIES], dtype=np.float32).T
    bad = [(Y, t) for t in ([], [0.0, 1.0], [-1.0], [1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [np.inf], np.arange(1, 258))]
    bad += [args for v in (0.0, np.nan, np.inf) for Yb in [np.where(np.arange(11)[:, None] == 3, np.float32(v), Y)] for args in ((Yb, [1.0]), (Y, [1.0], Yb))]
    for args in bad:
        with pytest.raises(native.TbnnError, match="T must be|not finite, not > 0 or not above|not a finite, nonzero time"):
            native.ipcw_weights(*args)


class BrierStubChain(WeibullStubChain):
    """answers ensemble_brier with brier = tau and per_network = i + tau^2, whose integrals are known"""

    def ensemble_brier(self, thetas, times, **kw):
        self.calls.append((np.asarray(thetas), np.asarray(times), kw.get("Y"), kw))
        m, ts = len(thetas), np.asarray(times, dtype=np.float64)
        out = {"brier": np.tile(ts, (self.d_out, 1)), "mean_weight": np.ones((self.d_out, ts.size)),
               "per_network": np.arange(m)[:, None, None] + np.tile(ts ** 2, (m, self.d_out, 1))}
        if kw.get("curves"):
            out["curves"] = np.zeros((ts.size, self.d_out, np.asarray(kw["X"]).shape[0]))
        return out


def test_brier_score_wrapper():
    from tensorbnn_amd.likelihood import GammaLikelihood, WeibullLikelihood
    p = stub_predictor(WeibullLikelihood(shape=3.0), HYPERS)
    p._chain = BrierStubChain()
    Y = WeibullLikelihood.encode(np.array([[1.0, 2.0], [3.0, 9.0], [5.0, 7.0]]), np.array([[True, True], [True, False], [False, True]]))
    res = p.brierScore(SX, Y, n=2)
    th, ts, _yy, kw = p._chain.calls[-1]
    assert np.array_equal(ts, np.linspace(*np.quantile([1.0, 2.0, 3.0, 7.0], [0.1, 0.9]), 32)) and np.array_equal(res["times"], ts)
    assert np.array_equal(th[:, 0], [0, 2, 4]) and kw["likelihood"] == 16 and p._chain.df == [3.0] and kw["censoringY"] is None
    assert res["brier"].shape == res["mean_weight"].shape == (32, 2) and res["per_network"].shape == (3, 32, 2) and "curves" not in res
    assert np.allclose(res["ibs"], 0.5 * (ts[0] + ts[-1]), rtol=1e-14)                          # the trapezoid is exact on a line
    exact = (ts[-1] ** 3 - ts[0] ** 3) / 3.0 / (ts[-1] - ts[0])
    assert np.allclose(res["ibs_per_network"], np.arange(3)[:, None] + exact, rtol=1e-3) and res["ibs_per_network"].shape == (3, 2)
    assert np.allclose(res["q50"], 1.0 + exact, rtol=1e-3) and res["n_bad"] == 0
    assert np.array_equal(res["n_events"], [2, 2]) and np.array_equal(res["n_censored"], [1, 1])
    one = p.brierScore(SX, Y, times=[2.0], censoringY=Y[:2], curves=True, weights=[1, 0, 2], n=2)
    assert np.all(np.isnan(one["ibs"])) and one["n_bad"] == 6 and one["curves"].shape == (1, 2, 3) and np.all(np.isnan(one["mean"]))
    assert p._chain.calls[-1][3]["censoringY"] is not None and np.array_equal(p._chain.calls[-1][3]["weights"], np.float32([1, 0, 2]))
    n_calls = len(p._chain.calls)
    with pytest.raises(ValueError, match="at least two distinct event times"):
        p.brierScore(SX, -np.abs(Y))
    with pytest.raises(ValueError, match="needs a WeibullLikelihood"):
        p.brierScore(SX, Y, likelihood=GammaLikelihood(shape=2.0))
    assert len(p._chain.calls) == n_calls
