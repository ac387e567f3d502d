"""The IPCW Brier score of tbnn_ensemble_brier (include/tbnn.h) in plain fp64 NumPy: the Kaplan-Meier estimate of the censoring time (events
leave the risk set first at equal times, factors multiplied in ascending time), the weights by selects, the Weibull survival probabilities."""
import numpy as np


def censoring_km(y):
    """y [n] signed targets -> (the distinct censoring times ascending, G just after each)"""
    t, cen = np.abs(np.asarray(y, dtype=np.float64)), np.asarray(y) < 0
    cs, c = np.unique(t[cen], return_counts=True)
    above = t.size - np.searchsorted(np.sort(t), cs, side="right")           # the rows with t > s; with c, the risk set at s
    return cs, np.cumprod(1.0 - c / (above + c))


def g_inv(km, x, left):
    """1 / G(x-) (left) or 1 / G(x), NaN where G is 0"""
    cs, cum = km
    g = np.concatenate([[1.0], cum])[np.searchsorted(cs, x, side="left" if left else "right")]
    with np.errstate(divide="ignore"):
        return np.where(g > 0, 1.0 / g, np.nan)


def weights(y, times, gy=None):
    """(w [T, n], I [T, n]) of one column: y [n] signed targets, gy the targets the censoring distribution comes from (None: y)"""
    km = censoring_km(y if gy is None else gy)
    t, times = np.abs(np.asarray(y, dtype=np.float64)), np.asarray(times, dtype=np.float64)
    alive = t[None] > times[:, None]
    w = np.where(alive, g_inv(km, times, False)[:, None], np.where((np.asarray(y) > 0)[None], g_inv(km, t, True)[None], 0.0))
    return w, alive.astype(np.float64)


def survival(f, k, times):
    """f fp32 [m, d_out, n] -> S [m, d_out, T, n] = exp(-exp(k (log tau - f))), k as the library holds it (an fp32)"""
    lt = np.log(np.asarray(times, dtype=np.float64))[None, None, :, None]
    with np.errstate(over="ignore"):
        return np.exp(-np.exp(float(np.float32(k)) * (lt - f.astype(np.float64)[:, :, None, :])))


def brier(y, S, times, gy=None):
    """one column: S [..., T, n] -> (the score [..., T], the mean weight [T])"""
    w, ind = weights(y, times, gy)
    return np.mean(w * (ind - S) ** 2, axis=-1), np.mean(w, axis=-1)
