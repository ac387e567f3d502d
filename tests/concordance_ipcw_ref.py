"""Uno's IPCW concordance index of tbnn_ensemble_concordance_ipcw (include/tbnn.h) restated from its pair definition in plain fp64 NumPy:
every ordered pair of rows, no sort and no suffix.  Boolean [n, n] matrices for small n, a loop over the event rows beyond that."""
import numpy as np


def concordance_ipcw(y, s, times, omega):
    """one column: y [n] signed targets; s [n] the scores, compared in their own dtype; omega [n] the weights 1 / G(t-)^2
    -> (C [T], D [T], the cases [T])"""
    y, s, omega = np.asarray(y), np.asarray(s), np.asarray(omega, dtype=np.float64)
    t, e, times = np.abs(y.astype(np.float64)), y > 0, np.asarray(times, dtype=np.float64)
    n = y.size
    if n <= 4096:
        comp = e[:, None] & ((t[:, None] < t[None]) | ((t[:, None] == t[None]) & ~e[None]))
        count = 2 * (comp & (s[:, None] < s[None])).sum(axis=1) + (comp & (s[:, None] == s[None])).sum(axis=1)
        partners = comp.sum(axis=1)
    else:
        count, partners = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for i in np.flatnonzero(e):
            comp = (t[i] < t) | ((t[i] == t) & ~e)
            count[i], partners[i] = 2 * np.sum(comp & (s[i] < s)) + np.sum(comp & (s[i] == s)), comp.sum()
    case = e[None] & (t[None] < times[:, None])                             # [T, n]: strict
    N = np.array([np.sum(omega[c] * count[c]) for c in case])
    D = np.array([np.sum(omega[c] * partners[c]) for c in case])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((D > 0) & ~np.isnan(s).any(), N / (2 * D), np.nan), D, case.sum(axis=1)
