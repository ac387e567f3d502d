"""The cumulative/dynamic time-dependent AUC of tbnn_ensemble_auc (include/tbnn.h) restated from its pair definition in plain fp64 NumPy:
O(n^2 T) compares, every (case, control) pair at every grid time, the cases taken in blocks so that a block's compare matrix stays small."""
import numpy as np


def auc(y, s, times, omega):
    """one column: y [n] signed targets; s the scores, LARGER for a later event (a network's outputs [n], the same at every time, or the
    mixture's survival probabilities [T, n]); omega [n] the case weights 1 / G(t-) -> (auc [T], W [T], the controls [T])"""
    y, s, omega = np.asarray(y), np.asarray(s), np.asarray(omega, dtype=np.float64)
    t, times = np.abs(y.astype(np.float64)), np.asarray(times, dtype=np.float64)
    T, n = times.size, y.size
    ctrl = t[None] > times[:, None]                                          # [T, n]
    case = (y > 0)[None] & ~ctrl
    W, C = np.array([omega[c].sum() for c in case]), ctrl.sum(axis=1)
    sg = np.broadcast_to(s, (T, n))
    num, rows, block = np.zeros(T), np.flatnonzero(case[-1]), max(1, (1 << 22) // n)
    for a in range(0, rows.size, block):
        i = rows[a:a + block]
        for g in range(T):
            if g == 0 or s.ndim == 2:
                later = (sg[g][i, None] < sg[g][None]) + 0.5 * (sg[g][i, None] == sg[g][None])       # [block, n]: 1 concordant, 1/2 tied
            num[g] += np.sum(np.where(case[g, i], omega[i] * (later @ ctrl[g].astype(np.float64)), 0.0))
    ok = (case.sum(axis=1) > 0) & (C > 0) & ~np.isnan(sg).any(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ok, num / (W * C), np.nan), W, C
