"""Harrell's concordance index restated from its pair definition in plain NumPy (tbnn_ensemble_concordance, include/tbnn.h): O(n^2) boolean
matrices over the times, flags and scores, int64 sums.  No sort and no suffix: independent of the library's staging."""
import numpy as np


def concordance_ref(y, s):
    """y [n]: signed targets (|y| the time, y > 0 an event); s [n]: scores, compared in their own dtype -> (comparable, concordant, tied);
    concordant = tied = -1 with a NaN among the scores"""
    y, s = np.asarray(y), np.asarray(s)
    t, e = np.abs(y), y > 0
    comp = e[:, None] & ((t[:, None] < t[None, :]) | ((t[:, None] == t[None, :]) & ~e[None, :]))
    if np.isnan(s).any():
        return int(comp.sum(dtype=np.int64)), -1, -1
    return (int(comp.sum(dtype=np.int64)), int((comp & (s[:, None] < s[None, :])).sum(dtype=np.int64)),
            int((comp & (s[:, None] == s[None, :])).sum(dtype=np.int64)))


def c_index(comparable, concordant, tied):
    return (concordant + 0.5 * tied) / comparable if comparable > 0 and concordant >= 0 else float("nan")
