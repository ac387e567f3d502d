"""The CRPS of a mixture of count distributions, restated in plain fp64 with SciPy (the definition of tbnn_ensemble_count_crps in
include/tbnn.h), and the cases tests/test_gpu_count_crps.py and tools/count_crps_ref_fig.py share."""
import numpy as np
from scipy import stats

POIS, NEGB = 5, 10
SPREAD = np.log([0.05, 300.0, 2.0, 4000.0, 0.07, 31.0, 700.0, 5.0, 1500.0, 0.5, 90.0, 12.0, 2500.0, 1.0, 180.0, 45.0, 3.0])   # tiny rates, a window of several tiles, disjoint windows (2, 4000), fillers


def count_crps_ref(f, w, y, lik, r=None):
    """f [m] log-rates, w [m] weights, y [n] targets -> (crps, error, spread) [n] each, and n_k.  K: where every component's sf is below
    1e-18 x max(1, mean), searched from 40 standard deviations past the largest mean (or target) by doubling the distance"""
    om = np.asarray(w, np.float64) / np.sum(w, dtype=np.float64)
    mu = np.exp(np.asarray(f, np.float64))[om > 0]
    om, d = om[om > 0], stats.poisson(mu) if lik == POIS else stats.nbinom(r, r / (r + mu))
    K = int(max(np.max(mu + 40 * d.std()), np.max(y), 1)) + 1
    while np.any(d.sf(K) >= 1e-18 * np.maximum(1.0, mu)):
        K *= 2
    k = np.arange(K + 1)[:, None]
    F, S = d.cdf(k) @ om, d.sf(k) @ om
    upper = np.asarray(y, np.float64)[None, :] <= k                      # [K + 1, n]: 1{y <= k}
    error = np.where(upper, S[:, None], F[:, None]).sum(0)
    crps = (np.where(upper, S[:, None], F[:, None]) ** 2).sum(0)
    spread = np.full(len(y), (F * S).sum())
    return crps, error, spread, K + 1


def poisson_error_closed(f, w, y):
    """E|Y - y| of the Poisson mixture for integer y >= 0: sum_i omega_i [2 (y F_i(y) - mu_i F_i(y - 1)) + mu_i - y]"""
    om, mu = np.asarray(w, np.float64) / np.sum(w, dtype=np.float64), np.exp(np.asarray(f, np.float64))
    return sum(o * (2 * (y * stats.poisson.cdf(y, m) - m * stats.poisson.cdf(y - 1, m)) + m - y) for o, m in zip(om, mu))


def log_rates(m, d_out, shift=0.0):
    """[m, d_out] fp32: the spread, rotated by one per output, plus shift"""
    return np.stack([np.roll(SPREAD, -j)[:m] for j in range(d_out)], 1).astype(np.float32) + np.float32(shift)


def targets(f, rows):
    """[rows, d_out] fp32, per row in turn: 0, a negative value, a non-integer, below every window, inside, above every window"""
    mu = np.exp(f.astype(np.float64))                                    # [m, d_out]
    top, mid = mu.max(0), np.median(mu, 0)
    kinds = [0 * top, 0 * top - 2.5, mid + 0.37, np.maximum(1.0, np.floor(mu.min(0) / 4)), np.floor(mid) + 1, np.floor(top + 8 * np.sqrt(top) + 30)]
    return np.stack([kinds[i % 6] + (i // 6 if i % 6 >= 4 else 0) for i in range(rows)]).astype(np.float32)
