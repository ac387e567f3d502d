"""Pareto-smoothed importance-sampling leave-one-out cross-validation and WAIC in fp64 NumPy, restated from the definition in include/tbnn.h
(tbnn_ensemble_loo) and independent of the kernel: the reference of tests/test_psis_host.py and tests/test_gpu_loo.py.  It is the R package
loo's algorithm (Vehtari, Gelman, Gabry 2017; the fit of Zhang and Stephens 2009 with loo's priors), continuous in its inputs.

l [m, n]: the log-likelihood of row r under network i.  Per row (a column of l):
  lppd      logsumexp_i(l_i) - log m;  p_waic = sum_i (l_i - mean l)^2 / (m - 1) (m = 1: NaN)
  ratios    x_i = -l_i - max_j(-l_j)
  tail      M = ceil(min(0.2 m, 3 sqrt(m / r_eff))); sorted v_(1) <= ... <= v_(m): the tail is v_(m-M+1 .. m), the cutoff c = v_(m-M)
  raw       if M < 5, or v_(m) - v_(m-M+1) = 0, or y_(q) is not > 0: k = +inf, lw = x
  fit       y_j = exp(v_(m-M+j)) - exp(c); q = floor(M / 4 + 1/2), G = 30 + floor(sqrt M); b_g = 1 / y_(M) + (1 - sqrt(G / (g - 1/2))) / (3 y_(q));
            kappa_g = mean_j log1p(-b_g y_j); L_g = M (log(-b_g / kappa_g) - kappa_g - 1); w_g = exp(L_g - logsumexp L);
            b = sum_g b_g w_g; kappa = mean_j log1p(-b y_j); sigma = -kappa / b; k = (M kappa + 5) / (M + 10)
  smoothing the j-th smallest tail value becomes min(log(exp(c) + sigma expm1(-k log1p(-p_j)) / k), 0), p_j = (j - 1/2) / M
            (|k| < 2^-52: -sigma log1p(-p_j) for the quotient); k or sigma not finite: lw = x, and the k obtained
  loo       elpd_loo = logsumexp_i(lw_i + l_i) - logsumexp_i(lw_i)
  undefined a NaN or infinity among the l_i: NaN in all four
The sort is stable, so of the values equal to the cutoff the ones with the largest network indices are the tail's members; only the multiset
of values enters the result.  The networks lie along the FIRST axis of every array summed here."""
import math

import numpy as np
from scipy.special import logsumexp


def tail_length(m, r_eff=1.0):
    return int(math.ceil(min(0.2 * m, 3.0 * math.sqrt(m / r_eff))))


def gpd_fit(y):
    """y [M, n], ascending along axis 0, y_(q) > 0 -> (k, sigma), each [n]"""
    y = np.asarray(y, dtype=np.float64)
    M = y.shape[0]
    q = int(math.floor(M / 4.0 + 0.5))
    G = 30 + int(math.floor(math.sqrt(M)))
    g = np.arange(1, G + 1, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        b = 1.0 / y[-1] + (1.0 - np.sqrt(G / (g - 0.5))) / (3.0 * y[q - 1])                  # [G, n]
        kap = np.stack([np.log1p(-bg * y).sum(axis=0) / M for bg in b])                       # [G, n]
        L = M * (np.log(-b / kap) - kap - 1.0)
        w = np.exp(L - logsumexp(L, axis=0))
        bb = (b * w).sum(axis=0)
        kappa = np.log1p(-bb * y).sum(axis=0) / M
        return (M * kappa + 5.0) / (M + 10.0), -kappa / bb


def psis_ref(l, r_eff=1.0):
    """l [m, n] -> dict of float64 [n]: elpd_loo, pareto_k, lppd, p_waic"""
    l = np.asarray(l, dtype=np.float64)
    m, n = l.shape
    bad = ~np.isfinite(l).all(axis=0)
    ls = np.where(bad, 0.0, l)                                   # (an undefined row is computed on zeros and overwritten below)
    lppd = logsumexp(ls, axis=0) - math.log(m)
    p_waic = ((ls - ls.sum(axis=0) / m) ** 2).sum(axis=0) / (m - 1) if m > 1 else np.full(n, np.nan)
    x = (-ls - (-ls).max(axis=0)) + 0.0
    M = tail_length(m, r_eff)
    order = np.argsort(x, axis=0, kind="stable")
    v = np.take_along_axis(x, order, axis=0)
    k = np.full(n, np.inf)
    lw = x.copy()
    if M >= 5:
        c, tail = v[m - M - 1], v[m - M:]
        ec = np.exp(c)
        y = np.exp(tail) - ec
        q = int(math.floor(M / 4.0 + 0.5))
        ok = (tail[-1] - tail[0] > 0) & (y[q - 1] > 0)
        if ok.any():
            kf, sf = gpd_fit(y[:, ok])
            k[ok] = kf
            fin = np.isfinite(kf) & np.isfinite(sf)
            z = np.log1p(-(np.arange(1, M + 1) - 0.5) / M)[:, None]
            with np.errstate(all="ignore"):
                qv = np.where(np.abs(kf) < 2.0 ** -52, -sf * z, sf * np.expm1(-kf * z) / kf)
                sm = np.minimum(np.log(ec[ok] + qv), 0.0)
            cols = np.flatnonzero(ok)[fin]
            lw[order[m - M:, cols], cols] = sm[:, fin]
    elpd = logsumexp(lw + ls, axis=0) - logsumexp(lw, axis=0)
    out = {"elpd_loo": elpd, "pareto_k": k, "lppd": lppd, "p_waic": p_waic}
    for a in out.values():
        a[bad] = np.nan
    return out
