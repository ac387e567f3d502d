"""Split-R-hat and effective sample size in fp64 NumPy, restated from the definition in include/tbnn.h (tbnn_ensemble_diagnostics) and
independent of the kernel: the reference of tests/test_diagnostics_host.py and tests/test_gpu_diagnostics.py.

An element's m = C S values t[c][s] are chain-major along axis 0 (network i = c S + s); every trailing axis is an axis of elements.
  split      N = S // 2; chain c gives the split chains 2 c (draws 0 .. N-1) and 2 c + 1 (draws S-N .. S-1): K = 2 C
  means      mu_k, d[k][s] = x[k][s] - mu_k
  autocov    a_k(l) = (1/N) sum_{s <= N-1-l} d[k][s] d[k][s+l], A(l) = mean_k a_k(l)
  variances  Wv = A(0) N / (N-1), Bn = var(mu_k, ddof=1), Vp = Wv (N-1) / N + Bn
  rhat       sqrt(Vp / Wv);  rho(l) = 1 - (Wv - A(l)) / Vp
  ess        P_0 = 1 + rho(1); P_k = rho(2k) + rho(2k+1) while 2k+1 <= N-1, stop at the first P_k not > 0 (unused), P'_k = min(P'_{k-1}, P_k);
             tau = max(-1 + 2 sum P'_k, 1 / log10(K N)); ess = K N / tau
  undefined  a NaN among the values, or Wv not > 0: rhat = ess = NaN
The draws lie along the FIRST axis of every array summed here, so NumPy adds them one after the other, in s order (and the split chains in k
order), as the definition says -- not pairwise.

margin: the smallest |P_k| over every P_k an element met up to and including its stop (P_0 among them), +inf for an undefined element --
how far the element is from the one discontinuity of the ESS, the sign decision of a P_k."""
import numpy as np


def diag_ref(t, chains=1):
    """t [m, ...] -> (rhat, ess, margin), each float64 of shape t.shape[1:]"""
    t = np.asarray(t)
    m, shape = t.shape[0], t.shape[1:]
    C = int(chains)
    if C < 1 or m % C or m // C < 8:
        raise ValueError("m must be chains x draws with at least 8 draws per chain")
    S = m // C
    N, K = S // 2, 2 * C
    x = t.reshape(C, S, -1).astype(np.float64)
    nan = np.isnan(x).any(axis=(0, 1))
    # [N, K, E]: s first, k = 2 c + h
    xs = np.stack([x[:, :N], x[:, S - N:]], axis=1).reshape(K, N, -1).transpose(1, 0, 2).copy()
    with np.errstate(all="ignore"):
        mu = xs.sum(axis=0) / N                                         # [K, E]
        d = xs - mu

        def A(l):
            return ((d[:N - l] * d[l:]).sum(axis=0) / N).sum(axis=0) / K

        Wv = A(0) * N / (N - 1)
        mbar = mu.sum(axis=0) / K
        Bn = ((mu - mbar) ** 2).sum(axis=0) / (K - 1)
        Vp = Wv * (N - 1) / N + Bn
        undefined = nan | ~(Wv > 0)
        rhat = np.sqrt(Vp / Wv)

        def rho(l):
            return 1.0 - (Wv - A(l)) / Vp

        P = 1.0 + rho(1)
        total, prev, margin = P.copy(), P.copy(), np.abs(P)
        live = ~undefined
        k = 1
        while 2 * k + 1 <= N - 1 and live.any():
            P = rho(2 * k) + rho(2 * k + 1)
            margin = np.where(live, np.minimum(margin, np.abs(P)), margin)
            live = live & (P > 0)
            prev = np.where(live, np.minimum(prev, P), prev)
            total = np.where(live, total + prev, total)
            k += 1
        tau = np.maximum(-1.0 + 2.0 * total, 1.0 / np.log10(K * N))
        ess = K * N / tau
    rhat = np.where(undefined, np.nan, rhat)
    ess = np.where(undefined, np.nan, ess)
    margin = np.where(undefined, np.inf, margin)
    return rhat.reshape(shape), ess.reshape(shape), margin.reshape(shape)
