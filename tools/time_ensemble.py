"""Times the routes to an ensemble's predictive moments and quantiles on the GPU:
  (a) Chain.forward_many, then np.mean / np.var in fp64 on the host (every prediction crosses to the host: 4 m d_out n bytes);
  (b) Chain.ensemble_moments (the reduction on the device: 16 d_out n bytes cross) -- also the forward-only floor of (d);
  (c) Chain.forward_many, then np.quantile(axis=0) at probs = [0.05, 0.5, 0.95] on the host (on the fp32 array as it comes: the cheapest
      form of that route; max_abs_diff_quantiles compares (d) with np.quantile of the fp64 cast, outside the timing);
  (d) Chain.ensemble_quantiles at the same probabilities (the selection on the device: 24 d_out n bytes cross);
  (e) Chain.forward_many, then the vectorised fp64 restatement of split-R-hat and the effective sample size on the host (tests/diag_ref.py),
      the m networks read as 4 chains of m / 4 draws (AR(1) walks around one base vector, so that the lag loop has work to do);
  (f) Chain.ensemble_diagnostics over the same thetas (the estimators on the device: 16 d_out n bytes cross).
  (g) Chain.forward_many, then the predictive quantiles at the same three probabilities on the host: a vectorised NumPy / SciPy bisection
      of the definition in include/tbnn.h (F(y) = mean_i ndtr((y - f_i) / s_i) = p between the smallest and the largest f_i + s_i z_p, 56
      halvings), per-network sd's from 0.05 to 0.2.  The bisection runs over the first HOST_ROWS rows, ONCE, and its time is scaled to all n
      rows (it is linear in them; at the headline shape the full run takes minutes of a GPU box's time); the forward_many part is timed
      over all rows like the other routes;
  (h) Chain.ensemble_predictive at the same probabilities and sd's (the inversion on the device: 24 d_out n bytes cross).
Shapes: the headline 5-50-50-50-1 with m = 256 networks over n = 100,000 rows, and the tutorial 784-20-20-1 with m = 256, n = 12,000.
Each route: one warm-up call, then the median of five calls on a host clock -- every call returns after its stream work has completed
(include/tbnn.h), so the clock covers the forward passes, the copies and, for (a) and (c), the host's pass.  Prints one JSON line per shape
with the library's build id.  Needs a gfx950 device; there is no fallback."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from tensorbnn_amd import _native as nat                     # noqa: E402
from diag_ref import diag_ref                                # noqa: E402

CHAINS = 4
HOST_ROWS = 2_000

SHAPES = {
    "headline": ([5, 50, 50, 50, 1], nat.ACT_RELU, nat.ACT_NONE, nat.LIK_GAUSSIAN, 256, 100_000),
    "tutorial": ([784, 20, 20, 1], nat.ACT_RELU, nat.ACT_SIGMOID, nat.LIK_BERNOULLI, 256, 12_000),
}


def lib_rhat_only(ch, thetas, X):
    """tbnn_ensemble_diagnostics with ess_out NULL: the element leaves after lag 0"""
    import ctypes as C
    rhat = np.empty((ch.d_out, X.shape[0]), dtype=np.float64)
    rc = nat.lib.tbnn_ensemble_diagnostics(ch._h, nat._p(thetas), thetas.shape[0], thetas.shape[1], CHAINS, nat.XFORM_NONE, 1.0, 0.0, 1, nat._p(X),
                                           X.shape[0], rhat.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert rc == 0, nat.lib.tbnn_last_error()
    return rhat


def host_predictive_quantiles(f, sd, probs, halvings=56):
    """f fp32 [m, d_out, rows], sd [m] -> float64 [n_probs, d_out, rows]: the upper end of the bisected bracket"""
    from scipy.special import ndtr, ndtri
    f = f.astype(np.float64)
    s = np.asarray(sd, dtype=np.float64)[:, None, None]
    out = []
    for p in probs:
        comp = f + s * ndtri(p)
        lo, hi = comp.min(axis=0) - 1e-9, comp.max(axis=0) + 1e-9
        for _ in range(halvings):
            mid = lo + 0.5 * (hi - lo)
            ge = ndtr((mid[None] - f) / s).mean(axis=0) >= p
            hi, lo = np.where(ge, mid, hi), np.where(ge, lo, mid)
        out.append(hi)
    return np.stack(out)


def median_of(fn, runs=5):
    fn()                                                   # warm-up: code objects loaded, pooled buffers grown
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def walks(rng, P, chains, draws):
    """thetas [chains draws, P], chain-major: AR(1) walks (phi 0 .. 0.9 over the chains) of small steps around one base vector"""
    base = rng.standard_normal(P) * 0.3
    out = np.empty((chains, draws, P), dtype=np.float32)
    for c in range(chains):
        phi = 0.9 * c / max(chains - 1, 1)
        dev = rng.standard_normal(P)
        for s in range(draws):
            dev = phi * dev + np.sqrt(1 - phi * phi) * rng.standard_normal(P)
            out[c, s] = base + 0.03 * dev
    return out.reshape(chains * draws, P)


def main():
    if nat.device_count() < 1:
        sys.exit("time_ensemble: no gfx950 device")
    for name, (dims, act, last, lik, m, n) in SHAPES.items():
        layers = [(dims[i], dims[i + 1], act if i < len(dims) - 2 else last, 0) for i in range(len(dims) - 1)]
        ch = nat.Chain(layers, likelihood=lik)
        rng = np.random.default_rng(0)
        X = (rng.standard_normal((n, dims[0])) / np.sqrt(max(dims[0] / 16.0, 1.0))).astype(np.float32)
        thetas = (rng.standard_normal((m, ch.P)) * 0.3).astype(np.float32)

        def host_route():
            f = ch.forward_many(thetas, X=X).astype(np.float64)
            return f.mean(axis=0), f.var(axis=0)

        ta, (mean_a, var_a) = median_of(host_route)
        tb, (mean_b, var_b) = median_of(lambda: ch.ensemble_moments(thetas, X=X))
        probs = [0.05, 0.5, 0.95]
        tc, _ = median_of(lambda: np.quantile(ch.forward_many(thetas, X=X), probs, axis=0))
        td, q_d = median_of(lambda: ch.ensemble_quantiles(thetas, probs, X=X))
        q_c = np.quantile(ch.forward_many(thetas, X=X).astype(np.float64), probs, axis=0)
        walk = walks(rng, ch.P, CHAINS, m // CHAINS)
        te, (rhat_e, ess_e, _margin) = median_of(lambda: diag_ref(ch.forward_many(walk, X=X), CHAINS))
        tf, (rhat_f, ess_f) = median_of(lambda: ch.ensemble_diagnostics(walk, chains=CHAINS, X=X))
        tr, _ = median_of(lambda: lib_rhat_only(ch, walk, X))
        sd = np.linspace(0.05, 0.2, m).astype(np.float32)
        hr = min(HOST_ROWS, n)
        f_host = ch.forward_many(thetas, X=X[:hr])
        t0 = time.perf_counter()
        q_g = host_predictive_quantiles(f_host, sd, probs)
        t_bis = (time.perf_counter() - t0) * n / hr
        t_fwd, _ = median_of(lambda: ch.forward_many(thetas, X=X))
        tg = t_fwd + t_bis
        th_, (q_h, _F, _Fb) = median_of(lambda: ch.ensemble_predictive(thetas, probs=probs, X=X, likelihood=nat.LIK_GAUSSIAN, sd=sd))
        print(json.dumps({"shape": name, "dims": dims, "kernel": ch.kernel_name, "m": m, "n": n, "build_id": nat.build_id(),
                          "forward_many_numpy_ms": round(ta * 1e3, 3), "ensemble_moments_ms": round(tb * 1e3, 3), "ratio": round(ta / tb, 2),
                          "bytes_to_host": {"forward_many": 4 * m * dims[-1] * n, "ensemble_moments": 16 * dims[-1] * n},
                          "forward_many_np_quantile_ms": round(tc * 1e3, 3), "ensemble_quantiles_ms": round(td * 1e3, 3),
                          "quantiles_ratio": round(tc / td, 2), "max_abs_diff_quantiles": float(np.abs(q_c - q_d).max()),
                          "forward_many_diag_ref_ms": round(te * 1e3, 3), "ensemble_diagnostics_ms": round(tf * 1e3, 3),
                          "diagnostics_ratio": round(te / tf, 2), "ensemble_diagnostics_rhat_only_ms": round(tr * 1e3, 3), "chains": CHAINS,
                          "max_rel_diff_rhat": float(np.nanmax(np.abs(rhat_f - rhat_e) / rhat_e)),
                          "max_rel_diff_ess": float(np.nanmax(np.abs(ess_f - ess_e) / ess_e)), "max_rhat": float(np.nanmax(rhat_f)),
                          "median_ess": float(np.nanmedian(ess_f)),
                          "forward_many_scipy_bisection_ms": round(tg * 1e3, 1), "host_bisection_rows": hr,
                          "host_bisection_ms_scaled_to_n": round(t_bis * 1e3, 1), "ensemble_predictive_ms": round(th_ * 1e3, 3),
                          "predictive_ratio": round(tg / th_, 1), "max_abs_diff_predictive": float(np.abs(q_h[:, :, :hr] - q_g).max()),
                          "max_abs_diff_mean": float(np.abs(mean_a - mean_b).max()), "max_abs_diff_var": float(np.abs(var_a - var_b).max())}),
              flush=True)
        ch.close()


if __name__ == "__main__":
    main()
