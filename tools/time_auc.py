"""Times the cumulative/dynamic time-dependent AUC of a survival ensemble on the device (Chain.ensemble_auc: tbnn_ensemble_auc, the pair
kernel k_ens_auc) for 256 networks of 5-50-50-50-1 over 10,000 and 100,000 rows at T = 32 times, shape 1.5, about 35 % censored, against
  forward_many_ms        Chain.forward_many alone: the 256 forward passes and their copy to the host;
  concordance_ms         Chain.ensemble_concordance at the same shape: the same pair compares per network, unweighted, no grid;
  host_scaled_ms         the host route: forward_many, then tests/auc_ref.py per network, MEASURED ON HOST_NETS NETWORKS AND THE FIRST
                         HOST_ROWS ROWS AND EXTRAPOLATED by (m / HOST_NETS) (n / HOST_ROWS)^2, plus the measured forward_many.
The host figure is a SINGLE RUN without a warm-up (its spread is not measured).
Each device figure: one warm-up call, then the median of five calls on a host clock -- every call returns after its stream work has
completed (include/tbnn.h) -- so auc_ms holds both passes over the forward kernels, the host's Kaplan-Meier and sort, the kernels and the
copies; auc_mixture_only_ms leaves the per-network pass out.  Prints one JSON line per shape with the library's build id and the largest
difference between the device and the host route on what that ran.  Needs a gfx950 device; there is no fallback."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from tensorbnn_amd import _native as nat                     # noqa: E402
import auc_ref as ar                                         # noqa: E402

M, T, K = 256, 32, 1.5
HOST_NETS, HOST_ROWS = 2, 4000
DIMS = [5, 50, 50, 50, 1]


def median_of(fn, runs=5):
    fn()                                                   # warm-up: code objects loaded, pooled buffers grown
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    if nat.device_count() < 1:
        sys.exit("time_auc: no gfx950 device")
    for n in (10_000, 100_000):
        rng = np.random.default_rng(0)
        X = rng.standard_normal((n, DIMS[0])).astype(np.float32)
        base = np.concatenate([(rng.standard_normal(o * i + o) * (2.0 / i) ** 0.5) for i, o in zip(DIMS[:-1], DIMS[1:])])
        thetas = (base[None, :] + 0.1 * rng.standard_normal((M, base.size))).astype(np.float32)
        layers = [(DIMS[i], DIMS[i + 1], nat.ACT_RELU if i < len(DIMS) - 2 else nat.ACT_NONE, 0) for i in range(len(DIMS) - 1)]
        ch = nat.Chain(layers, likelihood=nat.LIK_FIXED_GAUSSIAN, fixed_sd=0.3)          # the predictor's forward chain: the shape is set on it
        ch.set_lik_df(K)
        f = ch.forward_many(thetas, X=X)
        lam = np.exp(f[:, 0].astype(np.float64).mean(axis=0))
        t_ev, t_ce = lam * rng.weibull(K, n), 1.5 * lam * rng.weibull(K, n)
        Y = np.where(t_ev <= t_ce, t_ev, -t_ce).astype(np.float32)[:, None]
        times = np.linspace(*np.quantile(t_ev, [0.1, 0.9]), T)
        call = lambda **kw: ch.ensemble_auc(thetas, times, Y=Y, X=X, likelihood=nat.LIK_WEIBULL, **kw)
        res = {"rows": n, "networks": M, "times": T, "kernel": ch.kernel_name, "build_id": nat.build_id(), "censored_share": float(np.mean(Y < 0)),
               "pairs_per_network": n * (n - 1) // 2}
        got = call()
        res["auc_ms"] = round(1e3 * median_of(call), 3)
        res["auc_mixture_only_ms"] = round(1e3 * median_of(lambda: call(per_network=False)), 3)
        res["concordance_ms"] = round(1e3 * median_of(lambda: ch.ensemble_concordance(thetas, Y=Y, X=X)), 3)
        res["forward_many_ms"] = round(1e3 * median_of(lambda: ch.forward_many(thetas, X=X)), 3)
        # the host route on a corner of the problem: its own weights and scores, so its own answer, compared with the device's on that corner
        ys, xs = Y[:HOST_ROWS], X[:HOST_ROWS]
        small = ch.ensemble_auc(thetas[:HOST_NETS], times, Y=ys, X=xs, likelihood=nat.LIK_WEIBULL)
        omega = nat.ipcw_weights(ys, times)[0][0]
        t0 = time.perf_counter()
        host = np.stack([ar.auc(ys[:, 0], f[i, 0, :HOST_ROWS], times, omega)[0] for i in range(HOST_NETS)])
        res["host_nets"], res["host_rows"] = HOST_NETS, HOST_ROWS
        res["host_scaled_ms"] = round(1e3 * (time.perf_counter() - t0) * (M / HOST_NETS) * (n / HOST_ROWS) ** 2 + res["forward_many_ms"], 1)
        res["iauc"] = float(np.sum(0.5 * (got["auc"][0, 1:] + got["auc"][0, :-1]) * np.diff(times)) / (times[-1] - times[0]))
        res["max_diff_per_network"] = float(np.nanmax(np.abs(small["per_network"][:, 0] - host)))
        print(json.dumps(res), flush=True)
        ch.close()


if __name__ == "__main__":
    main()
