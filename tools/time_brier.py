"""Times the IPCW Brier score of a survival ensemble over a time grid on the device (Chain.ensemble_brier: tbnn_ensemble_brier, the kernel
k_ens_brier) for 256 networks of 5-50-50-50-1 over 10,000 and 100,000 rows at T = 32 times, shape 1.5, about 35 % censored, against
  forward_many_ms       Chain.forward_many alone: the 256 forward passes and their copy to the host;
  host_mixture_ms       the present host route to the mixture's score: predictor.survival's loop -- one Chain.ensemble_predictive CDF call
                        per time, each running all forward passes again -- followed by the NumPy restatement tests/brier_ref.py;
  host_per_network_scaled_ms  the host route to the per-network scores, which that loop cannot give: forward_many, then brier_ref's survival
                        probabilities and score per network, MEASURED ON HOST_NETS NETWORKS AND SCALED by m / HOST_NETS (the full
                        [m, T, n] fp64 array would take 6.5 GB at 1e5 rows), plus the measured forward_many.
The two host figures are SINGLE RUNS without a warm-up (their spread is not measured).
Each device figure: one warm-up call, then the median of five calls on a host clock -- every call returns after its stream work has
completed (include/tbnn.h) -- so brier_ms holds the forward passes, the host's Kaplan-Meier staging, the kernels and the copies, and
brier_curves_ms the same with the [T, 1, n] curves copied back too.  Prints one JSON line per shape with the library's build id and the
largest difference between the device and the host routes on what those ran.  Needs a gfx950 device; there is no fallback."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from tensorbnn_amd import _native as nat                     # noqa: E402
import brier_ref as br                                       # noqa: E402

M, T, K = 256, 32, 1.5
HOST_NETS = 8
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
        sys.exit("time_brier: no gfx950 device")
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
        call = lambda **kw: ch.ensemble_brier(thetas, times, Y=Y, X=X, likelihood=nat.LIK_WEIBULL, **kw)
        res = {"rows": n, "networks": M, "times": T, "kernel": ch.kernel_name, "build_id": nat.build_id(), "censored_share": float(np.mean(Y < 0)),
               "probabilities_per_call": M * n * T}
        got = call(curves=True)
        res["brier_ms"] = round(1e3 * median_of(call), 3)
        res["brier_curves_ms"] = round(1e3 * median_of(lambda: call(curves=True)), 3)
        res["brier_mixture_only_ms"] = round(1e3 * median_of(lambda: call(per_network=False)), 3)
        res["forward_many_ms"] = round(1e3 * median_of(lambda: ch.forward_many(thetas, X=X)), 3)

        def host_mixture():
            S = np.stack([1.0 - ch.ensemble_predictive(thetas, Y=np.full((n, 1), np.float32(t)), X=X, likelihood=nat.LIK_WEIBULL)[1][0] for t in times])
            return S, br.brier(Y[:, 0], S, times)[0]
        t0 = time.perf_counter()
        S_host, bs_host = host_mixture()
        res["host_mixture_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        t0 = time.perf_counter()
        net_host = br.brier(Y[:, 0], br.survival(f[:HOST_NETS], K, times)[:, 0], times)[0]
        res["host_nets"] = HOST_NETS
        res["host_per_network_scaled_ms"] = round(1e3 * (time.perf_counter() - t0) * M / HOST_NETS + res["forward_many_ms"], 1)
        res["ibs"] = float(np.sum(0.5 * (got["brier"][0, 1:] + got["brier"][0, :-1]) * np.diff(times)) / (times[-1] - times[0]))
        res["max_diff_mixture"] = float(np.max(np.abs(got["brier"][0] - bs_host)))
        res["max_diff_curves"] = float(np.max(np.abs(got["curves"][:, 0] - S_host)))
        res["max_diff_per_network"] = float(np.max(np.abs(got["per_network"][:HOST_NETS, 0] - net_host)))
        print(json.dumps(res), flush=True)
        ch.close()


if __name__ == "__main__":
    main()
