"""Times the CRPS of the predictive mixture on the device (predictor.crps: tbnn_ensemble_crps, the pair kernel k_ens_crps) against the
route it replaces: Chain.forward_many (4 m d_out n bytes to the host) followed by the fp64 NumPy restatement of the definition
(tests/crps_ref.py: crps_np, the full double sum over an [m, m, rows] intermediate).
Shapes: 256 networks of 5-50-50-50-1 over 100,000 rows (the benchmark's flagship network) and of 784-20-20-1 over 12,000 rows.  Each
device figure: one warm-up call, then the median of five calls on a host clock -- every call returns after its stream work has completed
(include/tbnn.h) -- so predictor_crps_ms holds the 256 forward passes, the pair kernel and the copies; forward_many_ms beside it is the
forward passes and their copy alone.  pred_quantiles_ms is predictor.predictiveQuantiles at three probabilities (k_ens_pred_quantiles) at
the same shape, for scale: one thread per element, some tens of passes over m.
THE HOST FIGURE IS EXTRAPOLATED: the [m, m, rows] fp64 intermediates of the NumPy route take 0.5 MB per row and temporary, so it is run
(once, after a warm-up on 8 rows) on the first HOST_ROWS rows only and host_route_extrapolated_ms = its time x rows / HOST_ROWS, plus the
measured forward_many over all rows.  The work is linear in the rows, so the extrapolation is fair; it is still not a measurement at the
full size, which the host cannot hold.
Prints one JSON line per shape with the library's build id, the pair terms per call, and the largest deviation between the two routes on
the host's rows in units of 2^-53 (error + spread), with the device's own deviation from the 40-digit restatement (crps_ref.ref40) on the
first three rows.  Needs a gfx950 device; there is no fallback."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
from tensorbnn_amd import _native as nat                     # noqa: E402
from tensorbnn_amd.likelihood import FixedGaussianLikelihood  # noqa: E402
from tensorbnn_amd.predictor import predictor                # noqa: E402
import crps_ref as cr                                        # noqa: E402

M = 256
HOST_ROWS = 128
REF40_ROWS = 3
SD = 0.3
SHAPES = {
    "flagship": ([5, 50, 50, 50, 1], 100_000),
    "tall": ([784, 20, 20, 1], 12_000),
}


def median_of(fn, runs=5):
    fn()                                                   # warm-up: code objects loaded, pooled buffers grown
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def memory_predictor(dims, thetas):
    """a predictor around networks held in memory: what loadNetworks / loadArchitecture leave behind, and the forward chain"""
    p = predictor.__new__(predictor)
    p.numNetworks, p.numChains = thetas.shape[0], 1
    p.vectors = [t for t in thetas]
    p.hypers = []
    p.likelihood = FixedGaussianLikelihood(sd=SD)
    layers = [(dims[i], dims[i + 1], nat.ACT_RELU if i < len(dims) - 2 else nat.ACT_NONE, 0) for i in range(len(dims) - 1)]
    p._chain = nat.Chain(layers, likelihood=nat.LIK_FIXED_GAUSSIAN, fixed_sd=SD)
    return p


def main():
    if nat.device_count() < 1:
        sys.exit("time_crps: no gfx950 device")
    for name, (dims, n) in SHAPES.items():
        rng = np.random.default_rng(0)
        X = (rng.standard_normal((n, dims[0])) / np.sqrt(max(dims[0] / 16.0, 1.0))).astype(np.float32)
        base = np.concatenate([(rng.standard_normal(o * i + o) * (2.0 / i) ** 0.5) for i, o in zip(dims[:-1], dims[1:])])
        thetas = (base[None, :] + 0.1 * rng.standard_normal((M, base.size))).astype(np.float32)
        p = memory_predictor(dims, thetas)
        ch = p._chain
        f = ch.forward_many(thetas, X=X)
        Y = (f[rng.integers(0, M, n), 0, np.arange(n)] + SD * rng.standard_normal(n)).astype(np.float32)[:, None]
        res = {"shape": name, "dims": dims, "networks": M, "rows": n, "kernel": ch.kernel_name, "build_id": nat.build_id(),
               "pair_terms": M * (M + 1) // 2 * n}
        res["predictor_crps_ms"] = round(1e3 * median_of(lambda: p.crps(X, Y)), 3)
        res["predictor_crps_no_noise_ms"] = round(1e3 * median_of(lambda: p.crps(X, Y, noise=False)), 3)
        res["forward_many_ms"] = round(1e3 * median_of(lambda: ch.forward_many(thetas, X=X)), 3)
        res["pred_quantiles_ms"] = round(1e3 * median_of(lambda: p.predictiveQuantiles(X, [0.05, 0.5, 0.95])), 3)
        sd = np.full(M, np.float32(SD))
        host = lambda rows: cr.crps_np(f[:, 0, :rows].astype(np.float64), cr.clip_sd(sd), None, Y[:rows, 0].astype(np.float64))
        host(8)
        t0 = time.perf_counter()
        ref = host(HOST_ROWS)
        t_host = time.perf_counter() - t0
        res["host_rows"] = HOST_ROWS
        res["host_numpy_ms_on_host_rows"] = round(1e3 * t_host, 1)
        res["host_route_extrapolated_ms"] = round(1e3 * t_host * n / HOST_ROWS + res["forward_many_ms"], 1)
        got = p.crps(X, Y)
        unit = cr.U * (ref[1] + ref[2])
        res["largest_deviation_u"] = {k: float(np.max(np.abs(got[k][0, :HOST_ROWS] - ref[i]) / unit)) for i, k in enumerate(("crps", "error", "spread"))}
        # (the NumPy sum over [m, m] runs along the outer axes, where NumPy adds one by one: most of that deviation is the host's own --
        # the device against the 40-digit restatement on the first REF40_ROWS rows, a second and a half of mpmath per row at m = 256)
        r40 = cr.ref40(f[:, 0, :REF40_ROWS].astype(np.float64), cr.clip_sd(sd), None, Y[:REF40_ROWS, 0].astype(np.float64))
        dev = cr.deviation_u([got[k][0, :REF40_ROWS] for k in ("crps", "error", "spread")], r40)
        res["deviation_from_40_digits_u"] = {k: float(dev[i].max()) for i, k in enumerate(("crps", "error", "spread"))}
        res["mean_crps"], res["se"] = float(got["mean_crps"][0]), float(got["se"][0])
        print(json.dumps(res), flush=True)
        ch.close()


if __name__ == "__main__":
    main()
