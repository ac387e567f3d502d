"""Times the input sensitivities of an ensemble on the device (Chain.ensemble_input_grad: tbnn_ensemble_input_grad, the MFMA kernel
k_ens_input_grad) beside Chain.forward_many at the same shape, and beside the route it replaces: forward_many at 2 d_in shifted inputs
followed by NumPy's central differences and moments.
Shapes: 256 networks of 5-50-50-50-1 over 10,000 and 100,000 rows, and of 784-20-20-1 over 12,000 rows.  Each device figure: one warm-up
call, then the median of five whole calls on a host clock -- every call returns after its stream work has completed (include/tbnn.h) -- so
input_grad_ms holds the uploads, the kernel, the finish kernel and the copies of the three planes.
THE HOST FIGURE IS EXTRAPOLATED where d_in > HOST_INPUTS: the 2 d_in forward_many calls and the NumPy differences are run for the first
HOST_INPUTS inputs only and scaled by d_in / HOST_INPUTS (the work is linear in the inputs); `host_route_extrapolated` says which.
flop = 2 P (1 + d_out) per network and row (forward and reverse pass); mfma_peak_fraction = flop / time / FP32_MFMA_PEAK, of the WHOLE
call, not of the kernel.  Prints one JSON line per shape.  Needs a gfx950 device; there is no fallback."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from tensorbnn_amd import _native as nat                     # noqa: E402

M = 256
HOST_INPUTS = 5
FP32_MFMA_PEAK = 157.3e12                  # MI355X, FP32 matrix, flop/s
SHAPES = [([5, 50, 50, 50, 1], 10_000), ([5, 50, 50, 50, 1], 100_000), ([784, 20, 20, 1], 12_000)]


def median_of(fn, runs=5):
    fn()                                                   # warm-up: code objects loaded
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    if nat.device_count() < 1:
        sys.exit("time_input_grad: no gfx950 device")
    for dims, n in SHAPES:
        rng = np.random.default_rng(0)
        X = (rng.standard_normal((n, dims[0])) / np.sqrt(max(dims[0] / 16.0, 1.0))).astype(np.float32)
        base = np.concatenate([(rng.standard_normal(o * i + o) * (2.0 / i) ** 0.5) for i, o in zip(dims[:-1], dims[1:])])
        thetas = (base[None, :] + 0.1 * rng.standard_normal((M, base.size))).astype(np.float32)
        layers = [(dims[i], dims[i + 1], nat.ACT_RELU if i < len(dims) - 2 else nat.ACT_NONE, 0) for i in range(len(dims) - 1)]
        ch = nat.Chain(layers, likelihood=nat.LIK_FIXED_GAUSSIAN, fixed_sd=0.3)
        flop = 2.0 * base.size * (1 + dims[-1]) * M * n
        res = {"dims": dims, "networks": M, "rows": n, "kernel": ch.kernel_name, "build_id": nat.build_id(), "flop": flop}
        t = median_of(lambda: ch.ensemble_input_grad(thetas, X=X))
        res["input_grad_ms"] = round(1e3 * t, 3)
        res["mfma_peak_fraction_of_whole_call"] = round(flop / t / FP32_MFMA_PEAK, 5)
        res["forward_many_ms"] = round(1e3 * median_of(lambda: ch.forward_many(thetas, X=X)), 3)
        k_host = min(dims[0], HOST_INPUTS)
        h = np.float32(1e-2)

        def host_route():
            out = np.empty((dims[-1], k_host, n))
            for k in range(k_host):
                e = np.zeros(dims[0], dtype=np.float32)
                e[k] = h
                d = (ch.forward_many(thetas, X=X + e).astype(np.float64) - ch.forward_many(thetas, X=X - e)) / (2.0 * float(h))
                out[:, k] = d.mean(axis=0)
                d.var(axis=0), np.abs(d).mean(axis=0)
            return out

        t_host = median_of(host_route, runs=1)
        res["host_inputs"] = k_host
        res["host_route_ms"] = round(1e3 * t_host * dims[0] / k_host, 1)
        res["host_route_extrapolated"] = dims[0] > k_host
        print(json.dumps(res), flush=True)
        ch.close()


if __name__ == "__main__":
    main()
