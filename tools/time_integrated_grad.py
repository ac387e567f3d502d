"""Times the integrated-gradients attributions of an ensemble on the device (Chain.ensemble_integrated_grad: tbnn_ensemble_integrated_grad,
the MFMA kernel k_ens_path_grad) beside the two routes it replaces, measured in the same session:
  (a) composition: Chain.ensemble_input_grad(per_network=True) at the P n path rows, then the NumPy quadrature, product with x - x0 and
      moments over the networks -- in blocks of BLOCK_ROWS data rows, since the per-network Jacobians of all P n rows do not fit the host.
      THE FIGURE IS EXTRAPOLATED: HOST_BLOCKS blocks are run and scaled by n / (HOST_BLOCKS BLOCK_ROWS) (the work is linear in the rows);
  (b) P times the plain Chain.ensemble_input_grad call over the n rows: the device work of P Jacobians without the host quadrature.
Shapes: 256 networks of 5-50-50-50-1 over 10,000 rows and of 784-20-20-1 over 12,000 rows, each at P = 16 and 64.  Each device figure:
one warm-up call, then the median of five whole calls on a host clock -- every call returns after its stream work has completed
(include/tbnn.h) -- so integrated_grad_ms holds the uploads, the kernel, the finish kernel and the copies of the planes and of diff.
flop = 2 P_net (1 + d_out) P per network and row less 2 d_in out_1 d_out (P - 1), the last product taken once; mfma_peak_fraction =
flop / time / FP32_MFMA_PEAK, of the WHOLE call, not of the kernel.  Prints one JSON line per shape and P.  Needs a gfx950 device; there
is no fallback."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from tensorbnn_amd import _native as nat                     # noqa: E402
from time_input_grad import FP32_MFMA_PEAK, M, median_of     # noqa: E402

BLOCK_ROWS = 8                             # 256 networks x 784 inputs x 8 x 64 path rows: 0.4 GB of Jacobians, 0.8 GB widened
HOST_BLOCKS = 2
SHAPES = [([5, 50, 50, 50, 1], 10_000), ([784, 20, 20, 1], 12_000)]


def main():
    if nat.device_count() < 1:
        sys.exit("time_integrated_grad: no gfx950 device")
    for dims, n in SHAPES:
        rng = np.random.default_rng(0)
        X = (rng.standard_normal((n, dims[0])) / np.sqrt(max(dims[0] / 16.0, 1.0))).astype(np.float32)
        x0 = np.zeros(dims[0], dtype=np.float32)
        base = np.concatenate([(rng.standard_normal(o * i + o) * (2.0 / i) ** 0.5) for i, o in zip(dims[:-1], dims[1:])])
        thetas = (base[None, :] + 0.1 * rng.standard_normal((M, base.size))).astype(np.float32)
        layers = [(dims[i], dims[i + 1], nat.ACT_TANH if i < len(dims) - 2 else nat.ACT_NONE, 0) for i in range(len(dims) - 1)]
        ch = nat.Chain(layers, likelihood=nat.LIK_FIXED_GAUSSIAN, fixed_sd=0.3)
        t_jac = median_of(lambda: ch.ensemble_input_grad(thetas, X=X))
        for P in (16, 64):
            flop = (2.0 * base.size * (1 + dims[-1]) * P - 2.0 * dims[0] * dims[1] * dims[-1] * (P - 1)) * M * n
            res = {"dims": dims, "networks": M, "rows": n, "points": P, "kernel": ch.kernel_name, "build_id": nat.build_id(), "flop": flop}
            try:
                t = median_of(lambda: ch.ensemble_integrated_grad(thetas, X, baseline=x0, points=P))
            except nat.TbnnError as e:                     # 784-20-20-1 fits the 16-row tile only: more than 16 points are refused
                print(json.dumps(dict(res, refused=str(e))), flush=True)
                continue
            res["integrated_grad_ms"] = round(1e3 * t, 3)
            res["mfma_peak_fraction_of_whole_call"] = round(flop / t / FP32_MFMA_PEAK, 5)
            a = (np.arange(P, dtype=np.float32) / np.float32(P - 1))[None, :, None]
            q = np.full(P, 1.0 / (P - 1))
            q[[0, P - 1]] *= 0.5

            def composition():
                for b in range(HOST_BLOCKS):
                    x = X[b * BLOCK_ROWS:(b + 1) * BLOCK_ROWS]
                    xs = (x0 + a * (x - x0)[:, None, :]).reshape(-1, dims[0])
                    jac = ch.ensemble_input_grad(thetas, X=xs, per_network=True)["per_network"]
                    att = (jac.reshape(jac.shape[:3] + (len(x), P)) * q).sum(axis=-1) * (x - x0).T.astype(np.float64)
                    att.mean(axis=0), att.var(axis=0), np.abs(att).mean(axis=0)

            res["composition_ms"] = round(1e3 * median_of(composition, runs=1) * n / (HOST_BLOCKS * BLOCK_ROWS), 1)
            res["composition_extrapolated_from_rows"] = HOST_BLOCKS * BLOCK_ROWS
            res["input_grad_ms"] = round(1e3 * t_jac, 3)
            res["points_times_input_grad_ms"] = round(1e3 * t_jac * P, 1)
            print(json.dumps(res), flush=True)
        ch.close()


if __name__ == "__main__":
    main()
