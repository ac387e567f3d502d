"""Times PSIS-LOO / WAIC of an ensemble (tbnn_ensemble_loo) against the host route it replaces:
  (a) Chain.ensemble_loo, all four row outputs (forward passes, the matrix, the smoothing; 32 n bytes cross to the host);
  (b) Chain.ensemble_loo asked for lppd and p_waic only through the C ABI (no smoothing kernel): (a) - (b) is what k_ens_psis costs;
  (c) Chain.ensemble_loglik (forward passes and the two sums the matrix was thrown away after): the floor;
  (d) Chain.forward_many (4 m d_out n bytes cross), the Gaussian terms in fp64 NumPy, then tests/psis_ref.py.  The host part runs over the
      first HOST_ROWS rows, once, and its time is scaled to all n rows (it is linear in them); forward_many is timed over all rows.
Shapes: 5-50-50-50-1 with m = 256 networks over n = 100,000 rows and 784-20-20-1 with m = 256 over n = 12,000 (judged as a fixed Gaussian
both: the cost does not depend on the likelihood's kind beyond the matrix).  The thetas are small walks around one base.
Device routes: one warm-up call, then RUNS calls, each between a pair of hipEvents recorded on the null stream.  The library works on a
stream of its own and every entry point returns after that stream has drained, so a pair brackets the whole call -- uploads, forward passes,
kernels, copies of the results -- as a host clock around it does (a call time, not a kernel time); the median and the spread (min .. max)
are printed, and the host clock's median beside them.  The host route (d) is timed once.  One JSON line per shape with
the library's build id.  Needs a gfx950 device; there is no fallback."""
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from tensorbnn_amd import _native as nat                     # noqa: E402
from psis_ref import psis_ref                                # noqa: E402

RUNS = 7
HOST_ROWS = 10_000
SD = 0.7
SHAPES = {
    "headline": ([5, 50, 50, 50, 1], nat.ACT_RELU, nat.ACT_NONE, 256, 100_000),
    "tutorial": ([784, 20, 20, 1], nat.ACT_RELU, nat.ACT_SIGMOID, 256, 12_000),
}

hip = C.CDLL("libamdhip64.so")
for fn, args in (("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]), ("hipEventSynchronize", [C.c_void_p]),
                 ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]), ("hipEventDestroy", [C.c_void_p])):
    getattr(hip, fn).argtypes, getattr(hip, fn).restype = args, C.c_int


def hipchk(rc):
    if rc:
        raise RuntimeError(f"HIP error {rc}")


def timed(fn):
    """(median ms, min ms, max ms) between event pairs, median ms on the host clock, the last result"""
    e0, e1 = C.c_void_p(), C.c_void_p()
    hipchk(hip.hipEventCreate(C.byref(e0))); hipchk(hip.hipEventCreate(C.byref(e1)))
    fn()                                                   # warm-up: code objects loaded, pooled buffers grown
    dev, host = [], []
    for _ in range(RUNS):
        hipchk(hip.hipEventRecord(e0, None))
        t0 = time.perf_counter()
        out = fn()
        host.append((time.perf_counter() - t0) * 1e3)
        hipchk(hip.hipEventRecord(e1, None)); hipchk(hip.hipEventSynchronize(e1))
        ms = C.c_float()
        hipchk(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        dev.append(ms.value)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return {"ms": round(statistics.median(dev), 3), "min": round(min(dev), 3), "max": round(max(dev), 3),
            "host_clock_ms": round(statistics.median(host), 3)}, out


def walk(rng, P, m):
    base = rng.standard_normal(P) * 0.3
    dev, out = rng.standard_normal(P), np.empty((m, P), dtype=np.float32)
    for s in range(m):
        dev = 0.6 * dev + 0.8 * rng.standard_normal(P)
        out[s] = base + 0.03 * dev
    return out


def gaussian_terms(f, Y, sd):
    d = (Y.T.astype(np.float64)[None] - f.astype(np.float64)) / sd
    return (-0.5 * d * d - math.log(sd) - 0.5 * math.log(2 * math.pi)).sum(axis=1)


def main():
    if nat.device_count() < 1:
        sys.exit("loo_time: no gfx950 device")
    dp = C.POINTER(C.c_double)
    for name, (dims, act, last, m, n) in SHAPES.items():
        layers = [(dims[i], dims[i + 1], act if i < len(dims) - 2 else last, 0) for i in range(len(dims) - 1)]
        ch = nat.Chain(layers, likelihood=nat.LIK_FIXED_GAUSSIAN, fixed_sd=SD)
        rng = np.random.default_rng(0)
        X = (rng.standard_normal((n, dims[0])) / np.sqrt(max(dims[0] / 16.0, 1.0))).astype(np.float32)
        thetas = walk(rng, ch.P, m)
        Y = (ch.forward_many(thetas[:1], X=X)[0].T + SD * rng.standard_normal((n, dims[-1]))).astype(np.float32)
        lppd, pw = np.empty(n), np.empty(n)

        def waic_only():
            rc = nat.lib.tbnn_ensemble_loo(ch._h, nat._p(thetas), m, thetas.shape[1], nat.LIK_FIXED_GAUSSIAN, None, 1, nat._p(X), nat._p(Y), n, 1.0,
                                           None, None, lppd.ctypes.data_as(dp), pw.ctypes.data_as(dp), None)
            assert rc == 0, nat.lib.tbnn_last_error()

        ta, res = timed(lambda: ch.ensemble_loo(thetas, Y=Y, X=X))
        tb, _ = timed(waic_only)
        tc, _ = timed(lambda: ch.ensemble_loglik(thetas, Y=Y, X=X))
        tf, _ = timed(lambda: ch.forward_many(thetas, X=X))
        hr = min(HOST_ROWS, n)
        f = ch.forward_many(thetas, X=X[:hr])
        t0 = time.perf_counter()
        ref = psis_ref(gaussian_terms(f, Y[:hr], SD))
        t_host = (time.perf_counter() - t0) * 1e3 * n / hr
        k = res["pareto_k"]
        fin = np.isfinite(ref["pareto_k"])
        print(json.dumps({"shape": name, "dims": dims, "kernel": ch.kernel_name, "m": m, "n": n, "build_id": nat.build_id(), "runs": RUNS,
                          "ensemble_loo": ta, "ensemble_loo_waic_only": tb, "ensemble_loglik": tc, "forward_many": tf,
                          "psis_kernel_ms": round(ta["ms"] - tb["ms"], 3), "host_rows": hr, "host_terms_psis_ref_ms_scaled_to_n": round(t_host, 1),
                          "forward_many_psis_ref_ms": round(tf["ms"] + t_host, 1), "ratio": round((tf["ms"] + t_host) / ta["ms"], 1),
                          "bytes_to_host": {"forward_many": 4 * m * dims[-1] * n, "ensemble_loo": 32 * n},
                          "pareto_k": [float(np.min(k)), float(np.median(k)), float(np.max(k))],
                          "max_abs_diff_k": float(np.abs(k[:hr] - ref["pareto_k"])[fin].max()),
                          "max_rel_diff_elpd_loo": float(np.max(np.abs(res["elpd_loo"][:hr] - ref["elpd_loo"]) / np.abs(ref["elpd_loo"])))}),
              flush=True)
        ch.close()


if __name__ == "__main__":
    main()
