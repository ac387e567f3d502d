"""Times pre-training on the device (Chain.optimize: tbnn_optimize) against the route it replaces and against its floor:
  (a) Chain.optimize, STEPS Adam / AMSGrad steps per call, checked every 1, 10 and 100 steps (a check is one more single-workgroup kernel,
      k_optim_logp, between the fused pass and the update);
  (b) the host route: a Python loop of Chain.logp_grad (the same fused pass, the gradient copied to the host) and a NumPy Adam step in
      fp32, HOST_STEPS steps per call;
  (c) Chain.hmc_run's leapfrog steps per second at the same shape and build (EPOCHS transitions of LEAPFROG steps; the per-step path: the
      trajectory kernel is for small problems): one step of either is one fused pass plus one update-shaped kernel, so this is the floor.
Shapes: configs[1]'s 5-50-50-50-1 over 100,000 rows, and the tutorial's 784-20-20-1 over 12,000 rows.  Each figure: one warm-up call, then
the median of five calls on a host clock -- every call returns after its stream work has completed (include/tbnn.h).  Every call starts
from the same state; the step sizes are small enough that the weights stay where they are.  Prints one JSON line per shape with the
library's build id.  Needs a gfx950 device; there is no fallback."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from tensorbnn_amd import _native as nat                     # noqa: E402

STEPS, HOST_STEPS, LEAPFROG, EPOCHS = 2000, 200, 200, 10
LR = 1e-5

SHAPES = {
    "headline": ([5, 50, 50, 50, 1], nat.ACT_RELU, nat.ACT_NONE, nat.LIK_GAUSSIAN, 100_000),
    "tutorial": ([784, 20, 20, 1], nat.ACT_RELU, nat.ACT_SIGMOID, nat.LIK_BERNOULLI, 12_000),
}


def median_of(fn, runs=5):
    fn()                                                   # warm-up: code objects loaded, pooled buffers grown
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def host_adam(ch, theta0, steps, lr=LR, b1=0.9, b2=0.999, eps=1e-8):
    f = np.float32
    theta = theta0.copy()
    m, v, vhat = np.zeros_like(theta), np.zeros_like(theta), np.zeros_like(theta)
    for t in range(1, steps + 1):
        _lp, g, _st = ch.logp_grad(theta)
        m = f(b1) * m + f(1 - b1) * g
        v = f(b2) * v + f(1 - b2) * (g * g)
        vhat = np.maximum(vhat, v)
        theta = theta + f(lr / (1 - b1 ** t)) * m / (np.sqrt(vhat) * f(1 / np.sqrt(1 - b2 ** t)) + f(eps))
    return theta


def main():
    if nat.device_count() < 1:
        sys.exit("time_optimize: no gfx950 device")
    for name, (dims, act, last, lik, n) in SHAPES.items():
        layers = [(dims[i], dims[i + 1], act if i < len(dims) - 2 else last, 0) for i in range(len(dims) - 1)]
        ch = nat.Chain(layers, likelihood=lik)
        rng = np.random.default_rng(0)
        X = (rng.standard_normal((n, dims[0])) / np.sqrt(max(dims[0] / 16.0, 1.0))).astype(np.float32)
        theta0 = np.concatenate([(rng.standard_normal(o * i + o) * (2.0 / o) ** 0.5) for i, o in zip(dims[:-1], dims[1:])]).astype(np.float32)
        if lik == nat.LIK_BERNOULLI:
            Y = (rng.random((n, dims[-1])) < 0.5).astype(np.float32)
        else:
            Y = rng.standard_normal((n, dims[-1])).astype(np.float32)
        ch.set_data(X, Y)
        res = {"shape": name, "dims": dims, "rows": n, "kernel": ch.kernel_name, "build_id": nat.build_id(), "steps_per_call": STEPS}

        for every in (1, 10, 100):
            def run(every=every):
                ch.set_state(theta0)
                return ch.optimize(STEPS, lr=LR, check_every=every, keep="last")
            res[f"optimize_steps_per_s_check_every_{every}"] = round(STEPS / median_of(run), 1)
        out = run(100)
        res["optimize_device_steps_per_s_check_every_100"] = round(STEPS / (out["device_us"] * 1e-6), 1)
        res["objective_first_last"] = [out["obj_first"], out["obj_last"]]

        res["host_loop_steps_per_s"] = round(HOST_STEPS / median_of(lambda: host_adam(ch, theta0, HOST_STEPS)), 1)
        res["host_steps_per_call"] = HOST_STEPS

        def sample():
            ch.set_state(theta0)
            return ch.hmc_run(1e-7, LEAPFROG, EPOCHS)
        res["hmc_run_leapfrog_steps_per_s"] = round(LEAPFROG * EPOCHS / median_of(sample), 1)
        res["hmc_run_path"] = ch.last_transition_path
        res["optimize_over_leapfrog_check_every_100"] = round(res["optimize_steps_per_s_check_every_100"] / res["hmc_run_leapfrog_steps_per_s"], 4)
        res["optimize_over_host_loop_check_every_10"] = round(res["optimize_steps_per_s_check_every_10"] / res["host_loop_steps_per_s"], 2)
        print(json.dumps(res), flush=True)
        ch.close()


if __name__ == "__main__":
    main()
