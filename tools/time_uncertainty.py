"""Times the classification-uncertainty reduction on the device (predictor.predictUncertainty: tbnn_ensemble_uncertainty) against the
route it replaces: Chain.forward_many (4 m d_out n bytes to the host) followed by the NumPy restatement of the definition
(tests/uncertainty_ref.py: fp64 softmax or clip, entropies, votes, np.longdouble sums).
Shapes: 256 networks of 784-100-100-10 read as a categorical over 12,000 rows (the reference's MNIST tutorial shape), and 256 networks of
20-100-100-2 with sigmoid outputs read as Bernoulli over 100,000 rows (configs[4] of the benchmark).  Each figure: one warm-up call, then
the median of five calls on a host clock -- every call returns after its stream work has completed (include/tbnn.h).  The networks are
random draws around one base vector; the predictor is built in memory around them (no files).  Prints one JSON line per shape with the
library's build id and the largest difference between the two routes.  Needs a gfx950 device; there is no fallback."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from tensorbnn_amd import _native as nat                     # noqa: E402
from tensorbnn_amd.likelihood import BernoulliLikelihood, CategoricalLikelihood     # noqa: E402
from tensorbnn_amd.predictor import predictor                # noqa: E402
import uncertainty_ref as ur                                 # noqa: E402

M = 256
SHAPES = {
    "mnist": ([784, 100, 100, 10], nat.ACT_RELU, nat.ACT_NONE, "categorical", 12_000),
    "configs4": ([20, 100, 100, 2], nat.ACT_RELU, nat.ACT_SIGMOID, "bernoulli", 100_000),
}


def median_of(fn, runs=5):
    fn()                                                   # warm-up: code objects loaded, pooled buffers grown
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def memory_predictor(dims, act, last, likelihood, thetas):
    """a predictor around networks held in memory: what loadNetworks / loadArchitecture leave behind, and the forward chain"""
    p = predictor.__new__(predictor)
    p.numNetworks, p.numChains = thetas.shape[0], 1
    p.vectors = [t for t in thetas]
    p.hypers = []
    p.likelihood = likelihood
    layers = [(dims[i], dims[i + 1], act if i < len(dims) - 2 else last, 0) for i in range(len(dims) - 1)]
    p._chain = nat.Chain(layers, likelihood=nat.LIK_FIXED_GAUSSIAN, fixed_sd=1.0)
    return p


def main():
    if nat.device_count() < 1:
        sys.exit("time_uncertainty: no gfx950 device")
    for name, (dims, act, last, kind, n) in SHAPES.items():
        rng = np.random.default_rng(0)
        X = (rng.standard_normal((n, dims[0])) / np.sqrt(max(dims[0] / 16.0, 1.0))).astype(np.float32)
        base = np.concatenate([(rng.standard_normal(o * i + o) * (2.0 / i) ** 0.5) for i, o in zip(dims[:-1], dims[1:])])
        thetas = (base[None, :] + 0.1 * rng.standard_normal((M, base.size))).astype(np.float32)
        lik = CategoricalLikelihood() if kind == "categorical" else BernoulliLikelihood()
        p = memory_predictor(dims, act, last, lik, thetas)
        ch = p._chain
        res = {"shape": name, "dims": dims, "networks": M, "rows": n, "reading": kind, "kernel": ch.kernel_name, "build_id": nat.build_id()}
        res["predictUncertainty_ms"] = round(1e3 * median_of(lambda: p.predictUncertainty(X)), 3)
        res["forward_many_ms"] = round(1e3 * median_of(lambda: ch.forward_many(thetas, X=X)), 3)
        res["host_route_ms"] = round(1e3 * median_of(lambda: ur.uncertainty(ch.forward_many(thetas, X=X), None, kind)), 1)
        got, ref = p.predictUncertainty(X), ur.uncertainty(ch.forward_many(thetas, X=X), None, kind)
        res["largest_difference"] = {k: float(np.max(np.abs(got[k] - ref[k]))) for k in ("probs", "votes", "total", "aleatoric", "epistemic")}
        res["epistemic_median"] = float(np.median(ref["epistemic"]))
        print(json.dumps(res), flush=True)
        ch.close()


if __name__ == "__main__":
    main()
