"""One rank of the world-2 Weibull test of the row-sharded chain (tests/test_gpu_weibull.py): run as a child process with TBNN_RCCL_LIB
pointing at the stub collective library.  argv: rank world idfile outfile.  (World size and shapes are tests/stubccl/worker_poisson.py's;
the problems are tests/weibull_ref.py's: signed targets drawn from the model, events and right-censored rows on every rank.)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import tbnn_oracle as o                      # noqa: E402  (problem generator: this is a test)
import weibull_ref as wr                    # noqa: E402
from tensorbnn_amd import _native as nat    # noqa: E402
from tensorbnn_amd import parallel          # noqa: E402
from worker import exchange_id              # noqa: E402

SHAPES = {
    # dims, rows, hidden activation, prior, jit, shape
    "narrow": ([5, 50, 50, 50, 1], 3001, o.ACT_RELU, o.PRIOR_CAUCHY, True, 0.5),       # the run-time fast3 table of tests/test_gpu_weibull.py
    "layered": ([40, 24, 24, 3], 900, o.ACT_TANH, o.PRIOR_CAUCHY, False, 1.5),
    "generic": ([4, 9, 2], 700, o.ACT_ELU, o.PRIOR_GAUSSIAN, None, 1.0),
}


def problem(name):
    dims, n, act, prior, _jit, k = SHAPES[name]
    return wr.problem_of(dims, n, act, prior, k)


def chain_of(name, spec):
    jit = SHAPES[name][4]
    layers = [(l.in_dim, l.out_dim, l.act, l.prior) for l in spec.layers]
    kw = dict(likelihood=nat.LIK_WEIBULL, lik_df=SHAPES[name][5])
    if jit is None:
        return nat.Chain(layers, kernel=nat.KERNEL_GENERIC, **kw)
    return nat.Chain(layers, kernel=nat.KERNEL_AUTO, jit=jit, **kw)


def main():
    rank, world, idfile, outfile = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    res = {}
    for name in SHAPES:
        spec, X, Y, theta, eta = problem(name)
        ch = chain_of(name, spec)
        comm = nat.Comm(ch, world, rank, exchange_id(rank, idfile + "." + name))
        lo, hi = parallel.shard_rows(ch, X, Y, comm)
        ch.set_state(theta); ch.set_hypers(eta)
        lp, g, st = ch.logp_grad(theta, eta)
        p0 = np.random.default_rng(5).standard_normal(spec.n_params).astype(np.float32)
        outs = [ch.hmc_step(1e-5, 4, p0=p0, log_u=-1e30, trace=True), ch.hmc_step(1e-5, 3)]      # injected, then free-running
        res[name + "_rows"] = np.array([lo, hi]); res[name + "_kernel"] = np.array(ch.kernel_name)
        res[name + "_lp"] = np.array(lp); res[name + "_g"] = g; res[name + "_st"] = np.array(st)
        res[name + "_trace"] = np.asarray(outs[0]["trace_logp"])
        res[name + "_lar"] = np.array([x["log_accept_ratio"] for x in outs]); res[name + "_acc"] = np.array([x["accepted"] for x in outs])
        res[name + "_theta"] = ch.get_state()
        comm.close(); ch.close()
    np.savez(outfile, **res)


if __name__ == "__main__":
    main()
