"""Times Harrell's concordance index of a survival ensemble on the device (Chain.ensemble_concordance: tbnn_ensemble_concordance, the pair
kernel k_ens_concordance) against the routes it replaces: Chain.forward_many (4 m d_out n bytes to the host) followed by (a) the quadratic
NumPy restatement of the definition (tests/concordance_ref.py) and (b) a sort-based host C per network: argsort by score, then a
Fenwick-tree count of the scores below and equal over the rows in time order -- O(n log n), the form this library does not build.
Shapes: 256 networks of 5-50-50-50-1 over 10,000 and 100,000 rows and of 784-20-20-1 over 12,000 rows; exponential times, 40 % censored.
Each device figure: one warm-up call, then the median of five calls on a host clock -- every call returns after its stream work has
completed (include/tbnn.h) -- so concordance_ms holds the 256 forward passes, the host staging, the gather and pair kernels and the copies;
forward_many_ms beside it is the forward passes and their copy alone, staging_ms the host's sort / suffix / work-list step alone
(restated here in NumPy from the same rule, so a little slower than the library's C++).
THE QUADRATIC HOST FIGURE IS EXTRAPOLATED: the boolean [n, n] matrices are run on the first HOST_ROWS rows of HOST_NETS networks and the
time scaled by (n / HOST_ROWS)^2 m / HOST_NETS, plus the measured forward_many: not a measurement at the full size.  The Fenwick route is
measured at the full row count on HOST_NETS networks and scaled by m / HOST_NETS (linear in the networks).
Prints one JSON line per shape with the library's build id, the pairs per call, and whether the device's counts equal both host routes'
on what those ran.  --ipcw: instead of all that, Uno's IPCW C beside Harrell's at the flagship shapes (ipcw_leg).
Needs a gfx950 device; there is no fallback."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from tensorbnn_amd import _native as nat                     # noqa: E402
import concordance_ref as cr                                 # noqa: E402

M = 256
HOST_ROWS = 2000
HOST_NETS = 2
SHAPES = [("flagship 1e4", [5, 50, 50, 50, 1], 10_000), ("flagship 1e5", [5, 50, 50, 50, 1], 100_000), ("tall", [784, 20, 20, 1], 12_000)]


def median_of(fn, runs=5):
    fn()                                                   # warm-up: code objects loaded, pooled buffers grown
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def staging(y):
    """the library's host step for one column, in NumPy: the sort, the suffix starts and the comparable count"""
    t, e = np.abs(y), y > 0
    perm = np.lexsort((~e, t))
    ts, es = t[perm], e[perm]
    n = y.size
    run_end = np.r_[np.flatnonzero((ts[1:] != ts[:-1]) | (es[1:] != es[:-1])) + 1, n]      # the end of every run of equal (time, flag)
    jstart = np.where(es, np.repeat(run_end, np.diff(np.r_[0, run_end])), n)
    return perm, jstart, int((n - jstart).sum())


def fenwick_counts(y, s):
    """(comparable, concordant, tied) by ranks and a Fenwick tree: rows enter the tree from the latest time down, each event asks how many
    scores above / equal to its own are in it (its own run of equal-time events enters after it asked)"""
    perm, jstart, comparable = staging(y)
    n = y.size
    vals, rank = np.unique(s[perm], return_inverse=True)
    tree, eq = [0] * (vals.size + 1), [0] * vals.size
    conc = tied = 0
    inside, j = 0, n
    for i in range(n - 1, -1, -1):
        if jstart[i] >= n:
            continue
        while j > jstart[i]:
            j -= 1
            k = int(rank[j]) + 1
            eq[k - 1] += 1
            inside += 1
            while k <= vals.size:
                tree[k] += 1
                k += k & -k
        k, below_eq = int(rank[i]) + 1, 0
        while k > 0:
            below_eq += tree[k]
            k -= k & -k
        conc += inside - below_eq
        tied += eq[int(rank[i])]
    return comparable, conc, tied


def ipcw_leg():
    """--ipcw: Uno's IPCW C (Chain.ensemble_concordance_ipcw: tbnn_ensemble_concordance_ipcw, the pair kernel k_ens_conc_ipcw) beside
    Harrell's at the flagship shapes, T = 1 (the 90 % quantile of the times) and T = 32 (10 % .. 90 %): whole calls, the two entry
    points alternating inside every repetition, one warm-up round, then the median of five.  One JSON line per (rows, T)."""
    name, dims = "flagship", SHAPES[0][1]
    for n in (10_000, 100_000):
        rng = np.random.default_rng(0)
        X = rng.standard_normal((n, dims[0])).astype(np.float32)
        base = np.concatenate([(rng.standard_normal(o * i + o) * (2.0 / i) ** 0.5) for i, o in zip(dims[:-1], dims[1:])])
        thetas = (base[None, :] + 0.1 * rng.standard_normal((M, base.size))).astype(np.float32)
        layers = [(dims[i], dims[i + 1], nat.ACT_RELU if i < len(dims) - 2 else nat.ACT_NONE, 0) for i in range(len(dims) - 1)]
        ch = nat.Chain(layers, likelihood=nat.LIK_FIXED_GAUSSIAN, fixed_sd=0.3)
        t_ev = np.exp(ch.forward_many(thetas[:1], X=X)[0, 0].astype(np.float64)) * rng.exponential(1.0, n)
        t_ce = rng.exponential(np.quantile(t_ev, 0.75), n)
        Y = np.where(t_ev <= t_ce, t_ev, -t_ce).astype(np.float32)[:, None]
        q = lambda p: np.quantile(np.abs(Y).astype(np.float64), p)
        for times in (np.array([q(0.9)]), np.linspace(q(0.1), q(0.9), 32)):
            legs = {"harrell": lambda: ch.ensemble_concordance(thetas, Y=Y, X=X), "ipcw": lambda: ch.ensemble_concordance_ipcw(thetas, times, Y=Y, X=X)}
            took = {k: [] for k in legs}
            for rep in range(6):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    got = fn()
                    if rep:                                # (repetition 0 is the warm-up)
                        took[k].append(time.perf_counter() - t0)
            ms = {k: 1e3 * statistics.median(v) for k, v in took.items()}
            print(json.dumps({"shape": f"{name} {n}", "dims": dims, "networks": M, "rows": n, "T": int(times.size), "kernel": ch.kernel_name,
                              "build_id": nat.build_id(), "censored_share": float(np.mean(Y < 0)), "harrell_ms": round(ms["harrell"], 3),
                              "ipcw_ms": round(ms["ipcw"], 3), "ipcw_over_harrell": round(ms["ipcw"] / ms["harrell"], 3),
                              "spread_ms": {k: [round(1e3 * min(v), 3), round(1e3 * max(v), 3)] for k, v in took.items()},
                              "c_index_last": float(got["c_index"][0, -1])}), flush=True)
        ch.close()


def main():
    if nat.device_count() < 1:
        sys.exit("time_concordance: no gfx950 device")
    if "--ipcw" in sys.argv[1:]:
        return ipcw_leg()
    for name, dims, n in SHAPES:
        rng = np.random.default_rng(0)
        X = (rng.standard_normal((n, dims[0])) / np.sqrt(max(dims[0] / 16.0, 1.0))).astype(np.float32)
        base = np.concatenate([(rng.standard_normal(o * i + o) * (2.0 / i) ** 0.5) for i, o in zip(dims[:-1], dims[1:])])
        thetas = (base[None, :] + 0.1 * rng.standard_normal((M, base.size))).astype(np.float32)
        layers = [(dims[i], dims[i + 1], nat.ACT_RELU if i < len(dims) - 2 else nat.ACT_NONE, 0) for i in range(len(dims) - 1)]
        ch = nat.Chain(layers, likelihood=nat.LIK_FIXED_GAUSSIAN, fixed_sd=0.3)          # (the entry point reads the raw outputs of any handle)
        f = ch.forward_many(thetas, X=X)
        t_ev = np.exp(f[0, 0].astype(np.float64)) * rng.exponential(1.0, n)
        t_ce = rng.exponential(np.quantile(t_ev, 0.75), n)
        Y = np.where(t_ev <= t_ce, t_ev, -t_ce).astype(np.float32)[:, None]
        res = {"shape": name, "dims": dims, "networks": M, "rows": n, "kernel": ch.kernel_name, "build_id": nat.build_id(),
               "censored_share": float(np.mean(Y < 0))}
        got = ch.ensemble_concordance(thetas, Y=Y, X=X)
        res["pairs_per_call"] = int(got["comparable"][0]) * (M + 1)
        res["concordance_ms"] = round(1e3 * median_of(lambda: ch.ensemble_concordance(thetas, Y=Y, X=X)), 3)
        res["forward_many_ms"] = round(1e3 * median_of(lambda: ch.forward_many(thetas, X=X)), 3)
        res["staging_ms"] = round(1e3 * median_of(lambda: staging(Y[:, 0])), 3)
        res["c_index_mean_score"] = float((got["mean_concordant"][0] + 0.5 * got["mean_tied"][0]) / got["comparable"][0])
        rows = min(HOST_ROWS, n)
        t0 = time.perf_counter()
        quad = [cr.concordance_ref(Y[:rows, 0], f[k, 0, :rows]) for k in range(HOST_NETS)]
        t_quad = time.perf_counter() - t0
        sub = ch.ensemble_concordance(thetas[:HOST_NETS], Y=Y[:rows], X=X[:rows])
        res["host_rows"], res["host_nets"] = rows, HOST_NETS
        res["host_quadratic_extrapolated_ms"] = round(1e3 * t_quad * (n / rows) ** 2 * M / HOST_NETS + res["forward_many_ms"], 1)
        res["equal_quadratic"] = all(quad[k] == (int(sub["comparable"][0]), int(sub["concordant"][k, 0]), int(sub["tied"][k, 0])) for k in range(HOST_NETS))
        t0 = time.perf_counter()
        fen = [fenwick_counts(Y[:, 0], f[k, 0]) for k in range(HOST_NETS)]
        t_fen = time.perf_counter() - t0
        res["host_fenwick_scaled_ms"] = round(1e3 * t_fen * M / HOST_NETS + res["forward_many_ms"], 1)
        res["equal_fenwick"] = all(fen[k] == (int(got["comparable"][0]), int(got["concordant"][k, 0]), int(got["tied"][k, 0])) for k in range(HOST_NETS))
        print(json.dumps(res), flush=True)
        ch.close()


if __name__ == "__main__":
    main()
