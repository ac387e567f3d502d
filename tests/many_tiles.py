"""The cases of the many-tiles tests (tests/test_gpu_many_tiles.py on the device, tests/test_many_tiles_host.py for the plan and the fp32 arm).

In the one-kernel fused families a wave walks a strided list of 16-row tiles and the launch has at most 256 workgroups, so below about
16 k rows a wave runs one tile and the loop's back edge -- the prefetch of the next tile's X, Y and row weight, the scalar row pointers
and their steps, fetch(tile + W), the carry of dW, stat and the fringe sums, the ragged-tile selects, the cooperative rounds -- is never
taken.  The kernels are templates over the likelihood and the weighted bit, and every instantiation has its own copy of that code.  The
likelihood modules run at most 3,001 rows on the default grid; here every likelihood, weighted and not, runs a few hundred rows on the
small grid of the test hook TBNN_FAST_GRID, where a wave takes several trips.

No shape of its own: every case names a case of a table the suite already has (`owner`, `name`) and takes its network, activation, prior,
likelihood parameters and TBNN_JIT_SKIP from there, so every run-time library is one those modules compile (tests/test_gpu_multiout.py,
which lends the Bernoulli case of the MFMA output tile, has no jit_jobs() of its own: its libraries are listed in tests/jit_shapes.json,
which the build compiles ahead); the problem is the owner's generator at the new row count, with its conditioning.  One case family
has other data: mid_bern of tests/test_gpu_row_weights.py carries the conditioning of tests/test_gpu_multiout.py on top of its
generator (the state times 0.3).  At the generator's own state its sigmoids
land on the clip and the oracle's fp32 arm itself is 8 to 14 value bands away from fp64 at 381, 333 and 173 rows (that module says so
of mid_bern and judges it against repeated rows only); scaled, it is inside 0.02 of a band.

Row counts.  Narrow (fast3, fast; TBNN_FAST_GRID=2: 8 waves; `split` of tests/test_gpu_narrow_rows.py) and mid (the same grid; `mid_plan`
below) in NARROW_ROWS and MID_ROWS.  Tall: 1,007 rows on 3 workgroups (`tall_plan`).  Wide has no grid hook: 17,009 rows, the N_WIDE of
tests/test_gpu_capacity.py, so that its waves carry more than one tile."""
import collections
import functools
import json
import os

import numpy as np

import gamma_ref as gr
import hetero_ref as hr
import negbin_ref as nb
import student_ref as sr
import tbnn_oracle as o
import test_gpu_gamma as gam
import test_gpu_hetero as het
import test_gpu_multiout as mo
import test_gpu_negbin as neg
import test_gpu_poisson as poi
import test_gpu_row_weights as rw
import test_gpu_student as stu
from tensor_checks import layers_of, tensor_errs
from test_gpu_capacity import N_WIDE
from test_gpu_narrow_rows import split

GRID = 2                                   # TBNN_FAST_GRID of the narrow and mid cases: W = 8 waves
TALL_GRID, TALL_ROWS = 3, 1007             # as tests/test_gpu_capacity.py runs the tall family
NARROW_ROWS = {"ragged-last-trip": 381,    # 24 tiles: three trips per wave, the ragged tile is wave 7's last
               "ragged-coop-tile": 393,    # 25 tiles: the ragged tile is the cooperative tile
               "two-coop-rounds": 173,     # 11 tiles: one trip, two cooperative rounds, the second one ragged
               "uneven-trips": 333}        # 21 tiles: waves 0 .. 4 three trips, 5 .. 7 two: the absent next tile falls on different trips
MID_ROWS = {"ragged-last-trip": 381, "uneven-trips": 333, "no-ragged-tile": 384}
LOGP_BAND, GRAD_BAND, STAT_BAND, FLOOR = 4e-6, 1e-4, 4e-6, 1e-3

# the likelihood's tag in a run-time kernel's name (csrc/fused_ops.hpp: fused_ops_shape)
TAG = {"gaussian": None, "bernoulli": "bernoulli", "categorical": "categorical", "poisson": "poisson", "negbin": "neg-binomial",
       "student": "student-t", "hetero": "hetero-gaussian", "gamma": "gamma"}

Case = collections.namedtuple("Case", "id family path lik weighted owner name rows grid zero_ragged")

# owner -> (its table, its TBNN_JIT_SKIP per family or None when the table carries it, its jit_jobs)
OWNERS = {"student": (sr.CASES, stu.FUSED, stu.jit_jobs), "negbin": (nb.CASES, neg.FUSED, neg.jit_jobs), "hetero": (hr.CASES, het.FUSED, het.jit_jobs),
          "poisson": (poi.CASES, poi.FUSED, poi.jit_jobs), "gamma": (gr.CASES, gam.FUSED, gam.jit_jobs), "rw": (rw.CASES, None, rw.jit_jobs), "multiout": (mo.CASES, mo.SKIP, None)}
FAMILY_AT = {"multiout": 5}                 # where an owner's table holds the kernel family (the others: 4)
LIK_OF_OWNER = {"student": "student", "negbin": "negbin", "hetero": "hetero", "poisson": "poisson", "gamma": "gamma"}
RW_LIK = {o.LIK_GAUSSIAN: "gaussian", o.LIK_BERNOULLI: "bernoulli", o.LIK_CATEGORICAL: "categorical"}
SHAPES_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jit_shapes.json")

# (family, last-layer path, owner, case of the owner's table, has a weighted library)
CELLS = [
    # fast3: k_fwd_bwd_fast3 -- the scalar row pointers Xq / Yq / Wq and their steps
    ("fast3", "valu1", "rw", "fast3_configs1", True), ("fast3", "valu1", "rw", "fast3_bern", True), ("fast3", "valu1", "poisson", "fast3", True),
    ("fast3", "valu1", "student", "fast3", True), ("fast3", "valu1", "negbin", "fast3", True), ("fast3", "valu2", "hetero", "fast3", True),
    ("fast3", "valu2", "student", "fast3_two_outputs", False), ("fast3", "valu2", "poisson", "fast3_two_outputs", False),
    ("fast3", "valu1", "gamma", "fast3", True), ("fast3", "valu2", "gamma", "fast3_two_outputs", False),
    # fast: k_fwd_bwd_fast
    ("fast", "valu2", "rw", "fast_gauss", True), ("fast", "valu2", "rw", "fast_bern", True), ("fast", "valu1", "poisson", "fast", False),
    ("fast", "valu1", "student", "fast", False), ("fast", "valu1", "negbin", "fast", False), ("fast", "valu2", "hetero", "fast", False),
    ("fast", "valu1", "gamma", "fast", True),
    # mid, the VALU last layer of one or two outputs
    ("mid", "valu1", "student", "mid1", False), ("mid", "valu1", "negbin", "mid1", False), ("mid", "valu1", "poisson", "mid1", False),
    ("mid", "valu2", "hetero", "mid", False), ("mid", "valu2", "rw", "mid_bern", True), ("mid", "valu1", "gamma", "mid1", False),
    # mid, the MFMA output tile (10 outputs: Y in the D layout, cat_delta4)
    ("mid", "mfma10", "rw", "mid_gauss", True), ("mid", "mfma10", "rw", "mid_cat", True), ("mid", "mfma10", "multiout", "bern10", False),
    ("mid", "mfma10", "poisson", "mid10", False),
    ("mid", "mfma10", "student", "mid10", False), ("mid", "mfma10", "negbin", "mid10", False),
    ("mid", "mfma10", "gamma", "mid10", True),          # (row weights with Y in the D layout under a log-link likelihood)
    # tall
    ("tall", "valu1", "rw", "tall_gauss", True), ("tall", "valu1", "poisson", "tall", False), ("tall", "mfma10", "rw", "tall_cat", True),
    ("tall", "valu1", "gamma", "tall", False),
    # wide
    ("wide", "valu1", "student", "wide1", False), ("wide", "mfma10", "student", "wide10", False), ("wide", "valu1", "poisson", "wide1", False),
    ("wide", "mfma10", "poisson", "wide10", False), ("wide", "mfma10", "rw", "wide_gauss", True), ("wide", "mfma10", "rw", "wide_cat", True),
    ("wide", "valu1", "gamma", "wide1", False), ("wide", "mfma10", "gamma", "wide10", False),
]
# weighted cases that run once more with every row of the ragged tile at weight 0: (family, owner, name, rows)
ZERO_RAGGED = [("fast3", "rw", "fast3_configs1", 381), ("fast3", "hetero", "fast3", 393), ("fast", "rw", "fast_bern", 381),
               ("mid", "rw", "mid_gauss", 381), ("mid", "rw", "mid_bern", 333), ("fast", "gamma", "fast", 381)]


def lik_of(owner, name):
    if owner in LIK_OF_OWNER:
        return LIK_OF_OWNER[owner]
    return RW_LIK[rw.CASES[name][3] if owner == "rw" else mo.CASES[name][4]]


def _cases():
    out = []
    for fam, path, owner, name, has_w in CELLS:
        assert OWNERS[owner][0][name][FAMILY_AT.get(owner, 4)] == fam, (owner, name)
        rows = NARROW_ROWS if fam in ("fast3", "fast") else MID_ROWS if fam == "mid" else {"": TALL_ROWS if fam == "tall" else N_WIDE}
        grid = GRID if fam in ("fast3", "fast", "mid") else TALL_GRID if fam == "tall" else None
        lik = lik_of(owner, name)
        for key, n in rows.items():
            for w in ((False, True) if has_w else (False,)):
                cid = "-".join(x for x in (fam, path, lik, "weighted" if w else "", f"{n}rows") if x)
                out.append(Case(cid, fam, path, lik, w, owner, name, n, grid, False))
                if w and (fam, owner, name, n) in ZERO_RAGGED:
                    out.append(Case(cid + "-zero-ragged", fam, path, lik, w, owner, name, n, grid, True))
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def skip_of(case):
    """the owner's TBNN_JIT_SKIP for the case's family: what selects the family and names the library"""
    table, fused, _jobs = OWNERS[case.owner]
    return table[case.name][5] if fused is None else fused[case.family]


def spec_of(case):
    return problem(case)[0]


def job_of(case, weighted):
    """the job of jit.prebuild that compiles the case's library (weighted: the one set_row_weights selects)"""
    spec = spec_of(case)
    j = {"layers": [list(l) for l in layers_of(spec)], "likelihood": spec.likelihood, "skip": skip_of(case), "flags": ""}
    if weighted:
        j["weighted"] = True
    return j


def aot(case):
    """the one case family whose unweighted side is an ahead-of-time table (no run-time library)"""
    return case.owner == "rw" and case.name == "fast3_configs1"


def jit_jobs():
    """the run-time instantiations the device module loads: for every case its unweighted library (a weighted case clears its weights too)
    and, where weighted, its weighted one -- each one a job of its owner's jit_jobs() (tests/test_many_tiles_host.py asserts it)"""
    jobs = []
    for c in CASES:
        if not aot(c):
            jobs.append(job_of(c, False))
        if c.weighted:
            jobs.append(job_of(c, True))
    return [j for i, j in enumerate(jobs) if j not in jobs[:i]]


def owners_jobs():
    """the union of the owning modules' jit_jobs(); for the one owner without a jit_jobs() the list the build compiles ahead"""
    jobs = []
    for _table, _fused, jj in OWNERS.values():
        jobs += jj() if jj is not None else json.load(open(SHAPES_JSON))
    return jobs


def _problem_of(owner, name, n):
    if owner == "rw":
        spec, X, Y, theta, eta = rw.problem(name, n)
        if name == "mid_bern":
            theta = (theta * 0.3).astype(np.float32)          # outputs off saturation (tests/test_gpu_multiout.py): see the docstring
        return spec, X, Y, theta, eta
    if owner == "multiout":
        # its generator takes the row count from its table; the first n rows ARE the problem of n rows (synth_problem draws row by row)
        spec, X, Y, theta, eta = mo.problem(name)
        assert n <= X.shape[0]
        return spec, X[:n], Y[:n], theta, eta
    c = OWNERS[owner][0][name]
    gen = {"student": sr.problem_of, "negbin": nb.problem_of, "hetero": hr.problem_of, "poisson": poi.problem_of, "gamma": gr.problem_of}[owner]
    return gen(c[0], n, c[2], c[3], *c[6:])


@functools.lru_cache(maxsize=None)
def _problem(owner, name, n):
    out = _problem_of(owner, name, n)
    arrays = tuple(np.ascontiguousarray(a) for a in out[1:])
    for a in arrays:
        a.setflags(write=False)
    return (out[0],) + arrays


def problem(case):
    """(spec, X, Y, theta, eta) of a case: the owner's generator at the case's row count, computed once and read-only"""
    return _problem(case.owner, case.name, case.rows)


def weights(case):
    """uniform(0.25, 2) with every seventh row at 0, as tests/test_gpu_row_weights.py has its zeros; zero_ragged: every row of the ragged
    tile at 0 as well"""
    n = case.rows
    w = np.random.default_rng(3).uniform(0.25, 2.0, n).astype(np.float32)
    w[::7] = 0.0
    if case.zero_ragged:
        assert n % 16
        w[n - n % 16:] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def _ref64(cid, weighted):
    c = BY_ID[cid]
    spec, X, Y, theta, eta = problem(c)
    w = weights(c) if weighted else None
    lp, g = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64, w=w)
    g.setflags(write=False)
    return float(lp), g, statistic(spec, theta, eta, X, Y, np.float64, w)


def ref64(case, weighted=None):
    """(log-prob, gradient, statistic) of the oracle in fp64, under the case's weights (weighted=False: without them); computed once"""
    return _ref64(case.id, case.weighted if weighted is None else weighted)


def statistic(spec, theta, eta, X, Y, dtype, w=None):
    """what tbnn_logp_grad returns as stat, from the oracle: sum w (y - f)^2 under the Gaussian likelihood, sum w log1p(u) under Student-t,
    the (weighted) log-likelihood with its constant under the others (Gamma: factor and constant included, as its module judges it)"""
    f = o.forward(spec, np.asarray(theta, dtype), np.asarray(X, dtype), dtype)
    if spec.likelihood == o.LIK_GAUSSIAN:
        r2 = ((np.asarray(Y, dtype).reshape(f.shape[1], -1).T - f) ** 2).sum(axis=0)
        return float(np.sum(r2 if w is None else np.asarray(w, dtype) * r2, dtype=np.float64))
    if spec.likelihood == o.LIK_STUDENT_T:
        return float(o.data_statistic(spec, eta, f, Y, dtype, w))
    return float(o.log_likelihood(spec, eta, f, Y, dtype, w))


def stat_gap(case, lp, st, lp64, st64):
    """(error, band) of a statistic, by the rule of the likelihood's own module: Student-t, negative binomial, heteroscedastic and Gamma
    4e-6 of the statistic (tests/test_gpu_student.py, test_gpu_negbin.py, test_gpu_hetero.py, test_gpu_gamma.py: the data term with its
    constant); Poisson: logp - stat, the priors, within 4e-6 of
    max(|logp|, 1) (tests/test_gpu_poisson.py: the statistic carries the fp64 constant); Gaussian, Bernoulli and categorical, whose
    modules do not judge it: 4e-6 of the statistic, as the first three"""
    if case.lik == "poisson":
        return abs((lp - st) - (lp64 - st64)), STAT_BAND * max(abs(lp), 1.0)
    return abs(st - st64), STAT_BAND * abs(st64)


def gaps(case, spec, lp, g, st, ref):
    """(value error over its band, worst tensor's gradient error over its band, statistic error over its band) against ref = ref64(...)"""
    lp64, g64, st64 = ref
    es, bs = stat_gap(case, lp, st, lp64, st64)
    return (abs(lp - lp64) / max(abs(lp64), 1.0) / LOGP_BAND, max(tensor_errs(spec, g, g64, FLOOR)) / GRAD_BAND, es / bs)


# ---- the plans, restated from the kernels
def mid_plan(n, G=GRID):
    """k_fwd_bwd_mid's loop `for (tile = wave; tile < ntiles; tile += W)` restated: (trips per wave, (wave, trip) of the ragged tile or
    None, the waves whose tile + W is past ntiles on a trip on which another wave goes on)"""
    W, ntiles = 4 * G, (n + 15) // 16
    trips = [len(range(w, ntiles, W)) for w in range(W)]
    ragged = ((ntiles - 1) % W, (ntiles - 1) // W) if n % 16 else None
    return trips, ragged, [w for w in range(W) if 0 < trips[w] < max(trips)]


def tall_plan(n, G=TALL_GRID, gmax=4):
    """tall_group_tiles / tall_grid / the group loop of k_fwd_bwd_tall restated (TallCfg::GMAX = 4): (tiles per group, groups, groups
    per workgroup, rows of the last group)"""
    ntiles = (n + 15) // 16
    best, best_cost = 1, 0
    for g in range(1, gmax + 1):
        groups = (ntiles + g - 1) // g
        cost = ((groups + 255) // 256) * (23 * g + 58)
        if g == 1 or cost < best_cost:
            best, best_cost = g, cost
    ngroups = (ntiles + best - 1) // best
    rounds = (ngroups + 255) // 256
    grid = min((ngroups + rounds - 1) // rounds, G)
    return best, ngroups, [len(range(b, ngroups, grid)) for b in range(grid)], n - (ngroups - 1) * best * 16


def default_grid(case):
    """the workgroups of the family's launch without the test hook (jit_narrow.hpp: grid, kernels_mid.hpp: mid_grid, kernels_tall.hpp:
    tall_grid at one round)"""
    if case.family == "tall":
        return len(tall_plan(case.rows, G=256)[2])
    return min(((case.rows + 15) // 16 + 3) // 4, 256)
