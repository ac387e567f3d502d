"""The plans of the reject tests (tests/test_gpu_rejects.py on the device, tests/test_rejects_host.py for the plans on the oracle alone).

A transition that diverges is rejected: `non-finite -> -inf -> reject` in the oracle's hmc_step and in k_energy.  After it the device holds
non-finite values in the proposal, its weight image, both gradients, the momentum, the gradient slabs and the statistic partials, and the
chain is right only if what it cached at the current state (q_cur, g_cur, gd_cur, the scalar record's stat_cur / prior_cur / logp_cur, the
flags cur_valid and q_img_valid) survives bit for bit.  The tests state that as an invariance, with no model of the handle:

    baseline   T0 (accepted, log u = -1e30), T2 (log u = log 0.5)
    disturbed  T0, one disturbance of DISTURBANCES, T2

and T2 is the same in both runs, bit for bit; T2 of the baseline is also judged against the fp64 oracle started from the state T0 left.

A case is a kernel family and a transition end.  The Gaussian cases are the smallest ahead-of-time shapes of tests/test_gpu_multichain.py
(jit=False), built by o.synth_problem; the other likelihoods and the row weights name a case of a table the suite already has (as
tests/many_tiles.py does: the owner's network, its TBNN_JIT_SKIP, its run-time library, its problem generator -- o.synth_problem with the
likelihood's own targets -- at a few hundred rows).

Step sizes.  `eps`: a sane step (T0, T2).  `eps_huge`: the proposal's energies are huge and finite, the log accept ratio finite and below
-1e3 (it must also fit the record's fp32 field).  EPS_NAN: the proposal is not finite, in fp32 and in fp64.  They were picked per case on
the CPU (the oracle's fp32 and fp64 arms) and tests/test_rejects_host.py holds them to those definitions before any GPU time is spent."""
import collections
import functools
import math

import numpy as np

import many_tiles as mt
import tbnn_oracle as o
from tensor_checks import layers_of

LOG_HALF = float(np.log(0.5))
L = 3                                      # leapfrog steps of every weight transition but the chain groups' own
L_H = 5                                    # of every hyper transition
EPS_NAN = 1e30                             # the weight step whose proposal is not finite
EPS_H, EPS_H_NAN = 1e-4, 1e30              # the sane hyper step and the one whose proposal is not finite
EPOCH = 11                                 # where both runs enter T2
SEED, CID = 50, 3                          # of the free-running variant and the chain groups
MARGIN = 0.1                               # |log accept ratio - log u| of T2 on the oracle, so that its decision is no coin toss
REC = ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new", "sjd", "accept_prob")
DISTURBANCES = ("forced-reject", "huge-finite", "non-finite", "queued-epochs", "probes", "diverged-hyper-step", "non-finite-then-hyper-step")
HYPER = ("diverged-hyper-step", "non-finite-then-hyper-step")          # need hypers; the last one has a baseline of its own

OFF = {"TBNN_TALL": "0", "TBNN_REGISTERED": "0"}                       # layered / generic whatever another module registered in this process
PER_STEP = {"TBNN_TRAJ": "0"}

# id: family, path, exact kernel name or (prefix, token), environment, source, eps, eps_huge
#   source ("synth", dims, rows, hidden activation, prior, likelihood) or ("owner", owner, case of its table, rows, weighted): many_tiles.OWNERS
_TABLE = {
    # ---- the Gaussian likelihood (sampled sigma) on every family, ahead-of-time shapes
    "fast3": ("fast3", "per-step", "fast3<relu;1,10,10,1>", PER_STEP, ("synth", [1, 10, 10, 1], 1000, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN), 0.0002, 0.03),
    "fast3-trajectory": ("fast3", "trajectory", "fast3<relu;1,10,10,1>", {"TBNN_TRAJ": "1"},
                         ("synth", [1, 10, 10, 1], 1000, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN), 0.0002, 0.03),
    "fast3-unmerged-end": ("fast3", "per-step", "fast3<relu;1,10,10,1>", {"TBNN_TRAJ": "0", "TBNN_MERGE_ENDS": "0"},
                           ("synth", [1, 10, 10, 1], 1000, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN), 0.0002, 0.03),
    "fast": ("fast", "per-step", "fast<sigmoid;4,7,3>", PER_STEP, ("synth", [4, 7, 3], 130, o.ACT_SIGMOID, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN), 0.0002, 0.3),
    "mid": ("mid", "per-step", "mid<tanh;4,24,40,1>", PER_STEP, ("synth", [4, 24, 40, 1], 517, o.ACT_TANH, o.PRIOR_GAUSSIAN, o.LIK_GAUSSIAN), 0.0002, 0.03),
    "tall": ("tall", "per-step", ("tall<", "128,16,2>"), PER_STEP, ("synth", [128, 16, 2], 333, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN), 0.0002, 0.1),
    "wide": ("wide", "per-step", "wide<tanh;3,20,36,2>", {"TBNN_TRAJ": "0", "TBNN_MID": "0"},
             ("synth", [3, 20, 36, 2], 517, o.ACT_TANH, o.PRIOR_GAUSSIAN, o.LIK_GAUSSIAN), 0.0002, 0.03),
    "layered": ("layered", "per-step", ("layered<", ""), dict(OFF, **PER_STEP),
                ("synth", [40, 24, 24, 3], 600, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN), 0.0002, 0.1),
    "generic": ("generic", "per-step", "generic", dict(OFF, **PER_STEP), ("synth", [5, 16, 16, 4], 517, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN), 0.0002, 0.1),
    # P = 82,801 > 32,768: the three-launch end (k_commit, k_commit_scal) and k_update's 32 x 16 geometry
    "wide-unmerged-big-p": ("wide", "per-step", "wide<relu;10,200,200,200,1>", {"TBNN_TRAJ": "0", "TBNN_MID": "0"},
                            ("synth", [10, 200, 200, 200, 1], 300, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN), 0.0001, 0.003),
    # ---- the other likelihoods, spread over the families
    # (the Gaussian prior: with the Cauchy prior every term of a Bernoulli target's gradient is bounded, and no step size carries the fp64
    # arm out of its range in three steps)
    "mid-bernoulli": ("mid", "per-step", "mid<sigmoid,sigmoid,bernoulli;20,32,48,2>", PER_STEP,
                      ("synth", [20, 32, 48, 2], 700, o.ACT_SIGMOID, o.PRIOR_GAUSSIAN, o.LIK_BERNOULLI), 0.0001, 0.3),
    "tall-poisson": ("tall", "per-step", ("jit-tall<", "poisson"), PER_STEP, ("owner", "poisson", "tall", 333, False), 0.0001, 0.01),
    "wide-student": ("wide", "per-step", ("jit-wide<", "student-t"), PER_STEP, ("owner", "student", "wide1", 333, False), 0.0001, 0.03),
    "fast-negbin": ("fast", "per-step", ("jit-fast<", "neg-binomial"), PER_STEP, ("owner", "negbin", "fast", 333, False), 0.0002, 0.03),
    "fast3-hetero": ("fast3", "per-step", ("jit-fast3<", "hetero-gaussian"), PER_STEP, ("owner", "hetero", "fast3_two_outputs", 333, False), 0.0002, 0.02),
    "mid-hetero": ("mid", "per-step", ("jit-mid<", "hetero-gaussian"), PER_STEP, ("owner", "hetero", "mid", 333, False), 0.0002, 0.1),
    # ---- row weights
    "fast3-weighted": ("fast3", "per-step", ("jit-fast3<", "weighted"), PER_STEP, ("owner", "rw", "fast3_configs1", 333, True), 0.0002, 0.01),
    "mid-weighted": ("mid", "per-step", ("jit-mid<", "weighted"), PER_STEP, ("owner", "rw", "mid_gauss", 333, True), 0.0002, 0.03),
}
Case = collections.namedtuple("Case", "id family path kernel env source eps eps_huge")
CASES = [Case(k, *v) for k, v in _TABLE.items()]
BY_ID = {c.id: c for c in CASES}
# chain groups: the families whose group shares launches (narrow per-step and trajectory, mid, tall) and one chain-by-chain family
GROUP_CASES = ("fast3", "fast3-trajectory", "mid", "tall", "wide")


def owner_case(c):
    """the case of tests/many_tiles.py that names the owner's table entry, or None for a synth case"""
    if c.source[0] != "owner":
        return None
    _o, owner, name, rows, weighted = c.source
    return mt.Case(c.id, c.family, None, mt.lik_of(owner, name), weighted, owner, name, rows, None, False)


@functools.lru_cache(maxsize=None)
def _problem(cid):
    c = BY_ID[cid]
    return _sigma_one(mt.problem(owner_case(c)) if c.source[0] == "owner" else _synth(c))


def _synth(c):
    out = o.synth_problem(*c.source[1:])
    arrays = tuple(np.ascontiguousarray(a) for a in out[1:])
    if c.source[1][0] > 64:                                              # keep a long fan-in's pre-activations O(1), as the owners' generators do
        arrays = ((arrays[0] / np.sqrt(c.source[1][0] / 16.0)).astype(np.float32),) + arrays[1:]
    return (out[0],) + tuple(_readonly(a) for a in arrays)


def _readonly(a):
    a.setflags(write=False)
    return a


def _sigma_one(prob):
    """a Gaussian case's likelihood sd at 1, not at the 0.1 of o.default_hypers.  The targets are standardised, so the start state's
    residuals are O(1): under sd 0.1 the log-prob of a few hundred rows is 1e5 .. 1e6, where the fp32 arithmetic of the REFERENCE (the
    oracle's fp32 arm) is itself up to four of the anchor's bands away from fp64 in the log accept ratio; under sd 1 it is inside half a
    band in every case (tests/test_rejects_host.py asserts it), so the bands are a fair demand on an fp32 kernel"""
    spec, X, Y, theta, eta = prob
    if spec.likelihood != o.LIK_GAUSSIAN:
        return prob
    eta = np.array(eta, dtype=np.float32)
    eta[-1] = 1.0
    assert float(o.likelihood_sigma(spec, eta, np.float64)) == 1.0
    return spec, X, Y, theta, _readonly(eta)


def problem(c):
    """(spec, X, Y, theta, eta) of a case, computed once and read-only"""
    return _problem(c.id)


def weights(c):
    """the case's row weights (many_tiles.weights: uniform(0.25, 2) with every seventh row at 0) or None"""
    oc = owner_case(c)
    return mt.weights(oc) if oc is not None and oc.weighted else None


def jit_of(c):
    return c.source[0] == "owner"


def env_of(c):
    env = dict(c.env)
    if jit_of(c):
        env["TBNN_JIT_SKIP"] = mt.skip_of(owner_case(c))
    return env


def jit_jobs():
    """the run-time instantiations the device module loads, each one a job of its owner's jit_jobs() (tests/test_rejects_host.py asserts it)"""
    jobs = []
    for c in CASES:
        oc = owner_case(c)
        if oc is None:
            continue
        if not mt.aot(oc):
            jobs.append(mt.job_of(oc, False))
        if oc.weighted:
            jobs.append(mt.job_of(oc, True))
    return [j for i, j in enumerate(jobs) if j not in jobs[:i]]


def kernel_ok(c, name):
    want = c.kernel
    return name == want if isinstance(want, str) else (name.startswith(want[0]) and want[1] in name)


# ---- the draws
def momentum(c, which):
    """the injected momentum of "T0", the disturbance ("D") or "T2"; of the hyper transitions: "H" """
    spec = problem(c)[0]
    k = {"T0": 100, "D": 101, "T2": 102, "H": 103}[which]
    n = spec.n_hypers if which == "H" else spec.n_params
    return np.random.default_rng(k).standard_normal(n).astype(np.float32)


def theta_probes(c, theta):
    """(theta_bad, a sane second theta) of the probes: 1e30 * theta, which leaves fp32's range, and theta moved by a per cent"""
    with np.errstate(over="ignore"):
        bad = (np.float32(1e30) * np.asarray(theta, np.float32)).astype(np.float32)
    return bad, (np.asarray(theta, np.float32) * np.float32(1.01)).astype(np.float32)


def group_states(c, n_chains=3):
    """every chain of a group its own perturbed theta (as tests/test_gpu_multichain.py)"""
    theta = problem(c)[3]
    rng = np.random.default_rng(2)
    return (theta[None, :] * (1.0 + 0.05 * rng.standard_normal((n_chains, theta.size)))).astype(np.float32)


# ---- the plans on the oracle
Plan = collections.namedtuple("Plan", "t0 t2 forced huge nan hyper_nan hyper_ok t2_after_hyper")


def arm(dtype):
    return dict(dtype=dtype, energy_dtype=np.float64) if dtype is np.float32 else dict(dtype=dtype)


@functools.lru_cache(maxsize=None)
def _plan(cid, fp64):
    c = BY_ID[cid]
    spec, X, Y, theta, eta = problem(c)
    w, kw = weights(c), arm(np.float64 if fp64 else np.float32)
    step = lambda th, et, eps, which, lu: o.weight_step(spec, th, et, X, Y, eps, L, momentum(c, which), lu, w=w, **kw)
    with np.errstate(all="ignore"):
        t0 = step(theta, eta, c.eps, "T0", -1e30)
        th = t0.theta
        t2 = step(th, eta, c.eps, "T2", LOG_HALF)
        forced = step(th, eta, c.eps, "D", 1e30)
        huge = step(th, eta, c.eps_huge, "D", LOG_HALF)
        nan = step(th, eta, EPS_NAN, "D", LOG_HALF)
        hyper_nan = hyper_ok = t2h = None
        if spec.n_hypers:
            hyper_nan = o.hyper_step(spec, eta, th, X, Y, EPS_H_NAN, L_H, momentum(c, "H"), LOG_HALF, w=w, **kw)
            hyper_ok = o.hyper_step(spec, eta, th, X, Y, EPS_H, L_H, momentum(c, "H"), -1e30, w=w, **kw)
            t2h = step(th, hyper_ok.theta, c.eps, "T2", LOG_HALF)
    return Plan(t0, t2, forced, huge, nan, hyper_nan, hyper_ok, t2h)


def plan(c, dtype):
    """the case's transitions on the oracle's fp32 arm (energies in fp64, as the device sums them) or its fp64 arm, computed once"""
    return _plan(c.id, dtype is np.float64)


@functools.lru_cache(maxsize=None)
def _free_run(cid, fp64):
    c = BY_ID[cid]
    spec, X, Y, theta, eta = problem(c)
    w, kw = weights(c), arm(np.float64 if fp64 else np.float32)
    th, out = theta, []
    with np.errstate(all="ignore"):
        for e, eps in enumerate((c.eps, c.eps, EPS_NAN, EPS_NAN)):
            p0 = o.philox_normals(spec.n_params, SEED, CID, e, o.PURPOSE_MOMENTUM)
            lu = float(o.philox_log_uniform(SEED, CID, e, o.PURPOSE_LOGU))
            r = o.weight_step(spec, th, eta, X, Y, eps, L, p0, lu, w=w, **kw)
            th = r.theta
            out.append(r)
    return out


def free_run(c, dtype):
    """the first four epochs of the free-running variant on the chain's own Philox draws: two at eps, two at EPS_NAN"""
    return _free_run(c.id, dtype is np.float64)


def finite(x):
    return bool(np.all(np.isfinite(np.asarray(x, dtype=np.float64))))


def is_minus_inf(x):
    return isinstance(x, float) and math.isinf(x) and x < 0
