"""The reference of the heteroscedastic Gaussian likelihood (include/tbnn.h TBNN_LIK_HETERO_GAUSSIAN) for the tests: the oracle
(oracle/tbnn_oracle.py) has no such likelihood, so the data term and its two deltas are stated here and everything else -- the forward pass,
the priors and their gradients, the reverse mode's layer loop, the leapfrog / Metropolis step, the hyper transition -- is the oracle's, as in
tests/negbin_ref.py.

The network has exactly 2 outputs and no last activation: output 0 the mean f, output 1 the log-sd g.  Per ROW, G = log(1e8),
gc = min(max(g, -G), G), u = exp(-2 gc), r = y - f:
    log p(y | f, g) = -1/2 log(2 pi) - gc - 1/2 r^2 u
    dL/df = r u        dL/dg = r^2 u - 1 for -G <= g <= G, else 0
A row weight w_i scales the row's term and both deltas, and the constant counts W = sum w_i rows.  Targets are one per row; [n, 2] is taken
with column 1 ignored.

Two arms.  dtype=np.float64: the definition as written.  dtype=np.float32: the KERNEL's own operations in order in fp32 (csrc/common.hpp
hetero_pair): the clip as two selects, u = exp(-2 gc), r = y - f, ru = r u, q = r ru, the term -gc - 1/2 q, the deltas ru and q - 1; the
terms are summed in fp64, as the kernels' accumulators sum them, the constant is fp64, and the priors are the oracle's fp32 arm.  The
network's own arithmetic (matrix products, activations) is the oracle's in that dtype.

A spec here is the oracle's NetSpec with likelihood LIK_FIXED_GAUSSIAN and no last activation (no likelihood hyper: H = 4 layers): the
oracle's own hyper transition of such a spec is the layer priors alone, which is this likelihood's hyper transition too."""
import math

import numpy as np

import tbnn_oracle as o
from student_ref import prior_log_prob          # (the oracle's layer priors)
import student_ref as _sr

LIK_HETERO_GAUSSIAN = 12
LOG_CLIP = math.log(1e8)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def make_spec(dims, act, prior):
    assert dims[-1] == 2
    return o.make_spec(dims, act, prior, o.LIK_FIXED_GAUSSIAN, o.ACT_NONE)


def targets(Y, n):
    """the one target per row, [n]: Y is [n], [n, 1] or [n, 2] (column 0)"""
    Y = np.asarray(Y)
    return Y.reshape(n) if Y.size == n else Y.reshape(n, -1)[:, 0]


def pair(f, Y, dtype):
    """(the row terms -gc - 1/2 r^2 u [n], the deltas [2, n]: dL/df and dL/dg) in `dtype`; f [2, n]"""
    dt = dtype
    f = np.asarray(f, dtype=dt)
    y = np.asarray(targets(Y, f.shape[1]), dtype=dt)
    G = dt(LOG_CLIP)
    g = f[1]
    gc = np.where(g < -G, -G, g)
    gc = np.where(g > G, G, gc).astype(dt)
    inside = (g >= -G) & (g <= G)
    with np.errstate(over="ignore"):
        u = np.exp(dt(-2) * gc).astype(dt)
        r = (y - f[0]).astype(dt)
        ru = (r * u).astype(dt)
        q = (r * ru).astype(dt)
        term = (-gc - dt(0.5) * q).astype(dt)
        dg = np.where(inside, q - dt(1), dt(0)).astype(dt)
    return term, np.stack([ru, dg]).astype(dt)


def terms(f, Y):
    """the log density per row, fp64 [n]"""
    t, _d = pair(np.asarray(f, dtype=np.float64), Y, np.float64)
    return t - HALF_LOG_2PI


def data_log_prob(spec, f, Y, dtype=np.float64, w=None, rows=None):
    """(the data term as a float64, the statistic sum w (-gc - 1/2 r^2 u) as the kernels accumulate it); rows: the count the constant is
    taken over (default: the rows of f, or the sum of the weights)"""
    t, _d = pair(f, Y, dtype)
    if w is not None:
        t = np.asarray(w, dtype=dtype) * t                    # (the kernel: wt * term in fp32, then the fp64 sum)
    stat = float(np.sum(t.astype(np.float64)))
    if rows is None:
        rows = float(f.shape[1]) if w is None else float(np.sum(np.asarray(w, dtype=np.float64)))
    return stat - HALF_LOG_2PI * rows, stat


def target_log_prob_and_grad(spec, theta, eta, X, Y, dtype=np.float64, w=None):
    """(log posterior as a float64, its gradient in `dtype`): the oracle's target_log_prob_and_grad with this data term"""
    dt = dtype
    theta, eta = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    parts = o.unflatten(spec, theta)
    f, acts = o.forward(spec, theta, X, dt, keep=True)
    logp = float(prior_log_prob(spec, theta, eta, dt)) + data_log_prob(spec, f, Y, dt, w)[0]
    _t, d_a = pair(f, Y, dt)
    if w is not None:
        d_a = np.asarray(w, dtype=dt) * d_a
    grads = [None] * len(spec.layers)
    for i in range(len(spec.layers) - 1, -1, -1):
        l = spec.layers[i]
        W, b = parts[i]
        delta = (d_a * o.act_grad_from_output(acts[i + 1], l.act)).astype(dt)
        gW = delta @ acts[i].T
        gb = np.sum(delta, axis=1, keepdims=True, dtype=dt)
        pW, pb = o.prior_grad(l, eta[4 * i:4 * i + 4], W, b, dt)
        grads[i] = ((gW + pW).astype(dt), (gb + pb).astype(dt))
        if i > 0:
            d_a = (W.T @ delta).astype(dt)
    return logp, o.flatten(grads).astype(dt)


def prior_grad_flat(spec, theta, eta, dtype=np.float64):
    """the gradient of the layer priors alone, flat"""
    dt = dtype
    th, et = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    pg = [tuple(o.prior_grad(l, et[4 * i:4 * i + 4], W, b, dt)) for i, (l, (W, b)) in enumerate(zip(spec.layers, o.unflatten(spec, th)))]
    return o.flatten(pg).astype(dt)


def likelihood_value_and_grad(spec, theta, eta, X, Y, dtype=np.float64, w=None):
    """the data term alone and its gradient (tbnn_optimize's objective "likelihood")"""
    dt = dtype
    lp, g = target_log_prob_and_grad(spec, theta, eta, X, Y, dt, w)
    return lp - float(prior_log_prob(spec, np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt), dt)), (g - prior_grad_flat(spec, theta, eta, dt)).astype(dt)


def weight_step(spec, theta, eta, X, Y, eps, L, p0, log_u, dtype=np.float64, w=None):
    """one weight transition: the oracle's leapfrog and Metropolis step over this module's value and gradient (energies in fp64)"""
    vg = lambda q: target_log_prob_and_grad(spec, q, eta, X, Y, dtype, w)
    return o.hmc_step(vg, theta, eps, L, p0, log_u, dtype, np.float64)


def hyper_step(spec, eta, theta, X, Y, eps_h, L_h, p0, log_u, dtype=np.float64):
    """the hyper transition: no likelihood hyper and no data term -- the oracle's own for a fixed-sd spec"""
    assert spec.likelihood == o.LIK_FIXED_GAUSSIAN
    return o.hyper_step(spec, eta, theta, np.asarray(X), np.zeros((len(X), 2), np.float32), eps_h, L_h, p0, log_u, dtype)


def last_bias_index(spec, out=1):
    """the position in theta of the last layer's bias of output `out`"""
    off = 0
    for l in spec.layers[:-1]:
        off += l.in_dim * l.out_dim + l.out_dim
    l = spec.layers[-1]
    return off + l.in_dim * l.out_dim + out


# ---- the cases of tests/test_gpu_hetero.py (tests/test_hetero_host.py judges the fp32 arm on the same problems): student_ref.CASES' row
# counts, activations, priors and environments, every network ending in 2 -- the smallest shapes with ragged last tiles that reach each kernel
def _two(name, rows=None):
    dims, n, act, prior, fam, env = _sr.CASES[name][:6]
    return (dims[:-1] + [2], n if rows is None else rows, act, prior, fam, dict(env))


CASES = {
    # dims, rows, hidden activation, prior, family, environment
    "fast3": _two("fast3"),
    "fast3_two_outputs": _two("fast3_two_outputs"),
    "fast": _two("fast"),                                  # TBNN_JIT_SKIP=fast3
    "mid": _two("mid1"),
    "tall": _two("tall"),
    "wide": _two("wide1"),
    "lay_last": _two("lay_last"),                          # k_lay_last
    "lay_separate": _two("lay_separate"),                  # TBNN_LAY_LAST=0: k_lay_lik
    "lay_tail": _two("lay_tail"),                          # k_lay_tail
    "generic": _two("generic"),
    # the trajectory kernel: with two outputs 1-10-10-2 holds one more fringe sum per tile than 1-10-10-1 and runs it with 4 waves per
    # workgroup, not 16 (kernels_traj.hpp: TrajCfg::REGS_OK), which takes at most 384 rows (TBNN_TRAJ_MAX_ROWS_4) -- student_ref's 500 rows
    # would run on the per-step kernels, so this case alone has its own row count: 380, the nearest ragged one that reaches the kernel
    "traj": _two("traj", rows=380),
}
CLIP_CASES = ("generic", "fast3")                          # the last bias of output 1 at +-25: g beyond the clip on every row


def problem_of(dims, n, act, prior, seed=11):
    """(spec, X, Y [n], theta, eta): the oracle's synthetic rows and initial state.  The targets are drawn from the model: the mean is the
    oracle's teacher's (standardised) output 0, the noise sd rises 10x over the rows, s = 0.1 * 10^v with v uniform on [0, 1].  So that
    both regimes of the term occur in every 16-row tile at the INITIAL state (f, g there), the first row of each tile is moved to
    f + 0.03 e^g (r^2 u ~ 1e-3) and the second to f + 10 e^g either way (r^2 u = 100), as student_ref moves its outliers."""
    _g, X, Yr, theta, eta = o.synth_problem(dims, n, act, prior, o.LIK_GAUSSIAN)
    spec = make_spec(dims, act, prior)
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1)
    eta = np.asarray(eta[:spec.n_hypers], dtype=np.float32)          # no likelihood hyper
    # the initial state's log-sd output scaled down (its row of the last layer's weights and its bias times 1/4): |g| < 6 on every row of
    # every case, far from the clip (the clip has its own cases), and sd's from e^-2 to e^2 rather than e^-6.6 to e^6.4
    parts = [(W.copy(), b.copy()) for W, b in o.unflatten(spec, np.asarray(theta, dtype=np.float32))]
    parts[-1][0][1, :] *= np.float32(0.25)
    parts[-1][1][1] *= np.float32(0.25)
    theta = o.flatten(parts).astype(np.float32)
    rng = np.random.default_rng(seed)
    mean = np.asarray(Yr, dtype=np.float64).reshape(n, -1)[:, 0]
    s = 0.1 * 10.0 ** rng.random(n)
    Y = mean + s * rng.standard_normal(n)
    f0 = o.forward(spec, np.asarray(theta, np.float64), np.asarray(X, np.float64), np.float64)
    sg = np.exp(np.clip(f0[1], -LOG_CLIP, LOG_CLIP))
    sign = rng.choice([-1.0, 1.0], n)
    idx = np.arange(n)
    near, far = idx % 16 == 0, idx % 16 == 1
    Y[near] = f0[0][near] + 0.03 * sg[near] * sign[near]
    Y[far] = f0[0][far] + 10.0 * sg[far] * sign[far]
    return spec, X, Y.astype(np.float32), theta, eta


_PROBLEMS = {}


def problem(name):
    """a case's problem: computed once per process and left unchanged"""
    if name not in _PROBLEMS:
        dims, n, act, prior, _fam, _env = CASES[name]
        _PROBLEMS[name] = problem_of(dims, n, act, prior)
    return _PROBLEMS[name]


_REF64 = {}


def ref64(name):
    """the fp64 value and gradient of a case at its state: once per process"""
    if name not in _REF64:
        spec, X, Y, theta, eta = problem(name)
        _REF64[name] = target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)
    return _REF64[name]


def step_size(name):
    """the leapfrog step of a case's injected transition (4 steps; the trajectory case: 1 and 9)"""
    return _sr.step_size(name)
