"""The reference of the Weibull likelihood with right-censored targets (include/tbnn.h TBNN_LIK_WEIBULL) for the tests: the oracle
(oracle/tbnn_oracle.py) has no such likelihood, so the data term and its derivative are stated here and everything else -- the forward
pass, the priors and their gradients, the reverse mode's layer loop, the leapfrog / Metropolis step, the hyper transition -- is the
oracle's.

Per (row, output), f the log of the scale, k the shape; the SIGN of the target is the censoring flag: y > 0 an event at time y (d = 1),
y < 0 a row right-censored at |y| (d = 0).  With t = |y| and u = (t e^-f)^k = exp(k (log t - f)):
    event     log p = log k + (k - 1) log t - k f - u
    censored  log S = -u
    dL/df     = k (u - d)
A row weight w_i scales the row's terms and deltas.

Two arms.  dtype=np.float64: the definition as written.  dtype=np.float32: the KERNEL's own formula, operation by operation in fp32
(csrc/common.hpp weibull_term, csrc/kernels_fast.hpp lik_delta): lt = log |y|, z = k (lt - f), u = exp(z), the term k f + u on an event and
u on a censored row, the delta k (u - 1) or k u, a weight multiplied onto either afterwards; the terms are summed in fp64, as the kernels'
accumulators sum them, the sign and the constant C = -sum w d (log k + (k - 1) log t) are fp64 (csrc/kernels_hmc.hpp data_logp,
k_pois_const), and the priors are the oracle's fp32 arm.  The network's own arithmetic (matrix products, activations) is the oracle's in
that dtype.

A spec here is the oracle's NetSpec with likelihood LIK_FIXED_GAUSSIAN and no last activation (no likelihood hyper: H = 4 layers): the
oracle's own hyper transition of such a spec is the layer priors alone, which is the Weibull hyper transition too."""
import functools
import math

import numpy as np

import tbnn_oracle as o
import student_ref as _sr

LIK_WEIBULL = 16


def make_spec(dims, act, prior):
    return o.make_spec(dims, act, prior, o.LIK_FIXED_GAUSSIAN, o.ACT_NONE)


def prior_log_prob(spec, theta, eta, dtype):
    """the layer priors of the oracle's target_log_prob, summed as it sums them"""
    dt = dtype
    theta, eta = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    prob = dt(0)
    for i, (l, (W, b)) in enumerate(zip(spec.layers, o.unflatten(spec, theta))):
        prob = dt(prob + o.layer_log_prob(l, eta[4 * i:4 * i + 4], W, b, dt))
    return prob


def _targets(f, Y, dtype):
    """Y [n, d_out] (or flat) as [d_out, n] in `dtype`"""
    return np.asarray(Y, dtype=dtype).reshape(f.shape[1], -1).T


def const_terms(Y, k):
    """d (log k + (k - 1) log t) per target, fp64 (the shape of Y): the part of the log density that does not depend on f -- events only"""
    y = np.asarray(Y, dtype=np.float64)
    k = float(k)
    return np.where(y > 0, math.log(k) + (k - 1.0) * np.log(np.abs(y)), 0.0)


def elementwise(f, Y, k, dtype):
    """(k d f + u, dL/df = k (u - d)), each [d_out, n] in `dtype`; f [d_out, n], Y [n, d_out] (or flat), signed"""
    dt = dtype
    f = np.asarray(f, dtype=dt)
    y = _targets(f, Y, dt)
    kk = dt(k)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        lt = np.log(np.abs(y)).astype(dt)
        z = (kk * (lt - f).astype(dt)).astype(dt)
        u = np.exp(z).astype(dt)
        ev = y > 0
        term = np.where(ev, ((kk * f).astype(dt) + u).astype(dt), u).astype(dt)
        delta = (kk * np.where(ev, (u - dt(1)).astype(dt), u).astype(dt)).astype(dt)
        return term, delta


def terms(f, Y, k):
    """the log density (event) or log survival function (censored) per (output, row), fp64 [d_out, n]"""
    f = np.asarray(f, dtype=np.float64)
    t, _d = elementwise(f, Y, k, np.float64)
    return const_terms(_targets(f, Y, np.float64), k) - t


def data_log_prob(spec, k, f, Y, dtype=np.float64, w=None):
    """(the data term as a float64, the statistic sum w (k d f + u) as the kernels accumulate it)"""
    t, _d = elementwise(f, Y, k, dtype)
    c = const_terms(_targets(np.asarray(f), Y, np.float64), k)          # [d_out, n]
    if w is not None:
        t = (np.asarray(w, dtype=dtype) * t).astype(dtype)       # (the kernel: wt * term in fp32, then the fp64 sum)
        c = np.asarray(w, dtype=np.float64) * c
    stat = float(np.sum(t.astype(np.float64)))
    return -stat + float(np.sum(c)), stat


def target_log_prob_and_grad(spec, k, theta, eta, X, Y, dtype=np.float64, w=None):
    """(log posterior as a float64, its gradient in `dtype`): the oracle's target_log_prob_and_grad with the Weibull data term"""
    dt = dtype
    theta, eta = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    parts = o.unflatten(spec, theta)
    f, acts = o.forward(spec, theta, X, dt, keep=True)
    logp = float(prior_log_prob(spec, theta, eta, dt)) + data_log_prob(spec, k, f, Y, dt, w)[0]
    _t, d_a = elementwise(f, Y, k, dt)
    if w is not None:
        d_a = (np.asarray(w, dtype=dt) * d_a).astype(dt)
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


def weight_step(spec, k, theta, eta, X, Y, eps, L, p0, log_u, dtype=np.float64, w=None):
    """one weight transition: the oracle's leapfrog and Metropolis step over this module's value and gradient (energies in fp64)"""
    vg = lambda q: target_log_prob_and_grad(spec, k, q, eta, X, Y, dtype, w)
    return o.hmc_step(vg, theta, eps, L, p0, log_u, dtype, np.float64)


def hyper_step(spec, eta, theta, X, Y, eps_h, L_h, p0, log_u, dtype=np.float64):
    """the hyper transition: no likelihood hyper and no data term -- the oracle's own for a fixed-sd spec"""
    assert spec.likelihood == o.LIK_FIXED_GAUSSIAN
    return o.hyper_step(spec, eta, theta, X, Y, eps_h, L_h, p0, log_u, dtype)


# ---- the cases of tests/test_gpu_weibull.py: student_ref.CASES' shapes, row counts, activations, priors, families and environments (the
# smallest with ragged last tiles that reach each kernel), the shapes spread over {0.5, 1, 1.5, 3}; one all-event and one all-censored
# dataset on the generic case's network ----
# The targets are drawn around the network's OWN untrained log-scales (problem_of), so that u = (t e^-f)^k is of order 1 at the state the
# tests evaluate: the data term is then a sum of n d_out terms of order 1, the event-only parts (k d f, the constant, the -d of the delta)
# are as large as the rest, and student_ref's leapfrog steps move the state by far more than the tolerances that judge it.  (Drawn around
# the teacher's log-scales 0.5 + 0.8 z instead, an untrained network of these widths is off by up to 12 units of f, u reaches 1e7 at
# k = 3, the log-posterior -5e8, and every relative band turns into an absolute one of hundreds: such cases got other data.)
_SHAPES = {"fast3": 0.5, "fast3_two_outputs": 3.0, "fast": 1.5, "mid1": 3.0, "mid10": 0.5, "tall": 1.0, "wide1": 0.5, "wide10": 1.0,
           "lay_last": 1.5, "lay_separate": 1.0, "lay_tail": 3.0, "generic": 3.0, "traj": 1.5}
CASES = {name: c[:6] + (_SHAPES[name], "mixed") for name, c in _sr.CASES.items()}      # dims, rows, act, prior, family, env, k, rows' kind
CASES["all_events"] = _sr.CASES["generic"][:6] + (1.5, "events")
CASES["all_censored"] = _sr.CASES["generic"][:6] + (3.0, "censored")


def problem_of(dims, n, act, prior, k, kind="mixed", seed=11):
    """(spec, X, Y, theta, eta): the oracle's synthetic rows and initial state; the event times are drawn from the model -- Weibull of
    shape k and scale exp(f0 + 0.3 z), f0 the network's own outputs at the initial state (fp64) and z the oracle's teacher's standardised
    outputs, a misfit the gradient can see -- and the censoring times from the same model times 1.5: the earlier of the two is the
    target, negative where the censoring time came first.  kind "events": every target the event time; "censored": every target minus
    the censoring time.  Times are kept inside fp32's normal range."""
    _g, X, Yr, theta, eta = o.synth_problem(dims, n, act, prior, o.LIK_GAUSSIAN)
    spec = make_spec(dims, act, prior)
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1)
    eta = np.asarray(eta[:spec.n_hypers], dtype=np.float32)          # no likelihood hyper
    rng = np.random.default_rng(seed)
    z = np.asarray(Yr, dtype=np.float64).reshape(n, -1)                                      # [n, d_out]
    f0 = o.forward(spec, np.asarray(theta, dtype=np.float64), X.astype(np.float64), np.float64).T                 # [n, d_out]
    lam = np.exp(f0 + 0.3 * z)
    T = np.clip(lam * rng.weibull(float(k), z.shape), 1e-30, 1e30)
    Cn = np.clip(1.5 * lam * rng.weibull(float(k), z.shape), 1e-30, 1e30)
    if kind == "events":
        Y = T
    elif kind == "censored":
        Y = -Cn
    else:
        Y = np.where(T <= Cn, T, -Cn)
    return spec, X, Y.astype(np.float32), theta, eta


@functools.lru_cache(maxsize=None)
def problem(name):
    """a case's problem, the shape included: computed once per process and left unchanged"""
    dims, n, act, prior, _fam, _env, k, kind = CASES[name]
    return problem_of(dims, n, act, prior, k, kind) + (k,)


@functools.lru_cache(maxsize=None)
def ref64(name):
    """the fp64 value and gradient of a case at its state: once per process"""
    spec, X, Y, theta, eta, k = problem(name)
    return target_log_prob_and_grad(spec, k, theta, eta, X, Y, np.float64)


def step_size(name):
    """the leapfrog step of a case's injected transition (4 steps; the trajectory case: 1 and 9): TEN times student_ref's, 3e-4 (traj:
    2e-3).  At student_ref's own step the fp64 reference's log accept ratio is 2e-7 .. 2e-3 over the cases, far inside the 2e-2 band
    that judges it; at ten times it is 6e-5 .. 14 (nine cases above 1e-2), the fp32 arm stays within 2.5e-3 of it, and the proposal
    moves some coordinate of theta by 4e-3 .. 6e-2 -- hundreds of times the 1e-5 / 2e-6 the state checks allow (MIN_MOVE)."""
    return 10.0 * _sr.step_size("generic" if name in ("all_events", "all_censored") else name)


# the least any case's injected transition must move some coordinate of theta (asserted where a state is compared, next to 50 x that
# check's own tolerance): 100 x the 1e-5 a state check allows at |theta|_inf <= 1
MIN_MOVE = 1e-3
