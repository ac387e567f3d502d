"""The reference of the Gamma likelihood (include/tbnn.h TBNN_LIK_GAMMA) for the tests: the oracle (oracle/tbnn_oracle.py) has no such
likelihood, so the data term and its derivative are stated here and everything else -- the forward pass, the priors and their gradients,
the reverse mode's layer loop, the leapfrog / Metropolis step, the hyper transition -- is the oracle's.

Per (row, output), f the log of the mean, a the shape, mu = exp(f):
    log p(y | f) = a log a - lgamma(a) + (a - 1) log y - a f - a y exp(-f)
    dL/df        = a (y exp(-f) - 1)
A row weight w_i scales the row's terms and deltas.

Two arms.  dtype=np.float64: the definition as written.  dtype=np.float32: the KERNEL's own formula, operation by operation in fp32
(csrc/common.hpp gamma_term, csrc/kernels_fast.hpp lik_delta): e = exp(-f), ye = y e, the term f + ye, the delta a (ye - 1), a weight
multiplied onto either afterwards; the terms are summed in fp64, as the kernels' accumulators sum them, the factor -a and the constant
C = sum w (lgamma(a) - a log a - (a - 1) log y) are fp64 (csrc/kernels_hmc.hpp data_logp, k_pois_const), and the priors are the oracle's
fp32 arm.  The network's own arithmetic (matrix products, activations) is the oracle's in that dtype.

A spec here is the oracle's NetSpec with likelihood LIK_FIXED_GAUSSIAN and no last activation (no likelihood hyper: H = 4 layers): the
oracle's own hyper transition of such a spec is the layer priors alone, which is the Gamma hyper transition too."""
import functools
import math

import numpy as np

import tbnn_oracle as o
import student_ref as _sr

LIK_GAMMA = 14


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


def const_terms(Y, a):
    """a log a - lgamma(a) + (a - 1) log y per target, fp64 (the shape of Y): the part of the log density that does not depend on f"""
    y = np.asarray(Y, dtype=np.float64)
    a = float(a)
    return (a * math.log(a) - math.lgamma(a)) + (a - 1.0) * np.log(y)


def elementwise(f, Y, a, dtype):
    """(f + y e^-f, dL/df = a (y e^-f - 1)), each [d_out, n] in `dtype`; f [d_out, n], Y [n, d_out] (or flat)"""
    dt = dtype
    f = np.asarray(f, dtype=dt)
    y = np.asarray(Y, dtype=dt).reshape(f.shape[1], -1).T
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-f).astype(dt)
        ye = (y * e).astype(dt)
        return (f + ye).astype(dt), (dt(a) * (ye - dt(1))).astype(dt)


def terms(f, Y, a):
    """the log density per (output, row), fp64 [d_out, n]"""
    f = np.asarray(f, dtype=np.float64)
    t, _d = elementwise(f, Y, a, np.float64)
    return const_terms(np.asarray(Y, dtype=np.float64).reshape(f.shape[1], -1).T, a) - float(a) * t


def data_log_prob(spec, a, f, Y, dtype=np.float64, w=None):
    """(the data term as a float64, the statistic sum w (f + y e^-f) as the kernels accumulate it)"""
    t, _d = elementwise(f, Y, a, dtype)
    c = const_terms(np.asarray(Y, dtype=np.float64).reshape(f.shape[1], -1).T, a)          # [d_out, n]
    if w is not None:
        t = (np.asarray(w, dtype=dtype) * t).astype(dtype)       # (the kernel: wt * term in fp32, then the fp64 sum)
        c = np.asarray(w, dtype=np.float64) * c
    stat = float(np.sum(t.astype(np.float64)))
    return -float(a) * stat + float(np.sum(c)), stat


def target_log_prob_and_grad(spec, a, theta, eta, X, Y, dtype=np.float64, w=None):
    """(log posterior as a float64, its gradient in `dtype`): the oracle's target_log_prob_and_grad with the Gamma data term"""
    dt = dtype
    theta, eta = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    parts = o.unflatten(spec, theta)
    f, acts = o.forward(spec, theta, X, dt, keep=True)
    logp = float(prior_log_prob(spec, theta, eta, dt)) + data_log_prob(spec, a, f, Y, dt, w)[0]
    _t, d_a = elementwise(f, Y, a, dt)
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


def likelihood_value_and_grad(spec, a, theta, eta, X, Y, dtype=np.float64, w=None):
    """the data term alone and its gradient (tbnn_optimize's objective "likelihood")"""
    dt = dtype
    lp, g = target_log_prob_and_grad(spec, a, theta, eta, X, Y, dt, w)
    th, et = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    pg = [tuple(o.prior_grad(l, et[4 * i:4 * i + 4], W, b, dt)) for i, (l, (W, b)) in enumerate(zip(spec.layers, o.unflatten(spec, th)))]
    return lp - float(prior_log_prob(spec, th, et, dt)), (g - o.flatten(pg).astype(dt)).astype(dt)


def weight_step(spec, a, theta, eta, X, Y, eps, L, p0, log_u, dtype=np.float64, w=None):
    """one weight transition: the oracle's leapfrog and Metropolis step over this module's value and gradient (energies in fp64)"""
    vg = lambda q: target_log_prob_and_grad(spec, a, q, eta, X, Y, dtype, w)
    return o.hmc_step(vg, theta, eps, L, p0, log_u, dtype, np.float64)


def hyper_step(spec, eta, theta, X, Y, eps_h, L_h, p0, log_u, dtype=np.float64):
    """the hyper transition: no likelihood hyper and no data term -- the oracle's own for a fixed-sd spec"""
    assert spec.likelihood == o.LIK_FIXED_GAUSSIAN
    return o.hyper_step(spec, eta, theta, X, Y, eps_h, L_h, p0, log_u, dtype)


# ---- the cases of tests/test_gpu_gamma.py: student_ref.CASES' shapes, row counts, activations, priors, families and environments (the
# smallest with ragged last tiles that reach each kernel), the shapes spread over {0.5, 2, 10, 200} ----
_SHAPES = (0.5, 2.0, 10.0, 200.0)
CASES = {name: c[:6] + (_SHAPES[i % 4],) for i, (name, c) in enumerate(_sr.CASES.items())}      # dims, rows, act, prior, family, env, a


def problem_of(dims, n, act, prior, a, seed=11):
    """(spec, X, Y, theta, eta): the oracle's synthetic rows and initial state; the targets are drawn from the model -- Gamma of shape a
    and mean exp(0.5 + 0.8 z), z the oracle's teacher's standardised outputs -- and kept strictly positive in fp32"""
    _g, X, Yr, theta, eta = o.synth_problem(dims, n, act, prior, o.LIK_GAUSSIAN)
    spec = make_spec(dims, act, prior)
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1)
    eta = np.asarray(eta[:spec.n_hypers], dtype=np.float32)          # no likelihood hyper
    rng = np.random.default_rng(seed)
    z = np.asarray(Yr, dtype=np.float64).reshape(n, -1)                                      # [n, d_out]
    mu = np.exp(0.5 + 0.8 * z)
    Y = np.maximum(rng.gamma(float(a), mu / float(a)), 1e-30)      # (a = 0.5 puts mass next to 0: no target rounds to 0 in fp32)
    return spec, X, Y.astype(np.float32), theta, eta


@functools.lru_cache(maxsize=None)
def problem(name):
    """a case's problem, the shape included: computed once per process and left unchanged"""
    dims, n, act, prior, _fam, _env, a = CASES[name]
    return problem_of(dims, n, act, prior, a) + (a,)


@functools.lru_cache(maxsize=None)
def ref64(name):
    """the fp64 value and gradient of a case at its state: once per process"""
    spec, X, Y, theta, eta, a = problem(name)
    return target_log_prob_and_grad(spec, a, theta, eta, X, Y, np.float64)


step_size = _sr.step_size
