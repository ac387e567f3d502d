"""The reference of the negative-binomial likelihood (include/tbnn.h TBNN_LIK_NEG_BINOMIAL) for the tests: the oracle (oracle/tbnn_oracle.py)
has no such likelihood, so the data term and its derivative are stated here and everything else -- the forward pass, the priors and their
gradients, the reverse mode's layer loop, the leapfrog / Metropolis step, the hyper transition -- is the oracle's, as in tests/student_ref.py.

Per (row, output), f the log of the mean, r the dispersion, mu = exp(f), p = mu / (r + mu), q = r / (r + mu):
    log p(y | f) = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y log p + r log q
    dL/df        = y q - r p = r (y - mu) / (r + mu)
A row weight w_i scales the row's terms and deltas.

Two arms.  dtype=np.float64: the definition as written -- log p = f - log(r + mu), log q = log r - log(r + mu) through np.logaddexp, the
delta as r (y - mu) / (r + mu).  dtype=np.float32: the KERNEL's own formula, operation by operation in fp32 (csrc/common.hpp negbin_term):
t = f - log r, a = |t|, e = exp(-a), l = log1p_fast(e) (the series below 1/4, log(1 + e) from there on), -log p = max(-t, 0) + l,
-log q = max(t, 0) + l, p and q from e and one reciprocal of 1 + e by the sign of t, the term -(y (-log p) + r (-log q)), the delta
y q - r p; the terms are summed in fp64, as the kernels' accumulators sum them, the constant is fp64, and the priors are the oracle's fp32
arm.  The network's own arithmetic (matrix products, activations) is the oracle's in that dtype.

A spec here is the oracle's NetSpec with likelihood LIK_FIXED_GAUSSIAN and no last activation (no likelihood hyper: H = 4 layers): the
oracle's own hyper transition of such a spec is the layer priors alone, which is the negative-binomial hyper transition too."""
import math

import numpy as np

import tbnn_oracle as o
from student_ref import log1p_kernel32, prior_log_prob          # (csrc/common.hpp log1p_fast in fp32 NumPy; the oracle's layer priors)
import student_ref as _sr

LIK_NEG_BINOMIAL = 10

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def make_spec(dims, act, prior):
    return o.make_spec(dims, act, prior, o.LIK_FIXED_GAUSSIAN, o.ACT_NONE)


def const_terms(Y, r):
    """lgamma(y + r) - lgamma(r) - lgamma(y + 1) per target, fp64 (the shape of Y)"""
    y = np.asarray(Y, dtype=np.float64)
    return _lgamma(y + float(r)) - math.lgamma(float(r)) - _lgamma(y + 1.0)


def elementwise(f, Y, r, dtype):
    """(y log p + r log q, dL/df), each [d_out, n] in `dtype`; f [d_out, n], Y [n, d_out] (or flat)"""
    dt = dtype
    f = np.asarray(f, dtype=dt)
    y = np.asarray(Y, dtype=dt).reshape(f.shape[1], -1).T
    if dt == np.float64:
        r = float(r)
        lr = math.log(r)
        lden = np.logaddexp(f, lr)                               # log(r + mu)
        with np.errstate(over="ignore"):
            mu = np.exp(f)
            d = np.where(np.isfinite(mu), r * (y - mu) / (r + mu), -r)
        return y * (f - lden) + r * (lr - lden), d
    one = np.float32(1)
    r32 = np.float32(r)
    lr = np.log(r32)                                             # (fp32: the kernels' logf of the prologue)
    t = f - lr
    a = np.abs(t)
    e = np.exp(-a).astype(np.float32)
    l = log1p_kernel32(e)
    nlp = np.maximum(-t, np.float32(0)) + l
    nlq = np.maximum(t, np.float32(0)) + l
    rc = one / (one + e)
    s = e * rc
    pos = t >= 0
    p, q = np.where(pos, rc, s), np.where(pos, s, rc)
    return (-(y * nlp + r32 * nlq)).astype(np.float32), (y * q - r32 * p).astype(np.float32)


def terms(f, Y, r):
    """the log density per (output, row), fp64 [d_out, n]"""
    f = np.asarray(f, dtype=np.float64)
    t, _d = elementwise(f, Y, r, np.float64)
    return t + const_terms(np.asarray(Y, dtype=np.float64).reshape(f.shape[1], -1).T, r)


def data_log_prob(spec, r, f, Y, dtype=np.float64, w=None):
    """(the data term as a float64, the statistic sum w (y log p + r log q) as the kernels accumulate it)"""
    t, _d = elementwise(f, Y, r, dtype)
    c = const_terms(np.asarray(Y, dtype=np.float64).reshape(f.shape[1], -1).T, r)          # [d_out, n]
    if w is not None:
        t = np.asarray(w, dtype=dtype) * t                    # (the kernel: wt * term in fp32, then the fp64 sum)
        c = np.asarray(w, dtype=np.float64) * c
    stat = float(np.sum(t.astype(np.float64)))
    return stat + float(np.sum(c)), stat


def target_log_prob_and_grad(spec, r, theta, eta, X, Y, dtype=np.float64, w=None):
    """(log posterior as a float64, its gradient in `dtype`): the oracle's target_log_prob_and_grad with the negative-binomial data term"""
    dt = dtype
    theta, eta = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    parts = o.unflatten(spec, theta)
    f, acts = o.forward(spec, theta, X, dt, keep=True)
    logp = float(prior_log_prob(spec, theta, eta, dt)) + data_log_prob(spec, r, f, Y, dt, w)[0]
    _t, d_a = elementwise(f, Y, r, dt)
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


def likelihood_value_and_grad(spec, r, theta, eta, X, Y, dtype=np.float64, w=None):
    """the data term alone and its gradient (tbnn_optimize's objective "likelihood")"""
    dt = dtype
    lp, g = target_log_prob_and_grad(spec, r, theta, eta, X, Y, dt, w)
    th, et = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    pg = [tuple(o.prior_grad(l, et[4 * i:4 * i + 4], W, b, dt)) for i, (l, (W, b)) in enumerate(zip(spec.layers, o.unflatten(spec, th)))]
    return lp - float(prior_log_prob(spec, th, et, dt)), (g - o.flatten(pg).astype(dt)).astype(dt)


def weight_step(spec, r, theta, eta, X, Y, eps, L, p0, log_u, dtype=np.float64, w=None):
    """one weight transition: the oracle's leapfrog and Metropolis step over this module's value and gradient (energies in fp64)"""
    vg = lambda q: target_log_prob_and_grad(spec, r, q, eta, X, Y, dtype, w)
    return o.hmc_step(vg, theta, eps, L, p0, log_u, dtype, np.float64)


def hyper_step(spec, eta, theta, X, Y, eps_h, L_h, p0, log_u, dtype=np.float64):
    """the hyper transition: no likelihood hyper and no data term -- the oracle's own for a fixed-sd spec"""
    assert spec.likelihood == o.LIK_FIXED_GAUSSIAN
    return o.hyper_step(spec, eta, theta, X, Y, eps_h, L_h, p0, log_u, dtype)


# ---- the cases of tests/test_gpu_negbin.py: student_ref.CASES' shapes, row counts, activations, priors, families and environments (the
# smallest with ragged last tiles that reach each kernel), the dispersions spread over {0.5, 2.5, 30, 1e4} ----
_DISPERSIONS = (0.5, 2.5, 30.0, 1e4)
CASES = {name: c[:6] + (_DISPERSIONS[i % 4],) for i, (name, c) in enumerate(_sr.CASES.items())}      # dims, rows, act, prior, family, env, r


def problem_of(dims, n, act, prior, r, seed=11):
    """(spec, X, Y, theta, eta): the oracle's synthetic rows and initial state; the targets are drawn from the model -- a gamma-Poisson
    mixture of dispersion r -- around log-rates 1.5 + 1.2 z, z the oracle's teacher's standardised outputs: rates from well below 1 to a
    few hundred, so zeros, small counts and counts far above r occur in every problem"""
    _g, X, Yr, theta, eta = o.synth_problem(dims, n, act, prior, o.LIK_GAUSSIAN)
    spec = make_spec(dims, act, prior)
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1)
    eta = np.asarray(eta[:spec.n_hypers], dtype=np.float32)          # no likelihood hyper
    rng = np.random.default_rng(seed)
    z = np.asarray(Yr, dtype=np.float64).reshape(n, -1)                                      # [n, d_out]
    mu = np.exp(1.5 + 1.2 * z)
    Y = rng.poisson(rng.gamma(float(r), mu / float(r)))
    return spec, X, Y.astype(np.float32), theta, eta


_PROBLEMS = {}


def problem(name):
    """a case's problem, r included: computed once per process and left unchanged"""
    if name not in _PROBLEMS:
        dims, n, act, prior, _fam, _env, r = CASES[name]
        _PROBLEMS[name] = problem_of(dims, n, act, prior, r) + (r,)
    return _PROBLEMS[name]


_REF64 = {}


def ref64(name):
    """the fp64 value and gradient of a case at its state: once per process"""
    if name not in _REF64:
        spec, X, Y, theta, eta, r = problem(name)
        _REF64[name] = target_log_prob_and_grad(spec, r, theta, eta, X, Y, np.float64)
    return _REF64[name]


def step_size(name):
    """the leapfrog step of a case's injected transition (4 steps; the trajectory case: 1 and 9)"""
    return _sr.step_size(name)
