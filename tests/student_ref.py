"""The reference of the Student-t likelihood (include/tbnn.h TBNN_LIK_STUDENT_T) for the tests: the oracle (oracle/tbnn_oracle.py) has no such
likelihood, so the data term and its derivative are stated here and everything else -- the forward pass, the priors and their gradients,
the reverse mode's layer loop, the leapfrog / Metropolis step, the hyper transition -- is the oracle's.

Per (row, output), r = y - f, s the scale (spec.fixed_sd, clipped to [1e-8, 1e8] as the Gaussian kinds clip theirs), nu the degrees of freedom:
    log p = lgamma((nu+1)/2) - lgamma(nu/2) - 1/2 log(nu pi) - log s - (nu+1)/2 log1p(r^2 / (nu s^2))
    dL/df = (nu+1) r / (nu s^2 + r^2)
A row weight w_i scales the row's terms and deltas, and the constant counts W = sum w_i rows.

Two arms.  dtype=np.float64: the definition as written, np.log1p and a division.  dtype=np.float32: the KERNEL's own formula, operation by
operation in fp32 (csrc/common.hpp log1p_fast, csrc/kernels_fast.hpp lik_delta): k = 1 / (nu s^2), u = r r k, the series
2 z (1 + z^2/3 + z^4/5 + z^6/7), z = u / (2 + u), below u = 1/4 and log(1 + u) from there on, the delta (nu + 1) (r k) / (1 + u); the terms
are summed in fp64, as the kernels' accumulators sum them, the constant is fp64, and the priors are the oracle's fp32 arm.  The network's
own arithmetic (matrix products, activations) is the oracle's in that dtype.

A spec here is the oracle's NetSpec with likelihood LIK_FIXED_GAUSSIAN (no likelihood hyper: H = 4 layers; fixed_sd = s): the oracle's own
hyper transition of such a spec is the layer priors alone, which is the Student-t hyper transition too."""
import math

import numpy as np

import tbnn_oracle as o

LIK_STUDENT_T = 8


def make_spec(dims, act, prior, s, final_act=o.ACT_NONE):
    spec = o.make_spec(dims, act, prior, o.LIK_FIXED_GAUSSIAN, final_act)
    spec.fixed_sd = float(s)
    return spec


def scale_of(spec):
    return min(max(float(np.float32(spec.fixed_sd)), 1e-8), 1e8)


def const(nu, s):
    """c(nu, s) of one (row, output) element, fp64"""
    nu = float(nu)
    return math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi) - math.log(float(s))


def log1p_kernel32(u):
    """csrc/common.hpp log1p_fast in fp32 NumPy: the series below 1/4, log(1 + u) from there on"""
    u = np.asarray(u, dtype=np.float32)
    one, two = np.float32(1), np.float32(2)
    with np.errstate(over="ignore", invalid="ignore"):
        z = u * (one / (two + u))
        z2 = z * z
        ser = (two * z) * (z2 * (z2 * (z2 * np.float32(1.0 / 7.0) + np.float32(0.2)) + np.float32(1.0 / 3.0)) + one)
        return np.where(u < np.float32(0.25), ser, np.log(one + u)).astype(np.float32)


def elementwise(f, Y, nu, s, dtype):
    """(log1p(r^2 / (nu s^2)), dL/df), each [d_out, n] in `dtype`; f [d_out, n], Y [n, d_out] (or flat)"""
    dt = dtype
    f = np.asarray(f, dtype=dt)
    y = np.asarray(Y, dtype=dt).reshape(f.shape[1], -1).T
    r = y - f
    if dt == np.float64:
        ns2 = float(nu) * float(s) ** 2
        return np.log1p(r * r / ns2), (float(nu) + 1.0) * r / (ns2 + r * r)
    nu32, s32 = np.float32(nu), np.float32(s)
    k = np.float32(1) / (nu32 * s32 * s32)
    u = r * r * k
    d = (nu32 + np.float32(1)) * (r * k) * (np.float32(1) / (np.float32(1) + u))
    return log1p_kernel32(u), d.astype(np.float32)


def terms(f, Y, nu, s):
    """the log density per (output, row), fp64 [d_out, n]"""
    t, _d = elementwise(f, Y, nu, s, np.float64)
    return const(nu, s) - 0.5 * (float(nu) + 1.0) * t


def data_log_prob(spec, nu, f, Y, dtype=np.float64, w=None):
    """(the data term as a float64, the statistic sum w log1p(.) as the kernels accumulate it)"""
    s = scale_of(spec)
    t, _d = elementwise(f, Y, nu, s, dtype)
    n, d_out = f.shape[1], f.shape[0]
    if w is not None:
        t = np.asarray(w, dtype=dtype) * t                    # (the kernel: wt * term in fp32, then the fp64 sum)
    stat = float(np.sum(t.astype(np.float64)))
    rows = float(n) if w is None else float(np.sum(np.asarray(w, dtype=np.float64)))
    return rows * d_out * const(nu, s) - 0.5 * (float(nu) + 1.0) * stat, stat


def prior_log_prob(spec, theta, eta, dtype):
    dt = dtype
    theta, eta = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    prob = dt(0)
    for i, (l, (W, b)) in enumerate(zip(spec.layers, o.unflatten(spec, theta))):
        prob = dt(prob + o.layer_log_prob(l, eta[4 * i:4 * i + 4], W, b, dt))
    return prob


def target_log_prob_and_grad(spec, nu, theta, eta, X, Y, dtype=np.float64, w=None):
    """(log posterior as a float64, its gradient in `dtype`): the oracle's target_log_prob_and_grad with the Student-t data term"""
    dt = dtype
    theta, eta = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    parts = o.unflatten(spec, theta)
    f, acts = o.forward(spec, theta, X, dt, keep=True)
    logp = float(prior_log_prob(spec, theta, eta, dt)) + data_log_prob(spec, nu, f, Y, dt, w)[0]
    _t, d_a = elementwise(f, Y, nu, scale_of(spec), dt)
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


def likelihood_value_and_grad(spec, nu, theta, eta, X, Y, dtype=np.float64, w=None):
    """the data term alone and its gradient (tbnn_optimize's objective "likelihood")"""
    dt = dtype
    lp, g = target_log_prob_and_grad(spec, nu, theta, eta, X, Y, dt, w)
    th, et = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    pg = [tuple(o.prior_grad(l, et[4 * i:4 * i + 4], W, b, dt)) for i, (l, (W, b)) in enumerate(zip(spec.layers, o.unflatten(spec, th)))]
    return lp - float(prior_log_prob(spec, th, et, dt)), (g - o.flatten(pg).astype(dt)).astype(dt)


def weight_step(spec, nu, theta, eta, X, Y, eps, L, p0, log_u, dtype=np.float64, w=None):
    """one weight transition: the oracle's leapfrog and Metropolis step over this module's value and gradient (energies in fp64)"""
    vg = lambda q: target_log_prob_and_grad(spec, nu, q, eta, X, Y, dtype, w)
    return o.hmc_step(vg, theta, eps, L, p0, log_u, dtype, np.float64)


def hyper_step(spec, eta, theta, X, Y, eps_h, L_h, p0, log_u, dtype=np.float64):
    """the hyper transition: no likelihood hyper and no data term -- the oracle's own for a fixed-sd spec"""
    assert spec.likelihood == o.LIK_FIXED_GAUSSIAN
    return o.hyper_step(spec, eta, theta, X, Y, eps_h, L_h, p0, log_u, dtype)


# ---- the cases of tests/test_gpu_student.py (tests/test_student_host.py judges the fp32 arm on the same problems) ----
CASES = {
    # dims, rows, hidden activation, prior, family, environment, nu, s
    "fast3": ([5, 50, 50, 50, 1], 3001, o.ACT_RELU, o.PRIOR_CAUCHY, "fast3", {}, 1e4, 0.1),                     # ragged last tile
    "fast3_two_outputs": ([7, 17, 33, 2], 777, o.ACT_TANH, o.PRIOR_GAUSSIAN, "fast3", {}, 2.5, 1.0),
    "fast": ([4, 30, 30, 1], 2500, o.ACT_TANH, o.PRIOR_GAUSSIAN, "fast", {}, 1.0, 0.1),                         # TBNN_JIT_SKIP=fast3
    "mid1": ([20, 64, 64, 1], 2000, o.ACT_SIGMOID, o.PRIOR_CAUCHY, "mid", {}, 30.0, 1.0),                       # VALU last layer
    "mid10": ([30, 80, 80, 10], 3001, o.ACT_ELU, o.PRIOR_CAUCHY, "mid", {}, 2.5, 0.1),                          # MFMA output tile
    "tall": ([784, 20, 20, 1], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "tall", {}, 1.0, 1.0),
    "wide1": ([10, 200, 200, 1], 3001, o.ACT_RELU, o.PRIOR_CAUCHY, "wide", {}, 30.0, 0.1),
    "wide10": ([10, 200, 200, 10], 1000, o.ACT_ELU, o.PRIOR_GAUSSIAN, "wide", {}, 1e4, 1.0),
    # the layered family (no run-time instantiation, no tall registry): which likelihood kernel runs follows from lay_plan_shape
    "lay_last": ([784, 100, 100, 10], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "layered", {}, 2.5, 1.0),                          # k_lay_last
    "lay_separate": ([784, 100, 100, 10], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "layered", {"TBNN_LAY_LAST": "0"}, 30.0, 0.1),  # k_lay_lik
    "lay_tail": ([784, 20, 20, 10], 1205, o.ACT_TANH, o.PRIOR_GAUSSIAN, "layered", {}, 1e4, 0.1),                          # k_lay_tail
    "generic": ([5, 16, 16, 4], 517, o.ACT_TANH, o.PRIOR_CAUCHY, "generic", {}, 1.0, 1.0),
    "traj": ([1, 10, 10, 1], 500, o.ACT_RELU, o.PRIOR_CAUCHY, "traj", {}, 2.5, 0.1),                            # the trajectory kernel
}


def problem_of(dims, n, act, prior, nu, s, outliers=0.05, seed=11):
    """(spec, X, Y, theta, eta): the oracle's synthetic rows and initial state; the targets are its teacher's (standardised) outputs plus
    N(0, s^2), with `outliers` of the rows moved by 20 s .. 50 s either way: r^2 << nu s^2 and r^2 >> nu s^2 both occur in every tile"""
    _g, X, Yr, theta, eta = o.synth_problem(dims, n, act, prior, o.LIK_GAUSSIAN)
    spec = make_spec(dims, act, prior, s)
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1)
    eta = np.asarray(eta[:spec.n_hypers], dtype=np.float32)          # no likelihood hyper
    rng = np.random.default_rng(seed)
    f = np.asarray(Yr, dtype=np.float64).reshape(n, -1)                                      # [n, d_out]
    Y = f + s * rng.standard_normal(f.shape)
    bad = rng.random(n) < outliers
    Y[bad] += s * rng.uniform(20.0, 50.0, (int(bad.sum()), f.shape[1])) * rng.choice([-1.0, 1.0], (int(bad.sum()), f.shape[1]))
    return spec, X, Y.astype(np.float32), theta, eta


_PROBLEMS = {}


def problem(name):
    """a case's problem, nu included: computed once per process and left unchanged"""
    if name not in _PROBLEMS:
        dims, n, act, prior, _fam, _env, nu, s = CASES[name]
        _PROBLEMS[name] = problem_of(dims, n, act, prior, nu, s) + (nu,)
    return _PROBLEMS[name]


_REF64 = {}


def ref64(name):
    """the fp64 value and gradient of a case at its state: once per process"""
    if name not in _REF64:
        spec, X, Y, theta, eta, nu = problem(name)
        _REF64[name] = target_log_prob_and_grad(spec, nu, theta, eta, X, Y, np.float64)
    return _REF64[name]


def step_size(name):
    """the leapfrog step of a case's injected transition (4 steps; the trajectory case: 1 and 9)"""
    return 2e-4 if name == "traj" else 3e-5
