"""The cases of the Gamma likelihood's tests (include/tbnn.h TBNN_LIK_GAMMA) and thin wrappers over the oracle, which models the
likelihood (oracle/tbnn_oracle.py LIK_GAMMA: gamma_elementwise, gamma_const_terms, gamma_terms and the Gamma branches of its targets).

Per (row, output), f the log of the mean, a the shape, mu = exp(f):
    log p(y | f) = a log a - lgamma(a) + (a - 1) log y - a f - a y exp(-f)
    dL/df        = a (y exp(-f) - 1)
A row weight w_i scales the row's terms and deltas.  The two arms (np.float64: the definition; np.float32: the kernel's own formula,
operation by operation) are described at the oracle's gamma_elementwise and _data_term.

A spec here is the oracle's NetSpec with likelihood LIK_GAMMA, no last activation and lik_df = a (no likelihood hyper: H = 4 layers).  The
functions below keep the call shapes the Gamma modules were written with -- (spec, a, ...) -- assert that the spec carries that shape and
hand over to the oracle."""
import functools

import numpy as np

import tbnn_oracle as o
import student_ref as _sr

LIK_GAMMA = o.LIK_GAMMA
assert LIK_GAMMA == 14


def make_spec(dims, act, prior, a=0.0):
    """a: the shape (0: a spec for its layers alone, as the run-time jobs read it)"""
    return o.make_spec(dims, act, prior, o.LIK_GAMMA, o.ACT_NONE, lik_df=float(a))


def _checked(spec, a):
    assert spec.likelihood == o.LIK_GAMMA and spec.lik_df == a, (spec.likelihood, spec.lik_df, a)
    return spec


def prior_log_prob(spec, theta, eta, dtype):
    """the layer priors of the oracle's target_log_prob, summed as it sums them"""
    dt = dtype
    theta, eta = np.asarray(theta, dtype=dt), np.asarray(eta, dtype=dt)
    prob = dt(0)
    for i, (l, (W, b)) in enumerate(zip(spec.layers, o.unflatten(spec, theta))):
        prob = dt(prob + o.layer_log_prob(l, eta[4 * i:4 * i + 4], W, b, dt))
    return prob


const_terms = o.gamma_const_terms
elementwise = o.gamma_elementwise
terms = o.gamma_terms


def data_log_prob(spec, a, f, Y, dtype=np.float64, w=None):
    """(the data term as a float64, the statistic sum w (f + y e^-f) as the kernels accumulate it)"""
    lp, stat = o._data_term(_checked(spec, a), np.asarray(f, dtype=dtype), Y, dtype, w)
    return float(lp), stat


def target_log_prob_and_grad(spec, a, theta, eta, X, Y, dtype=np.float64, w=None):
    """(log posterior as a float64, its gradient in `dtype`)"""
    lp, g = o.target_log_prob_and_grad(_checked(spec, a), theta, eta, X, Y, dtype, w=w)
    return float(lp), g


def likelihood_value_and_grad(spec, a, theta, eta, X, Y, dtype=np.float64, w=None):
    """the data term alone and its gradient (tbnn_optimize's objective "likelihood")"""
    lp, g = o.likelihood_value_and_grad(_checked(spec, a), theta, eta, X, Y, dtype, w=w)
    return float(lp), g


def weight_step(spec, a, theta, eta, X, Y, eps, L, p0, log_u, dtype=np.float64, w=None):
    """one weight transition: the oracle's leapfrog and Metropolis step (energies in fp64)"""
    return o.weight_step(_checked(spec, a), theta, eta, X, Y, eps, L, p0, log_u, dtype, np.float64, w=w)


def hyper_step(spec, eta, theta, X, Y, eps_h, L_h, p0, log_u, dtype=np.float64):
    """the hyper transition: no likelihood hyper and no data term -- the layer priors alone"""
    assert spec.likelihood == o.LIK_GAMMA
    return o.hyper_step(spec, eta, theta, X, Y, eps_h, L_h, p0, log_u, dtype)


# ---- the cases of tests/test_gpu_gamma.py: student_ref.CASES' shapes, row counts, activations, priors, families and environments (the
# smallest with ragged last tiles that reach each kernel), the shapes spread over {0.5, 2, 10, 200} ----
_SHAPES = (0.5, 2.0, 10.0, 200.0)
CASES = {name: c[:6] + (_SHAPES[i % 4],) for i, (name, c) in enumerate(_sr.CASES.items())}      # dims, rows, act, prior, family, env, a


def problem_of(dims, n, act, prior, a, seed=11):
    """(spec, X, Y, theta, eta): the oracle's synthetic rows and initial state; the targets are drawn from the model -- Gamma of shape a
    and mean exp(0.5 + 0.8 z), z the oracle's teacher's standardised outputs -- and kept strictly positive in fp32"""
    _g, X, Yr, theta, eta = o.synth_problem(dims, n, act, prior, o.LIK_GAUSSIAN)
    spec = make_spec(dims, act, prior, a)
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
