"""The cases of the Student-t likelihood tests (include/tbnn.h TBNN_LIK_STUDENT_T; tests/test_gpu_student.py on the device,
tests/test_student_host.py for the fp32 arm on the same problems) and what the negative-binomial and heteroscedastic case tables
(tests/negbin_ref.py, tests/hetero_ref.py) share with them: the cache of a table's problems and fp64 references, and the step size.

No formula is stated here.  The likelihood itself -- its element functions in both arms, the data term, the reverse pass, the leapfrog and
the hyper transition -- is the oracle's (oracle/tbnn_oracle.py LIK_STUDENT_T, student_elementwise): a problem's spec carries the real
likelihood code, the scale as fixed_sd and the degrees of freedom as lik_df."""
import functools

import numpy as np

import tbnn_oracle as o

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
    spec = o.make_spec(dims, act, prior, o.LIK_STUDENT_T, o.ACT_NONE, fixed_sd=float(s), lik_df=float(nu))
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1)
    eta = np.asarray(eta[:spec.n_hypers], dtype=np.float32)          # no likelihood hyper
    rng = np.random.default_rng(seed)
    f = np.asarray(Yr, dtype=np.float64).reshape(n, -1)                                      # [n, d_out]
    Y = f + s * rng.standard_normal(f.shape)
    bad = rng.random(n) < outliers
    Y[bad] += s * rng.uniform(20.0, 50.0, (int(bad.sum()), f.shape[1])) * rng.choice([-1.0, 1.0], (int(bad.sum()), f.shape[1]))
    return spec, X, Y.astype(np.float32), theta, eta


def cached_cases(cases, problem_of):
    """(problem, ref64) of a case table whose entries are problem_of's first four arguments, the kernel family, the environment and
    problem_of's remaining arguments: problem(name) is the case's (spec, X, Y, theta, eta), ref64(name) the oracle's fp64 value and
    gradient at that state -- each computed once per process and left unchanged"""
    @functools.lru_cache(maxsize=None)
    def problem(name):
        c = cases[name]
        return problem_of(*c[:4], *c[6:])

    @functools.lru_cache(maxsize=None)
    def ref64(name):
        spec, X, Y, theta, eta = problem(name)
        return o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)

    return problem, ref64


problem, ref64 = cached_cases(CASES, problem_of)


def step_size(name):
    """the leapfrog step of a case's injected transition (4 steps; the trajectory case: 1 and 9)"""
    return 2e-4 if name == "traj" else 3e-5
