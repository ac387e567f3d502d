"""The cases of the negative-binomial likelihood tests (include/tbnn.h TBNN_LIK_NEG_BINOMIAL; tests/test_gpu_negbin.py on the device,
tests/test_negbin_host.py for the fp32 arm on the same problems).  No formula is stated here: the likelihood is the oracle's
(oracle/tbnn_oracle.py LIK_NEG_BINOMIAL, negbin_elementwise), and a problem's spec carries the real likelihood code and the dispersion as
lik_df."""
import numpy as np

import tbnn_oracle as o
import student_ref as _sr

# ---- the cases of tests/test_gpu_negbin.py: student_ref.CASES' shapes, row counts, activations, priors, families and environments (the
# smallest with ragged last tiles that reach each kernel), the dispersions spread over {0.5, 2.5, 30, 1e4} ----
_DISPERSIONS = (0.5, 2.5, 30.0, 1e4)
CASES = {name: c[:6] + (_DISPERSIONS[i % 4],) for i, (name, c) in enumerate(_sr.CASES.items())}      # dims, rows, act, prior, family, env, r


def problem_of(dims, n, act, prior, r, seed=11):
    """(spec, X, Y, theta, eta): the oracle's synthetic rows and initial state; the targets are drawn from the model -- a gamma-Poisson
    mixture of dispersion r -- around log-rates 1.5 + 1.2 z, z the oracle's teacher's standardised outputs: rates from well below 1 to a
    few hundred, so zeros, small counts and counts far above r occur in every problem"""
    _g, X, Yr, theta, eta = o.synth_problem(dims, n, act, prior, o.LIK_GAUSSIAN)
    spec = o.make_spec(dims, act, prior, o.LIK_NEG_BINOMIAL, o.ACT_NONE, lik_df=float(r))
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1)
    eta = np.asarray(eta[:spec.n_hypers], dtype=np.float32)          # no likelihood hyper
    rng = np.random.default_rng(seed)
    z = np.asarray(Yr, dtype=np.float64).reshape(n, -1)                                      # [n, d_out]
    mu = np.exp(1.5 + 1.2 * z)
    Y = rng.poisson(rng.gamma(float(r), mu / float(r)))
    return spec, X, Y.astype(np.float32), theta, eta


problem, ref64 = _sr.cached_cases(CASES, problem_of)
step_size = _sr.step_size
