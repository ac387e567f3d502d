"""The cases of the heteroscedastic Gaussian likelihood tests (include/tbnn.h TBNN_LIK_HETERO_GAUSSIAN; tests/test_gpu_hetero.py on the
device, tests/test_hetero_host.py for the fp32 arm on the same problems).  No formula is stated here: the likelihood is the oracle's
(oracle/tbnn_oracle.py LIK_HETERO_GAUSSIAN, hetero_pair), and a problem's spec carries the real likelihood code.  The network has exactly 2
outputs and no last activation: output 0 the mean f, output 1 the log-sd g; targets are one per row."""
import numpy as np

import tbnn_oracle as o
import student_ref as _sr


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
    assert dims[-1] == 2
    spec = o.make_spec(dims, act, prior, o.LIK_HETERO_GAUSSIAN, o.ACT_NONE)
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
    sg = np.exp(np.clip(f0[1], -o.LOG_CLIP, o.LOG_CLIP))
    sign = rng.choice([-1.0, 1.0], n)
    idx = np.arange(n)
    near, far = idx % 16 == 0, idx % 16 == 1
    Y[near] = f0[0][near] + 0.03 * sg[near] * sign[near]
    Y[far] = f0[0][far] + 10.0 * sg[far] * sign[far]
    return spec, X, Y.astype(np.float32), theta, eta


problem, ref64 = _sr.cached_cases(CASES, problem_of)
step_size = _sr.step_size
