"""What the optimiser tests share: a NumPy restatement of tbnn_optimize (include/tbnn.h) over the oracle's value and gradient, in a dtype
of choice, and the problems the CPU and GPU modules both use.

One step, as torch.optim.Adam(lr, betas, eps, amsgrad=..., maximize=True) defines it:
    m = b1 m + (1 - b1) g ; v = b2 v + (1 - b2) g^2 ; vhat = amsgrad ? max(vhat, v) : v
    theta += a_t m / (sqrt(vhat) r_t + eps),   a_t = lr / (1 - b1^t),   r_t = 1 / sqrt(1 - b2^t)
The C ABI carries lr, the betas and epsilon as fp32: F32 rounds a hyper-parameter the way the library receives it, and every GPU test
hands the restatement those values."""
import math

import numpy as np

import tbnn_oracle as o


def F32(x):
    return float(np.float32(x))


LR, B1, B2, EPS = F32(1e-3), F32(0.9), F32(0.999), F32(1e-8)


def adam_step(theta, g, m, v, vhat, t, lr, b1=B1, b2=B2, eps=EPS, amsgrad=True, dtype=np.float64):
    """one step (t counts from 1) in `dtype`: (theta, m, v, vhat) after it"""
    dt = dtype
    theta, g, m, v, vhat = (np.asarray(a, dtype=dt) for a in (theta, g, m, v, vhat))
    m = dt(b1) * m + dt(1.0 - b1) * g
    v = dt(b2) * v + dt(1.0 - b2) * (g * g)
    vhat = np.maximum(vhat, v) if amsgrad else v
    a_t = dt(lr / (1.0 - b1 ** t))
    r_t = dt(1.0 / math.sqrt(1.0 - b2 ** t))
    theta = theta + a_t * m / (np.sqrt(vhat) * r_t + dt(eps))
    return theta.astype(dt), m.astype(dt), v.astype(dt), vhat.astype(dt)


def value_and_grad(spec, theta, eta, X, Y, dtype=np.float64, w=None, objective="posterior"):
    if objective == "likelihood":
        return o.likelihood_value_and_grad(spec, theta, eta, X, Y, dtype, w)
    return o.target_log_prob_and_grad(spec, theta, eta, X, Y, dtype, w=w)


def run(spec, theta0, eta, X, Y, steps, lr=LR, b1=B1, b2=B2, eps=EPS, amsgrad=True, check_every=1, dtype=np.float64, w=None,
        objective="posterior"):
    """tbnn_optimize from a fresh optimiser state: (trace of the checked objectives as float64, theta after `steps` steps, the gradients
    of the steps)"""
    dt = dtype
    theta = np.asarray(theta0, dtype=dt)
    m = v = vhat = np.zeros_like(theta)
    trace, grads = [], []
    for i in range(steps):
        lp, g = value_and_grad(spec, theta, eta, X, Y, dt, w, objective)
        if i % check_every == 0:
            trace.append(float(lp))
        grads.append(g)
        theta, m, v, vhat = adam_step(theta, g, m, v, vhat, i + 1, lr, b1, b2, eps, amsgrad, dt)
    trace.append(float(value_and_grad(spec, theta, eta, X, Y, dt, w, objective)[0]))
    return np.asarray(trace, dtype=np.float64), theta, grads


# ---- the free-run cases (tests/test_gpu_optimize.py runs them on the device; tests/test_optimize_host.py judges the yardstick on them) ----
# dims, rows, prior: tanh hidden layers, Gaussian likelihood; the shapes are those of tests/jit_shapes.json
FREE_RUN = {
    "fast3": ([6, 24, 24, 1], 1501, o.PRIOR_GAUSSIAN),            # P = 793, not a multiple of 4: pitch padding
    "fast3_deep": ([5, 49, 49, 49, 1], 3001, o.PRIOR_CAUCHY),
    "mid": ([20, 100, 48, 2], 1000, o.PRIOR_CAUCHY),
    "tall": ([100, 64, 32, 1], 1205, o.PRIOR_CAUCHY),             # P = 8577 >= UPD_BIG_P: the big block geometry
    "wide": ([10, 200, 256, 1], 700, o.PRIOR_CAUCHY),             # one dense slab
}
FREE_STEPS = 30


def problem(dims, n, prior, act=o.ACT_TANH, likelihood=o.LIK_GAUSSIAN):
    spec, X, Y, theta, eta = o.synth_problem(dims, n, act, prior, likelihood)
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1)
    return spec, X, Y, theta, np.asarray(eta[:spec.n_hypers], dtype=np.float32)


_FREE = {}


def free_run(name):
    """(problem, fp64 run, fp32 run) of a free-run case: computed once per process and left unchanged"""
    if name not in _FREE:
        dims, n, prior = FREE_RUN[name]
        pb = problem(dims, n, prior)
        spec, X, Y, theta, eta = pb
        r64 = run(spec, theta, eta, X, Y, FREE_STEPS, dtype=np.float64)[:2]
        r32 = run(spec, theta, eta, X, Y, FREE_STEPS, dtype=np.float32)[:2]
        _FREE[name] = (pb, r64, r32)
    return _FREE[name]


def free_gaps(tr, th, tr64, th64, lr=LR):
    """(largest trace error relative to max(|value|, 1), largest theta error in units of lr)"""
    tr, tr64 = np.asarray(tr, np.float64), np.asarray(tr64, np.float64)
    return (float(np.max(np.abs(tr - tr64) / np.maximum(np.abs(tr64), 1.0))),
            float(np.max(np.abs(np.asarray(th, np.float64) - np.asarray(th64, np.float64))) / lr))
