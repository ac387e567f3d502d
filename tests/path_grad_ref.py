"""Integrated-gradients attributions against fp64: the problems, the reference and the band of tests/test_gpu_path_grad.py.  No test
functions here.
  reference  attributions(): the path points are formed in fp32 exactly as include/tbnn.h defines them -- d = x - x0, a_s = s / (P - 1),
             x_s = fmaf(a_s, d, x0), the fmaf emulated by the fp64 product and sum rounded once to fp32, the last point x itself --,
             input_grad_ref.jacobian runs at those n P points, and the trapezoid sum and the product with the fp32 d are taken in fp64.
  band       tol = |d_k| sum_s q_s (gamma(spec) + (P + 4) 2^-24) (A_s + |J_s|): input_grad_ref's own band per path point (FACTOR = 64,
             unchanged) plus one (P + 4) u for the P-term quadrature sum, its weights and the product with d.  Derived, not measured.
  kinks      a data row is flagged when any of its path points is flagged under any network; flagged rows are not compared, and
             check_rows() holds them to one in ten with a row of the first tile and one of the partial last tile kept.  With these
             cases and baselines no row is flagged at any P (checked on the CPU).  The relu cases of input_grad_ref are not reused: 26
             of 70 rows of its headline are flagged at P = 16, 57 at P = 64; hence relu at 12 units and tanh at the wide shapes.  A
             16-layer case is left out on purpose: its band is some 400 times the attribution.
"""
import numpy as np

import forward_ref as fr
import input_grad_ref as ig
import tbnn_oracle as o

POINTS = (16, 32, 64)
# tag: dims, hidden activations, last activation, networks, rows, seed; the baseline is rng(seed).uniform(-0.5, 0.5, d_in)
CASES = {
    "headline-tanh": ([5, 50, 50, 50, 1], o.ACT_TANH, o.ACT_NONE, 4, 9, 21),      # 9 rows: 3, 5, 9 tiles at P = 16, 32, 64; fringe columns 48..49
    "relu-small": ([5, 12, 12, 1], o.ACT_RELU, o.ACT_NONE, 3, 9, 22),
    "one-input": ([1, 17, 1], o.ACT_TANH, o.ACT_NONE, 5, 1, 23),
    "no-hidden": ([3, 2], [], o.ACT_SIGMOID, 4, 5, 24),                           # the seed is G_1
    "odd-widths": ([33, 7, 19, 3], [o.ACT_ELU, o.ACT_TANH], o.ACT_EXP, 3, 6, 25),
    "16-outputs": ([6, 20, 20, 16], o.ACT_SIGMOID, o.ACT_NONE, 2, 5, 26),
    "16-row-tile": ([40, 200, 200, 2], o.ACT_TANH, o.ACT_NONE, 2, 3, 27),         # P = 16 only: P = 32 on it is refused
}
RUNS = [(tag, P) for tag in CASES for P in POINTS if tag != "16-row-tile" or P == 16]


def problem(tag, m=None):
    """(spec, X, thetas, baseline [d_in] fp32)"""
    dims, acts, last, nets, n, seed = CASES[tag]
    spec, X, thetas = fr.problem(dims, acts, last, nets if m is None else m, n, seed)
    return spec, X, thetas, np.random.default_rng(seed).uniform(-0.5, 0.5, dims[0]).astype(np.float32)


def path(X, baseline, P):
    """(the path points [n, P, d_in] and d = x - x0 [n, d_in], both fp32, and the trapezoid weights q [P] fp64)"""
    x0 = np.asarray(baseline, dtype=np.float32)
    d = (X - x0).astype(np.float32)
    a = np.arange(P, dtype=np.float32) / np.float32(P - 1)
    xs = (a.astype(np.float64)[None, :, None] * d.astype(np.float64)[:, None, :] + x0.astype(np.float64)).astype(np.float32)
    xs[:, P - 1] = X
    q = np.full(P, 1.0 / (P - 1))
    q[[0, P - 1]] *= 0.5
    return xs, d, q


def attributions(spec, thetas, X, baseline, P, dtype=np.float64, xform=ig.XFORM_NONE, scale=1.0):
    """(attr, tol [m, d_out, d_in, n] fp64, flagged [n] bool, diff [m, d_out, n] fp64 and its tolerance)"""
    n, d_in = X.shape
    xs, d, q = path(X, baseline, P)
    J, A, fl = ig.jacobian(spec, thetas, xs.reshape(n * P, d_in), dtype, xform, scale)
    J, A = (v.astype(np.float64).reshape(v.shape[:3] + (n, P)) for v in (J, A))
    dk = d.astype(np.float64).T[None, None]                                        # [1, 1, d_in, n]
    attr = dk * (J * q).sum(axis=-1)
    tol = np.abs(dk) * ((ig.gamma(spec) + (P + 4) * ig.U32) * (A + np.abs(J)) * q).sum(axis=-1)
    g = {ig.XFORM_EXP: np.exp, ig.XFORM_SIGMOID: lambda f: 1.0 / (1.0 + np.exp(-f))}.get(xform, np.asarray)
    t1, t0 = (scale * g(fr.reference(spec, thetas, x)) for x in (X, xs[:, 0]))     # the transformed outputs at x and at x0
    return attr, tol, fl.reshape(n, P).any(axis=1), t1 - t0, fr.tolerance(t1) + fr.tolerance(t0)


def check_rows(tag, flagged, P):
    """ig.check_rows with the tile of data rows the kernel uses: 64 / P rows, one under the 16-row tile"""
    return ig.check_rows(tag, flagged, tile=1 if tag == "16-row-tile" else 64 // P)
