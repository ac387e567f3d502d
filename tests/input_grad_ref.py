"""Input sensitivities against fp64: the problems, the reference and the band of tests/test_input_grad_host.py and
tests/test_gpu_input_grad.py.  No test functions here.

  reference  jacobian(): a plain NumPy reverse pass, network by network.  The forward runs in `dtype`, act' comes from the activation
             OUTPUTS by the oracle's act_grad_from_output (the formulas of act_bwd, csrc/common.hpp), J = s g'(f) df/dx.  Beside J it
             returns A, the same recursion on |W_l| and |act'|: the sum of the absolute products behind every element of J.
  band       tol = GAMMA (A + |J|), GAMMA = FACTOR sum_l (in_l + out_l + 4) 2^-24: one (k + 2) u per length-k dot product, forward and
             reverse, against the absolute product; FACTOR covers what the fp32 activations' own error does to act'.  It was supposed to
             be 2.  tests/test_input_grad_host.py holds the fp32 restatement of the reference to a quarter of the band, and at 2 the
             restatement itself missed that: 6.57 times the band (26 times the quarter) at a saturated sigmoid of the no-hidden case --
             act' = a (1 - a) from an fp32 a within an ulp of 1 carries a relative error of u / (1 - a), which no multiple of u against
             the absolute product describes.  Every other case stayed below 0.03.  On that evidence alone FACTOR is 64, the next power
             of two above 2 x 26.3.
  kinks      a relu unit whose pre-activation fp32 and fp64 may place on different sides of 0 changes a whole row's Jacobian and says
             nothing about a kernel: a row is flagged when, under any network, a relu unit has
             |z| < 4 (in_l + 2) 2^-24 (|W_l| |a_{l-1}| + |b_l|), four times the forward bound of that dot product.  Flagged rows are left
             out of the comparisons; check_rows() asserts they are at most one in ten and that a row of the first tile and one of a
             partial last tile are still compared.
"""
import numpy as np

import forward_ref as fr
import tbnn_oracle as o

U32 = 2.0 ** -24
FACTOR = 64.0
XFORM_NONE, XFORM_EXP, XFORM_SIGMOID = 0, 1, 2
MIXED = [o.ACT_RELU, o.ACT_TANH, o.ACT_SIGMOID, o.ACT_ELU, o.ACT_NONE] * 3      # 15 hidden layers: every code but exp ...

# tag: dims, hidden activations, last activation, networks, rows, seed
CASES = {
    "headline": ([5, 50, 50, 50, 1], o.ACT_RELU, o.ACT_NONE, 8, 70, 11),
    "one-input": ([1, 17, 1], o.ACT_TANH, o.ACT_NONE, 5, 1, 12),
    "no-hidden": ([3, 2], [], o.ACT_SIGMOID, 4, 19, 13),
    "odd-widths": ([33, 7, 19, 3], [o.ACT_ELU, o.ACT_TANH], o.ACT_EXP, 6, 65, 14),            # ... which the last layer here has
    "16-outputs": ([6, 20, 20, 16], o.ACT_SIGMOID, o.ACT_NONE, 4, 130, 15),
    "16-row-tile": ([40, 200, 200, 2], o.ACT_RELU, o.ACT_NONE, 3, 37, 16),
    "16-layers": ([5] + [9] * 15 + [1], MIXED, o.ACT_EXP, 3, 33, 17),
}


def problem(tag):
    dims, acts, last, m, n, seed = CASES[tag]
    return fr.problem(dims, acts, last, m, n, seed)


def layers_of(spec):
    return [(l.in_dim, l.out_dim, l.act, 0) for l in spec.layers]


def gamma(spec):
    return FACTOR * sum(l.in_dim + l.out_dim + 4 for l in spec.layers) * U32


def gprime(f, xform):
    if xform == XFORM_EXP:
        return np.exp(f)
    if xform == XFORM_SIGMOID:
        g = 1.0 / (1.0 + np.exp(-f))
        return (g * (1.0 - g)).astype(f.dtype)
    return np.ones_like(f)


def jacobian(spec, thetas, X, dtype=np.float64, xform=XFORM_NONE, scale=1.0):
    """(J, A, flagged): J, A [m, d_out, d_in, n] in `dtype`, flagged [n] bool"""
    n, d_out = X.shape[0], spec.layers[-1].out_dim
    Js, As = [], []
    flagged = np.zeros(n, dtype=bool)
    for th in thetas:
        parts = o.unflatten(spec, np.asarray(th, dtype=dtype))
        a = np.ascontiguousarray(np.asarray(X, dtype=dtype).T)
        acts = [a]
        for l, (W, b) in zip(spec.layers, parts):
            z = W @ a + b
            if l.act == o.ACT_RELU:
                bound = 4.0 * (l.in_dim + 2) * U32 * (np.abs(W) @ np.abs(a) + np.abs(b))
                flagged |= (np.abs(z) < bound).any(axis=0)
            a = o.activate(z, l.act)
            acts.append(a)
        f = acts[-1]
        seed = (dtype(scale) * gprime(f, xform) * o.act_grad_from_output(f, spec.layers[-1].act)).astype(dtype)
        G = np.eye(d_out, dtype=dtype)[:, :, None] * seed[None]                # [output o, unit j, row]
        Ab = np.abs(G)
        for li in range(len(parts) - 1, -1, -1):
            W = parts[li][0]
            G = np.einsum("ojn,jk->okn", G, W)
            Ab = np.einsum("ojn,jk->okn", Ab, np.abs(W))
            if li > 0:
                d = o.act_grad_from_output(acts[li], spec.layers[li - 1].act)
                G, Ab = G * d[None], Ab * np.abs(d)[None]
        Js.append(G)
        As.append(Ab)
    return np.stack(Js).astype(dtype), np.stack(As).astype(dtype), flagged


def tolerance(spec, J, A):
    return gamma(spec) * (A.astype(np.float64) + np.abs(J.astype(np.float64)))


def check_rows(tag, flagged, tile=64):
    """the rows a case compares: at most one in ten flagged, a row of the first tile and one of the partial last tile among the rest"""
    n = flagged.size
    keep = ~flagged
    assert flagged.sum() * 10 <= n, (tag, int(flagged.sum()), n)
    assert keep[:tile].any(), tag
    assert keep[n // tile * tile:].any() or n % tile == 0, tag
    return keep


def worst(got, J, tol, keep):
    """the largest err / tol over the compared rows (inf where got is not finite) and where"""
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got.astype(np.float64) - J.astype(np.float64)) / np.maximum(tol, np.finfo(np.float64).tiny)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)[..., keep]
    at = tuple(int(v) for v in np.unravel_index(np.argmax(ratio), ratio.shape))
    return float(ratio[at]), at
