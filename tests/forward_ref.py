"""The multi-network forward pass against fp64: a problem builder, the reference and the checker of tests/test_forward_ref_host.py and
tests/test_gpu_forward_many.py (and of the anchor in tests/test_gpu_ensemble.py::test_two_real_chunks).  No test functions here.

Every other ensemble module (test_gpu_ensemble / _quantiles / _predictive / _diagnostics / _loo) takes Chain.forward_many as its truth and
so isolates its reduction; this module is what forward_many itself is held against: oracle/tbnn_oracle.py's forward in fp64, network by
network, independent of the kernels.

  problem    X standard normal; per layer W ~ N(0, 2 / fan_in), b ~ N(0, 0.1^2), all rounded to fp32 once.  The fan-in scaling keeps every
             layer's pre-activations O(1) whatever the widths (784 inputs are divided by nothing), so that the fp32 ORACLE itself stays
             within a quarter of the tolerance below (tests/test_forward_ref_host.py asserts that for every problem the GPU module uses):
             the condition under which missing the tolerance says something about a kernel and not about fp32.
  tolerance  |got - ref| <= ATOL + RTOL |ref| per element with tests/test_gpu_metrics.py::test_forward_many's own rtol = atol = 2e-5.
             One tier, every element, no skips.
"""
import numpy as np

import tbnn_oracle as o

RTOL = 2e-5
ATOL = 2e-5


def spec_of(dims, acts, last_act):
    """acts: the hidden layers' activation, or one per hidden layer"""
    nl = len(dims) - 1
    hidden = [int(acts)] * (nl - 1) if np.isscalar(acts) else [int(a) for a in acts]
    assert len(hidden) == nl - 1
    layers = [o.DenseSpec(dims[i], dims[i + 1], hidden[i] if i < nl - 1 else int(last_act), o.PRIOR_CAUCHY) for i in range(nl)]
    return o.NetSpec(layers, o.LIK_GAUSSIAN)


def problem(dims, acts, last_act, m, n, seed):
    """(spec, X [n, d_in] fp32, thetas [m, P] fp32 in the library's layout: per layer W[out, in] then b[out])"""
    spec = spec_of(dims, acts, last_act)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dims[0])).astype(np.float32)
    thetas = np.empty((m, spec.n_params), dtype=np.float32)
    for l, (ow, ob) in zip(spec.layers, spec.offsets()):
        thetas[:, ow:ob] = rng.standard_normal((m, ob - ow)) * np.sqrt(2.0 / l.in_dim)
        thetas[:, ob:ob + l.out_dim] = rng.standard_normal((m, l.out_dim)) * 0.1
    return spec, X, thetas


def reference(spec, thetas, X, rows=None, dtype=np.float64):
    """[m, d_out, len(rows)]: the oracle's forward of every network over X[rows] (all rows when None).  The oracle works row by row, so
    a subset of the rows is the same computation (to the order of an fp64 sum)"""
    Xr = X if rows is None else X[np.asarray(rows)]
    return np.stack([o.forward(spec, th, Xr, dtype) for th in thetas])


def tolerance(ref):
    return ATOL + RTOL * np.abs(ref)


def check(got, ref, tag):
    """got: fp32 predictions [m, d_out, rows] (or [d_out, rows] of one network), ref: fp64 of the same shape.  Prints the worst element,
    then asserts every one"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float32, (tag, got.dtype)
    assert ref.dtype == np.float64, (tag, ref.dtype)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    if got.ndim == 2:
        got, ref = got[None], ref[None]
    assert got.ndim == 3 and got.size > 0, (tag, got.shape)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got.astype(np.float64) - ref) / tolerance(ref)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)                # a NaN or an infinity anywhere fails
    at = tuple(int(v) for v in np.unravel_index(np.argmax(ratio), ratio.shape))
    worst = float(ratio[at])
    print(f"[forward] {tag}: worst err/tol {worst:.3f} at (network, output, row) = {at}")
    assert worst <= 1.0, (tag, worst, at, float(got[at]), float(ref[at]))
    return worst


def check_duplicates(got, pairs):
    """networks given identical thetas within one launch: the same tiles, the same weights, another blockIdx.y -- bit for bit"""
    for a, b in pairs:
        same = got[a].view(np.uint32) == got[b].view(np.uint32)
        assert same.all(), (a, b, int((~same).sum()), tuple(int(v) for v in np.argwhere(~same)[0]))


def row_subset(n, periods):
    """the rows a large case takes its reference on: every 7th row, the first 64 and the last 64, and the 64 rows on either side of every
    multiple of each period (the rows one round of a capped grid covers) -- sorted, unique, never fewer than 2,000 (or all n)"""
    keep = np.zeros(n, dtype=bool)
    keep[::7] = True
    keep[:64] = True
    keep[-64:] = True
    for p in periods:
        for edge in range(p, n + 64, p):
            keep[max(edge - 64, 0):min(edge + 64, n)] = True
    rows = np.flatnonzero(keep)
    assert rows.size >= min(n, 2000)
    return rows
