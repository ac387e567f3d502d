"""GPU: the multi-network forward pass of every kernel family (Backend::forward, csrc/backend.hpp -- what tbnn_forward, tbnn_predict,
tbnn_metrics, tbnn_forward_many and every ensemble reduction predict with) against the fp64 oracle, network by network
(tests/forward_ref.py: the problems, the reference, the tolerance -- tests/test_gpu_metrics.py::test_forward_many's rtol = atol = 2e-5 on
every element -- and why it means something).  The ensemble modules take Chain.forward_many as their truth ("the forward kernels are
shared, so both sides see the same bits"); this module is what that truth rests on.

What the cases reach, read against the code:

  grid regimes   FusedBackend::forward launches min(ceil(ceil(n / 16) / 4), cap) workgroups per network (gridDim.y = network), cap = 256
                 below 8 networks, 64 from 8 and 16 from 64; a workgroup takes 64 rows a round.  (1, 20,011), (7 | 8, 5,003) and
                 (63 | 64 | 65, 1,237) cross each cap from both sides of its network count and leave an uneven number of rounds per
                 workgroup (313 groups on 256, 79 on 64, 20 on 16) with a ragged last tile -- k_forward_fast3's stride, and the
                 next-round prefetch of k_fwd_bwd_mid<S, true> and k_fwd_bwd_tall<S, NW, true, 4>.  The wide forward (one launch per
                 network) caps at 256 workgroups = 16,384 rows, generic_forward at 512 blocks of 256 rows = 131,072 rows, the layered
                 family's k_lay_pack_x at 4,096 blocks (784 inputs: from 336 rows) and k_lay_unpack_f at 2,048 tiles = 32,768 rows.
  drivers        ensemble_row_blocks runs every family at dX + r0 * d_in over blocks of 64 and of 128 rows with a ragged last block;
                 ensemble_forward cuts 8 networks into chunks of 3, 3 and 2 (csrc/ensemble_api.hpp).
  single calls   predict over both staged row sets, forward over host rows, forward_many over both staged row sets.

Where a case's last network is a copy of its first, the two must agree bit for bit: the same grid, the same tiles, the same weights,
another blockIdx.y (or another launch).

The wide family's handles whose kernel library has no forward instantiation (wide_forward_ok<S>() false: a streamed weight image with
fewer than three forward chunks, csrc/kernels_wide.hpp) would predict through generic_forward under a `wide<` name.  No admitted shape
is one: fewer than three forward chunks means sum_l ceil(in(l) / 16) <= 2 over the middle layers, i.e. ONE middle layer of at most 32
inputs (one or two outputs) or two of at most 16 each; with the family's limits (fan-in <= 128, widths <= 256) such an image takes at
most 16 KB (W_0) + 32 KB + 32 KB (the two segments of a 32 x 256 layer) next to 55 KB of per-wave scratch, below the 160 KB at which
WideCfg::RESIDENT keeps it in LDS -- and a resident image has a forward kernel.  The only shape forced onto the stream (the registry's
20-32-16-48-2) has three forward chunks.  So that case is left out.

The multi-output shapes are run-time instantiations listed in tests/jit_shapes.json (tests/test_gpu_traj.py's and
tests/test_gpu_multiout.py's, under the latter's likelihoods and TBNN_JIT_SKIP); the others are ahead-of-time shapes (jit=False), built as
tests/test_gpu_ensemble.py builds them.  A shape that does not land on its family fails on the kernel name; nothing skips.
"""
import numpy as np
import pytest

import forward_ref as fr
import tbnn_oracle as o

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LIK_GAUSSIAN, LIK_FIXED_GAUSSIAN, LIK_BERNOULLI = 0, 1, 2
SKIP = {"mid": "fast3,fast,tall,wide", "tall": "fast3,fast,mid,wide", "wide": "fast3,fast,mid,tall"}      # tests/test_gpu_multiout.py

SHAPES = {
    # dims, hidden activation, last activation, the handle's likelihood, kernel-name prefix, TBNN_JIT_SKIP of a run-time shape (None: jit=False)
    "narrow": ([5, 50, 50, 50, 1], o.ACT_RELU, o.ACT_NONE, LIK_FIXED_GAUSSIAN, "fast3<", None),
    "narrow2": ([7, 17, 33, 2], o.ACT_RELU, o.ACT_NONE, LIK_GAUSSIAN, "jit-fast3<", ""),
    "mid": ([7, 33, 18, 50, 2], o.ACT_RELU, o.ACT_NONE, LIK_GAUSSIAN, "mid<", None),
    "mid5": ([20, 64, 64, 5], o.ACT_RELU, o.ACT_NONE, LIK_GAUSSIAN, "jit-mid<", SKIP["mid"]),
    "tall": ([784, 20, 20, 1], o.ACT_RELU, o.ACT_SIGMOID, LIK_BERNOULLI, "tall<", None),
    "tall10": ([784, 20, 20, 10], o.ACT_RELU, o.ACT_SIGMOID, LIK_BERNOULLI, "jit-tall<", SKIP["tall"]),
    "wide": ([10, 200, 200, 200, 1], o.ACT_RELU, o.ACT_NONE, LIK_GAUSSIAN, "wide<", None),
    "wide2": ([3, 20, 36, 2], o.ACT_TANH, o.ACT_NONE, LIK_GAUSSIAN, "wide<", None),
    "wide10": ([10, 200, 200, 10], o.ACT_RELU, o.ACT_SIGMOID, LIK_BERNOULLI, "jit-wide", SKIP["wide"]),
    "layered10": ([12, 40, 10], o.ACT_TANH, o.ACT_NONE, LIK_FIXED_GAUSSIAN, "layered<", None),
    "layered784": ([784, 100, 100, 10], o.ACT_RELU, o.ACT_NONE, LIK_FIXED_GAUSSIAN, "layered<", None),
    "generic4": ([5, 16, 16, 4], o.ACT_TANH, o.ACT_NONE, LIK_FIXED_GAUSSIAN, "generic", None),
}
BATCHED = ("narrow", "narrow2", "mid", "mid5", "tall", "tall10")        # one launch, gridDim.y = network (FusedBackend::forward)
ONE_OUTPUT = ("narrow", "mid", "tall", "wide", "wide2", "layered10", "generic4")      # the first shape(s) of every family

GRID_CASES = ([(name, m, n) for name in ("narrow", "mid", "tall")
               for m, n in ((1, 20011), (7, 5003), (8, 5003), (63, 1237), (64, 1237), (65, 1237), (9, 300))]
              + [(name, m, n) for name in ("narrow2", "mid5", "tall10") for m, n in ((64, 1237), (3, 20011))]
              + [("wide2", 1, 16407), ("wide2", 3, 20011), ("wide", 2, 1237), ("wide10", 2, 1237)]
              + [("layered10", 3, 1203), ("layered10", 2, 33007), ("layered784", 2, 1205)]
              + [("generic4", 2, 131377), ("generic4", 6, 517)])
SUBSET_FROM = 33007                       # the two largest row counts take their reference on forward_ref.row_subset
STAGED = (8, 5003, 1237)                  # test_staged_rows_and_single_calls: networks, training rows, validation rows
BLOCKS = (9, 333)                         # test_row_blocks_every_family: networks, rows
CHUNKS = (8, 517)                         # test_network_chunks_every_family: networks, rows


def seed_of(test, name, m, n):
    return 1000 * test + 37 * list(SHAPES).index(name) + m + n % 101


def problems():
    """every (tag, dims, hidden activation, last activation, m, n, seed) this module runs: tests/test_forward_ref_host.py asserts the
    conditioning of each"""
    out = [(f"grid {name} m={m} n={n}", name, m, n, seed_of(1, name, m, n)) for name, m, n in GRID_CASES]
    out += [(f"staged {name}", name, STAGED[0], STAGED[1] + STAGED[2], seed_of(2, name, *STAGED[:2])) for name in ONE_OUTPUT]
    out += [(f"blocks {name}", name, *BLOCKS, seed_of(3, name, *BLOCKS)) for name in SHAPES]
    out += [(f"chunks {name}", name, *CHUNKS, seed_of(4, name, *CHUNKS)) for name in SHAPES]
    return [(tag, *SHAPES[name][:3], m, n, seed) for tag, name, m, n, seed in out]


def make_problem(test, name, m, n):
    dims, act, last = SHAPES[name][:3]
    return fr.problem(dims, act, last, m, n, seed_of(test, name, m, n))


def make_chain(native, monkeypatch, name):
    dims, act, last, lik, prefix, skip = SHAPES[name]
    layers = [(dims[i], dims[i + 1], act if i < len(dims) - 2 else last, 0) for i in range(len(dims) - 1)]
    if skip is not None:
        monkeypatch.setenv("TBNN_JIT_SKIP", skip)
    kernel = native.KERNEL_GENERIC if prefix == "generic" else native.KERNEL_AUTO
    ch = native.Chain(layers, likelihood=lik, fixed_sd=0.7, kernel=kernel, jit=skip is not None)
    assert ch.kernel_name.startswith(prefix), (name, ch.kernel_name)
    return ch


def round_rows(name, m):
    """(workgroups' cap, rows one round of the capped grid covers) of the family's forward launch"""
    if name in BATCHED:
        cap = 16 if m >= 64 else 64 if m >= 8 else 256
        return cap, cap * 64
    if name.startswith("wide"):
        return 256, 256 * 64
    if name.startswith("layered"):
        return 2048, 2048 * 16                          # k_lay_unpack_f's tiles (k_lay_pack_x: 4,096 blocks over tiles x k-tiles)
    return 512, 512 * 256                               # generic_forward


# ------------------------------------------------------------------------------------------------------------------------- (a) the grids
@pytest.mark.parametrize("name,m,n", GRID_CASES, ids=[f"{a}-m{b}-n{c}" for a, b, c in GRID_CASES])
def test_grid_regimes(native, monkeypatch, name, m, n):
    assert n % 16 != 0
    spec, X, thetas = make_problem(1, name, m, n)
    if m > 1:
        thetas[m - 1] = thetas[0]
    ch = make_chain(native, monkeypatch, name)
    got = ch.forward_many(thetas, X=X)
    ch.close()
    d_out = SHAPES[name][0][-1]
    assert got.shape == (m, d_out, n) and got.dtype == np.float32
    if m > 1:
        fr.check_duplicates(got, [(0, m - 1)])
    cap, per_round = round_rows(name, m)
    rows = fr.row_subset(n, [cap * 64, per_round]) if n >= SUBSET_FROM else np.arange(n)
    ref = fr.reference(spec, thetas, X, rows)
    fr.check(got[:, :, rows], ref, f"{name} m={m} n={n} ({rows.size} rows checked): cap {cap}, {n / per_round:.2f} rounds of {per_round} rows")


# --------------------------------------------------------------------------------------------------- (b) staged rows and the single calls
@pytest.mark.parametrize("name", ONE_OUTPUT)
def test_staged_rows_and_single_calls(native, monkeypatch, name):
    """forward_many over the staged training and validation rows, predict over both with an explicit theta, forward over host rows: each
    against fp64 (what they share bit for bit is asserted in tests/test_gpu_metrics.py and tests/test_gpu_ensemble.py, not assumed here)"""
    m, n, nv = STAGED
    spec, Xall, thetas = fr.problem(*SHAPES[name][:3], m, n + nv, seed_of(2, name, m, n))
    X, Xv = Xall[:n], Xall[n:]
    d_out = SHAPES[name][0][-1]
    ref_t, ref_v = fr.reference(spec, thetas, X), fr.reference(spec, thetas, Xv)
    ch = make_chain(native, monkeypatch, name)
    ch.set_data(X, np.zeros((n, d_out), dtype=np.float32))
    ch.set_validation(Xv, np.zeros((nv, d_out), dtype=np.float32))
    fr.check(ch.forward_many(thetas, which=0), ref_t, f"{name} forward_many(which=0) m={m} n={n}")
    fr.check(ch.forward_many(thetas, which=1), ref_v, f"{name} forward_many(which=1) m={m} n={nv}")
    fr.check(np.stack([ch.predict(0, th) for th in thetas]), ref_t, f"{name} predict(0, theta_i) n={n}")
    fr.check(np.stack([ch.predict(1, th) for th in thetas]), ref_v, f"{name} predict(1, theta_i) n={nv}")
    fr.check(np.stack([ch.forward(X, th) for th in thetas]), ref_t, f"{name} forward(X, theta_i) n={n}")
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------- (c) row blocks
@pytest.mark.parametrize("rb", [64, 128])
@pytest.mark.parametrize("name", list(SHAPES))
def test_row_blocks_every_family(native, monkeypatch, name, rb):
    """ensemble_row_blocks (csrc/ensemble_api.hpp) runs a block's forward passes at dX + r0 * d_in.  The inverted-CDF quantiles at 0, 1/2
    and 1 are, per element, the smallest, the lower median and the largest of the device's nine fp32 predictions, converted exactly; an
    order statistic is 1-Lipschitz in the sup norm of its arguments (tests/test_gpu_quantiles.py), so each lies within the forward
    tolerance of the fp64 reference's order statistic -- and a block run at another row offset, or a ragged block reading past its rows,
    is an O(1) error there."""
    m, n = BLOCKS
    assert n % 64 == 13
    spec, X, thetas = make_problem(3, name, m, n)
    d_out = SHAPES[name][0][-1]
    budget = m * d_out * rb + 7
    assert max(64, budget // (m * d_out) // 64 * 64) == rb                         # the driver's rule (ens_block_rows) ...
    blocks = [(r0, min(rb, n - r0)) for r0 in range(0, n, rb)]
    assert blocks[-1] == {64: (320, 13), 128: (256, 77)}[rb] and len(blocks) == {64: 6, 128: 3}[rb]       # ... and what it cuts
    probs = [0.0, 0.5, 1.0]
    ref = np.quantile(fr.reference(spec, thetas, X), probs, axis=0, method="inverted_cdf")
    ch = make_chain(native, monkeypatch, name)
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    got = ch.ensemble_quantiles(thetas, probs, X=X, method="inverted_cdf")
    assert got.dtype == np.float64 and np.array_equal(got, got.astype(np.float32).astype(np.float64))
    fr.check(got.astype(np.float32), ref, f"{name} blocks of {rb} rows, explicit X (quantile, output, row)")
    ch.set_data(X, np.zeros((n, d_out), dtype=np.float32))
    got = ch.ensemble_quantiles(thetas, probs, which=0, method="inverted_cdf")
    assert np.array_equal(got, got.astype(np.float32).astype(np.float64))
    fr.check(got.astype(np.float32), ref, f"{name} blocks of {rb} rows, staged rows (quantile, output, row)")
    ch.close()


# -------------------------------------------------------------------------------------------------------------------- (d) network chunks
@pytest.mark.parametrize("name", list(SHAPES))
def test_network_chunks_every_family(native, monkeypatch, name):
    """ensemble_forward cuts 8 networks into chunks of 3, 3 and 2.  The unweighted mean against the fp64 reference's mean: each f_i within
    the forward tolerance (taken at the largest |ref_i| of the element), plus the moments' own 4 m U max_i |f_i - f_0|
    (tests/test_gpu_ensemble.py).  With all the weight on network 6 -- the first of the third chunk -- the mean IS that network."""
    m, n = CHUNKS
    spec, X, thetas = make_problem(4, name, m, n)
    d_out = SHAPES[name][0][-1]
    budget = 3 * d_out * n + 5
    assert min(m, budget // (d_out * n)) == 3                                      # ensemble_forward's rule: 3 + 3 + 2
    ref = fr.reference(spec, thetas, X)
    ch = make_chain(native, monkeypatch, name)
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    mean, _var = ch.ensemble_moments(thetas, X=X)
    one, _var = ch.ensemble_moments(thetas, X=X, weights=[0, 0, 0, 0, 0, 0, 1, 0])
    ch.close()
    tol_f = fr.tolerance(np.abs(ref).max(axis=0))
    span = np.abs(ref - ref[0]).max(axis=0) + 2 * tol_f                            # of the device's f_i, each within tol_f of ref_i
    tol = tol_f + 4 * m * U * span
    err = np.abs(mean - ref.mean(axis=0))
    print(f"[forward] {name} chunks of 3 + 3 + 2 networks, n={n}: mean worst err/tol {np.max(err / tol):.3f}")
    assert mean.shape == (d_out, n) and mean.dtype == np.float64 and np.all(np.isfinite(mean))
    assert np.all(err <= tol), (name, float(np.max(err / tol)))
    # f_0 + (f_6 - f_0) in fp64 is f_6 itself (or one fp64 rounding from it: nothing at fp32)
    fr.check(one.astype(np.float32), ref[6], f"{name} chunks of 3 + 3 + 2 networks: network 6 (third chunk) through the weights")
