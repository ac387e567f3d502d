"""CPU: what tests/test_gpu_forward_many.py rests on (tests/forward_ref.py).

Conditioning.  The tolerance |got - ref| <= 2e-5 + 2e-5 |ref| says something about a kernel only where fp32 itself is far inside it: for
every problem the GPU module runs (and the one tests/test_gpu_ensemble.py::test_two_real_chunks anchors), the fp32 ORACLE must stay
within a quarter of the tolerance of the fp64 oracle -- over the first 2,000 rows and 4 networks.  A problem that does not is changed,
never the tolerance.

The checker can fail.  Five defects a wrong grid, tile or offset would cause, applied to a reference of the shape [9, 2, 1237]: each must
raise; the reference rounded to fp32 must pass."""
import numpy as np
import pytest

import forward_ref as fr
import tbnn_oracle as o
import test_gpu_ensemble as ens
import test_gpu_forward_many as gpu

PROBLEMS = gpu.problems()


def conditioning(spec, X, thetas):
    X, thetas = X[:2000], thetas[:4]
    r64 = fr.reference(spec, thetas, X)
    r32 = fr.reference(spec, thetas, X, dtype=np.float32)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    return float(np.max(np.abs(r32.astype(np.float64) - r64) / fr.tolerance(r64)))


@pytest.mark.parametrize("case", PROBLEMS, ids=[p[0].replace(" ", "-") for p in PROBLEMS])
def test_fp32_oracle_within_a_quarter_of_the_tolerance(case):
    tag, dims, act, last, m, n, seed = case
    spec, X, thetas = fr.problem(dims, act, last, m, n, seed)
    assert X.shape == (n, dims[0]) and X.dtype == np.float32
    assert thetas.shape == (m, spec.n_params) and thetas.dtype == np.float32
    worst = conditioning(spec, X, thetas)
    print(f"[forward] {tag}: fp32 oracle at {worst:.3f} of the tolerance")
    assert worst <= 0.25, (tag, worst)


def test_fp32_oracle_on_the_two_real_chunks_problem():
    """test_two_real_chunks keeps tests/test_gpu_ensemble.py's own problem() (12-40-10 Tanh, 1,000,003 rows, seed 3)"""
    dims, act, last = ens.CASES["layered10"][:3]
    X, thetas = ens.problem("layered10", 28, seed=3, n=1_000_003)
    worst = conditioning(fr.spec_of(dims, act, last), X, thetas)
    print(f"[forward] two real chunks: fp32 oracle at {worst:.3f} of the tolerance")
    assert worst <= 0.25, worst


def test_problem_layout_and_scaling():
    """per layer W[out, in] then b[out] (oracle/tbnn_oracle.py: unflatten); weights N(0, 2 / fan_in), biases N(0, 0.1^2)"""
    spec, X, thetas = fr.problem([784, 20, 20, 10], o.ACT_RELU, o.ACT_SIGMOID, 50, 300, 1)
    assert [l.act for l in spec.layers] == [o.ACT_RELU, o.ACT_RELU, o.ACT_SIGMOID]
    for l, (ow, ob) in zip(spec.layers, spec.offsets()):
        W, b = thetas[:, ow:ob], thetas[:, ob:ob + l.out_dim]
        assert abs(W.std() / np.sqrt(2.0 / l.in_dim) - 1) < 0.05 and abs(b.std() / 0.1 - 1) < 0.12
    assert abs(X.std() - 1) < 0.01
    ref = fr.reference(spec, thetas[:3], X, rows=[5, 17, 299])
    assert ref.shape == (3, 10, 3) and ref.dtype == np.float64
    # a row subset is the same computation row by row; a BLAS may sum a row's 784 products in another order for another matrix shape:
    # 784 x 2^-53 of values of order 1, nothing beside the 2e-5 of the tolerance
    assert np.abs(ref - fr.reference(spec, thetas[:3], X)[:, :, [5, 17, 299]]).max() <= 784 * 2.0 ** -53 * 8


def test_row_subset():
    rows = fr.row_subset(131377, [512 * 64, 512 * 256])
    assert rows.size >= 2000 and np.all(np.diff(rows) > 0) and rows[0] == 0 and rows[-1] == 131376
    for edge in (32768, 65536, 98304, 131072):
        assert np.isin(np.arange(edge - 64, edge + 64), rows).all()
    assert np.isin(np.arange(131377 - 64, 131377), rows).all() and np.isin(np.arange(64), rows).all()
    assert np.array_equal(fr.row_subset(300, [64])[:130], np.arange(130))


# ------------------------------------------------------------------------------------------------------------------ the checker can fail
@pytest.fixture(scope="module")
def ref9():
    spec, X, thetas = fr.problem([7, 33, 18, 50, 2], o.ACT_RELU, o.ACT_NONE, 9, 1237, 77)
    ref = fr.reference(spec, thetas, X)
    assert ref.shape == (9, 2, 1237)
    ref.setflags(write=False)
    return ref


def swapped(ref):
    bad = ref.copy()
    bad[[2, 5]] = ref[[5, 2]]
    return bad


def ragged_tile_zeroed(ref):
    bad = ref.copy()
    bad[4, :, 1232:] = 0.0
    return bad


def shifted_by_a_tile(ref):
    bad = ref.copy()
    bad[3, :, 1024:1237 - 16] = ref[3, :, 1040:]
    return bad


def planes_exchanged(ref):
    bad = ref.copy()
    bad[7] = ref[7, ::-1]
    return bad


def one_element_moved(ref):
    bad = ref.copy()
    bad[8, 1, 1236] += 4e-5 * (1 + abs(ref[8, 1, 1236]))
    return bad


def test_checker_passes_on_fp32_rounding(ref9, capsys):
    worst = fr.check(ref9.astype(np.float32), ref9, "rounded")
    assert worst < 0.01
    assert "[forward] rounded: worst err/tol" in capsys.readouterr().out
    fr.check(ref9[0].astype(np.float32), ref9[0], "one network")                  # [d_out, rows] of a single call


@pytest.mark.parametrize("defect", [swapped, ragged_tile_zeroed, shifted_by_a_tile, planes_exchanged, one_element_moved])
def test_checker_catches(ref9, defect):
    bad = defect(ref9).astype(np.float32)
    assert bad.shape == ref9.shape
    with pytest.raises(AssertionError):
        fr.check(bad, ref9, defect.__name__)


def test_checker_asserts_shape_dtype_and_finiteness(ref9):
    got = ref9.astype(np.float32)
    with pytest.raises(AssertionError):
        fr.check(ref9.copy(), ref9, "fp64 predictions")
    with pytest.raises(AssertionError):
        fr.check(got[:, :, :-1], ref9, "a row short")
    bad = got.copy()
    bad[1, 0, 3] = np.nan
    with pytest.raises(AssertionError):
        fr.check(bad, ref9, "a NaN")


def test_check_duplicates(ref9):
    got = ref9.astype(np.float32)
    got[8] = got[0]
    fr.check_duplicates(got, [(0, 8)])
    got[8, 1, 1000] = np.nextafter(got[8, 1, 1000], np.float32(np.inf))
    with pytest.raises(AssertionError):
        fr.check_duplicates(got, [(0, 8)])
