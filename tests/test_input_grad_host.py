"""Input sensitivities without a GPU (tests/input_grad_ref.py: the reference, the band, the flagged rows): the fp32 restatement of the
reference stays within a quarter of the band of the fp64 one for every problem tests/test_gpu_input_grad.py uses -- the condition under
which missing the band says something about the kernel --, the reference differentiates the oracle's forward, and the entry point's
prototype and its refusal of a null handle.

Measured, the fp32 restatement's worst err / tol over the unflagged rows at the factor 2 the band was first given: headline 0.001,
one-input 0.006, no-hidden 6.567, odd-widths 0.029, 16-outputs 0.007, 16-row-tile and 16-layers below 0.0005 -- the no-hidden case 26 times
the quarter, hence the factor 64 of input_grad_ref.FACTOR, at which the same figures are 32 times smaller (no-hidden: 0.205)."""
import ctypes as C

import numpy as np
import pytest

import input_grad_ref as ig
import tbnn_oracle as o
from test_ensemble_host import CTYPE, header_prototypes


@pytest.mark.parametrize("tag", list(ig.CASES))
def test_fp32_reference_within_a_quarter_of_the_band(tag):
    spec, X, thetas = ig.problem(tag)
    xform = ig.XFORM_EXP if tag == "headline" else ig.XFORM_NONE
    J, A, flagged = ig.jacobian(spec, thetas, X, np.float64, xform, 2.5)
    keep = ig.check_rows(tag, flagged)
    J32, _A, _f = ig.jacobian(spec, thetas, X, np.float32, xform, 2.5)
    w, at = ig.worst(J32, J, ig.tolerance(spec, J, A), keep)
    print(f"[input_grad] {tag}: fp32 reference worst err/tol {w:.2e} at {at}; {int(flagged.sum())} of {flagged.size} rows flagged")
    assert w <= 0.25, (tag, w, at)


def test_reference_against_central_differences():
    spec, X, thetas = ig.fr.problem([4, 9, 6, 2], o.ACT_TANH, o.ACT_NONE, 2, 7, 5)
    J, _A, _f = ig.jacobian(spec, thetas, X, np.float64)
    h = 1e-6
    for k in range(4):
        e = np.zeros(4)
        e[k] = h
        for i, th in enumerate(thetas):
            fd = (o.forward(spec, th, X + e, np.float64) - o.forward(spec, th, X - e, np.float64)) / (2 * h)
            assert np.allclose(fd, J[i, :, k, :], rtol=1e-7, atol=1e-9), (i, k)


def test_null_handle_and_prototype(native):
    z = np.zeros(4, dtype=np.float64)
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    assert native.lib.tbnn_ensemble_input_grad(None, None, 1, 1, None, 0, 1.0, 0, None, 0, dp, None, None, None) < 0
    assert "null handle" in native.lib.tbnn_last_error().decode()
    proto = header_prototypes()["tbnn_ensemble_input_grad"]
    res, args = {name: (r, a) for name, r, a in native.SYMBOLS}["tbnn_ensemble_input_grad"]
    assert res is C.c_int and len(args) == len(proto) == 14
    for i, (a, t) in enumerate(zip(args, proto)):
        assert a is CTYPE[t], (i, t, a)
