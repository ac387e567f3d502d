"""GPU: every branch of the narrow fused kernel's prologue (k_fwd_bwd_fast3, kernels_fast3.hpp) against the fp64 oracle.

The prologue requests a wave's first tile and the W / bias images before it splits the row tiles into full rounds and cooperative rounds, and
sends the W^T images behind its barrier, to be waited for behind the first forward pass -- or at once, when a wave of the workgroup has no
tile.  With TBNN_FAST_GRID=2 (W = 8 waves) the row counts below put the number of row tiles into each branch of that split: 5 (waves
without a tile: the early W^T wait), 16 (no remainder), 17 (one cooperative round), 19 (two), 21 (a plain extra round); each as
16 ntiles - 3 rows, so that the last tile is ragged; and 1 and 15 rows.  Both ahead-of-time shapes: 5 -> 50 -> 50 -> 50 -> 1 and
1 -> 10 -> 10 -> 1 (the loop form of the cooperative tail).  tests/test_gpu_parity.py (test_logp_grad_fast_cooperative_tail) sweeps the
cooperative rounds of the first shape at grids of 3 to 10 workgroups; the row counts here are the ones it leaves out.

Value, gradient and the forward-only kernel; the parity tolerances of tests/test_gpu_depth.py (log-prob 4e-6 relative, gradient 1e-4 of each
tensor's inf-norm, forward 2e-5), the fp32 oracle inside them first.  Every launch runs three times and must be bit-identical."""
import numpy as np
import pytest

import tbnn_oracle as o
from tensor_checks import layers_of, tensor_err
from test_gpu_depth import FLOOR, FWD_TOL, GRAD_TOL, LOGP_RTOL, fwd_err, problem, thrice

pytestmark = pytest.mark.gpu

GRID = 2
SHAPES = {"5-50-50-50-1": [5, 50, 50, 50, 1], "1-10-10-1": [1, 10, 10, 1]}
NTILES = {"idle-waves": 5, "no-remainder": 16, "one-coop-round": 17, "two-coop-rounds": 19, "extra-round": 21}
ROWS = {k: 16 * v - 3 for k, v in NTILES.items()}
ROWS.update({"one-row": 1, "fifteen-rows": 15})
CASES = [(s, r) for s in SHAPES for r in ROWS]


def test_the_row_counts_reach_every_branch():
    W, G = 4 * GRID, GRID
    rem = {k: v % W for k, v in NTILES.items()}
    assert NTILES["idle-waves"] < W and rem["no-remainder"] == 0 and 0 < rem["one-coop-round"] <= G
    assert G < rem["two-coop-rounds"] <= 2 * G and rem["extra-round"] > 2 * G
    assert all((16 * v - 3 + 15) // 16 == v for v in NTILES.values())


@pytest.mark.parametrize("shape,rows", CASES, ids=[f"{s}-{r}" for s, r in CASES])
def test_value_gradient_forward(native, monkeypatch, shape, rows):
    monkeypatch.setenv("TBNN_FAST_GRID", str(GRID))
    dims, n = SHAPES[shape], ROWS[rows]
    spec, X, Y, theta, eta = problem(dims, n, acts=[o.ACT_RELU] * (len(dims) - 2), seed=len(dims) + n)
    lp64, g64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[:2]
    f64 = o.forward(spec, theta, X, np.float64)
    lp32, g32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)[:2]
    assert abs(lp32 - lp64) <= LOGP_RTOL * max(abs(lp64), 1.0), ("fp32 oracle", lp32, lp64)
    assert tensor_err(spec, g32, g64, FLOOR) <= GRAD_TOL, ("fp32 oracle gradient", tensor_err(spec, g32, g64, FLOOR))
    assert fwd_err(o.forward(spec, theta, X, np.float32), f64) <= FWD_TOL, "fp32 oracle forward"
    ch = native.Chain(layers_of(spec), likelihood=spec.likelihood, fixed_sd=spec.fixed_sd, jit=False)
    try:
        name = ch.kernel_name
        assert "fast3" in name, name
        ch.set_data(X, Y)
        lp, g, _ = thrice(lambda: ch.logp_grad(theta, eta))
        f = thrice(lambda: (ch.forward(X, theta),))[0]
    finally:
        ch.close()
    e_lp, e_g, e_f = abs(lp - lp64) / max(abs(lp64), 1.0), tensor_err(spec, g, g64, FLOOR), fwd_err(f, f64)
    print(f"{name} {n} rows: logp {e_lp:.2e} ({LOGP_RTOL}) gradient per tensor {e_g:.2e} ({GRAD_TOL}) forward {e_f:.2e} ({FWD_TOL})")
    assert e_lp <= LOGP_RTOL, f"{name}: logp {lp} against {lp64} ({e_lp:.2e} relative)"
    assert e_g <= GRAD_TOL, f"{name}: gradient {e_g:.3e} of a tensor's inf-norm"
    assert e_f <= FWD_TOL, f"{name}: forward {e_f:.3e}"
