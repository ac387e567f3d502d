"""GPU: the narrow fused kernel's row bookkeeping (k_fwd_bwd_fast3, kernels_fast3.hpp) against the fp64 oracle.

The tile loop keeps which tile a trip runs in scalar registers: a 32-bit trip count per wave, scalar row pointers, and three wave-uniform
cases of a tile -- full (no per-lane predicate at all), the one ragged tile of the data set (its last, when n % 16 != 0; named by the wave
and the trip it falls on) and an absent next tile (no request).  With TBNN_FAST_GRID=2 (G = 2 workgroups, W = 8 waves) the row counts below
put the ragged tile and the absent tile where those cases split:
  24 tiles            three full rounds, no cooperative round: the ragged tile is wave 7's last trip, with 13 rows and with a single row;
                      and 16 * 24 rows exactly, where no tile is ragged;
  25 tiles            the ragged tile is the cooperative tile;
  9 and 11 tiles      one round, every wave without a next trip; then one cooperative round (9) or two (11);
  17 rows             the ragged tile is a wave's only tile (a cooperative one) and waves stand idle;
  6 tiles             a plain round of six waves' only trips (no cooperative round: the remainder is above 2 G): the ragged tile is trip 0 of
                      wave 5 -- its rows come from the prologue's per-lane fetch, not from the loop's -- and two waves of workgroup 1 are idle.
Both ahead-of-time shapes, 5 -> 50 -> 50 -> 50 -> 1 and 1 -> 10 -> 10 -> 1.  A two-chain ChainGroup at 24 tiles, ragged, must give the solo
chains' bits: blockIdx.y's offsets meet the scalar row pointers.

Value, gradient and the forward-only kernel under the tolerances of tests/test_gpu_depth.py (log-prob 4e-6 relative, gradient 1e-4 of each
tensor's inf-norm, forward 2e-5), the fp32 oracle inside them first.  Every launch runs three times and must be bit-identical."""
import numpy as np
import pytest

import tbnn_oracle as o
from tensor_checks import layers_of, tensor_err
from test_gpu_depth import FLOOR, FWD_TOL, GRAD_TOL, LOGP_RTOL, fwd_err, problem, thrice

pytestmark = pytest.mark.gpu

GRID = 2
SHAPES = {"5-50-50-50-1": [5, 50, 50, 50, 1], "1-10-10-1": [1, 10, 10, 1]}
ROWS = {"ragged-last-round-13": 16 * 24 - 3, "ragged-last-round-1": 16 * 24 - 15, "no-ragged-tile": 16 * 24,
        "ragged-coop-tile": 16 * 25 - 7, "one-trip-one-coop": 16 * 9 - 3, "one-trip-two-coops": 16 * (8 + 3) - 3, "seventeen-rows": 17,
        "ragged-first-trip": 16 * 6 - 3}
CASES = [(s, r) for s in SHAPES for r in ROWS]


def split(n, G=GRID):
    """the kernel's plan for n rows on G workgroups, restated: (ntiles, trips per wave, (wave, trip) of the ragged tile in the loop or None,
    cooperative rounds, index of the ragged tile or None)"""
    W = 4 * G
    ntiles = (n + 15) // 16
    q, rem = divmod(ntiles, W)
    coop = 0 if rem == 0 or rem > 2 * G else (1 if rem <= G else 2)
    main_end = ntiles - rem if coop else ntiles
    trips = [len(range(w, main_end, W)) for w in range(W)]
    ragged = ntiles - 1 if n % 16 else None
    in_loop = (ragged % W, ragged // W) if ragged is not None and ragged < main_end else None
    return ntiles, trips, in_loop, coop, ragged


def test_the_row_counts_reach_every_case():
    W = 4 * GRID
    for key in ("ragged-last-round-13", "ragged-last-round-1"):
        ntiles, trips, in_loop, coop, ragged = split(ROWS[key])
        assert ntiles == 24 and trips == [3] * W and coop == 0 and in_loop == (W - 1, 2), key      # the last trip of a multi-round loop
    assert ROWS["ragged-last-round-13"] % 16 == 13 and ROWS["ragged-last-round-1"] % 16 == 1
    ntiles, trips, in_loop, coop, ragged = split(ROWS["no-ragged-tile"])
    assert ntiles == 24 and trips == [3] * W and coop == 0 and ragged is None
    ntiles, trips, in_loop, coop, ragged = split(ROWS["ragged-coop-tile"])
    assert ntiles == 25 and trips == [3] * W and coop == 1 and ragged == 24 and in_loop is None   # tile 24 = main_end + workgroup 0
    ntiles, trips, in_loop, coop, ragged = split(ROWS["one-trip-one-coop"])
    assert ntiles == 9 and trips == [1] * W and coop == 1 and in_loop is None                     # no wave has a next trip
    ntiles, trips, in_loop, coop, ragged = split(ROWS["one-trip-two-coops"])
    assert ntiles == 11 and trips == [1] * W and coop == 2 and in_loop is None
    ntiles, trips, in_loop, coop, ragged = split(ROWS["seventeen-rows"])
    assert ntiles == 2 and trips == [0] * W and coop == 1 and ragged == 1                         # workgroup 1's cooperative tile: one row
    ntiles, trips, in_loop, coop, ragged = split(ROWS["ragged-first-trip"])
    assert ntiles == 6 and trips == [1] * 6 + [0] * 2 and coop == 0 and in_loop == (5, 0)         # the prologue's rows, a single trip
    # the plain extra round (tests/test_gpu_narrow_prologue.py: 21 tiles) is where the ragged tile falls on a wave's extra trip
    ntiles, trips, in_loop, coop, ragged = split(16 * 21 - 3)
    assert trips == [3] * 5 + [2] * 3 and in_loop == (4, 2) and coop == 0


def check(native, spec, X, Y, theta, eta):
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
    print(f"{name} {X.shape[0]} rows: logp {e_lp:.2e} ({LOGP_RTOL}) gradient per tensor {e_g:.2e} ({GRAD_TOL}) forward {e_f:.2e} ({FWD_TOL})")
    assert e_lp <= LOGP_RTOL, f"{name}: logp {lp} against {lp64} ({e_lp:.2e} relative)"
    assert e_g <= GRAD_TOL, f"{name}: gradient {e_g:.3e} of a tensor's inf-norm"
    assert e_f <= FWD_TOL, f"{name}: forward {e_f:.3e}"


@pytest.mark.parametrize("shape,rows", CASES, ids=[f"{s}-{r}" for s, r in CASES])
def test_value_gradient_forward(native, monkeypatch, shape, rows):
    monkeypatch.setenv("TBNN_FAST_GRID", str(GRID))
    dims, n = SHAPES[shape], ROWS[rows]
    spec, X, Y, theta, eta = problem(dims, n, acts=[o.ACT_RELU] * (len(dims) - 2), seed=len(dims) + n)
    check(native, spec, X, Y, theta, eta)


def test_two_chain_group_is_the_solo_chains(native, monkeypatch):
    """gridDim.y = 2 at 24 tiles with a ragged last tile, on the per-step kernels: each chain's transition bit for bit the solo chain's"""
    monkeypatch.setenv("TBNN_FAST_GRID", str(GRID))
    monkeypatch.setenv("TBNN_TRAJ", "0")
    dims, n = SHAPES["5-50-50-50-1"], ROWS["ragged-last-round-13"]
    spec, X, Y, theta, eta = problem(dims, n, acts=[o.ACT_RELU] * (len(dims) - 2), seed=11)
    nc, c0, seed = 2, 3, 50
    rng = np.random.default_rng(4)
    thetas = (theta[None, :] * (1.0 + 0.05 * rng.standard_normal((nc, theta.size)))).astype(np.float32)
    etas = np.tile(eta, (nc, 1)).astype(np.float32) * (1.0 + 0.01 * np.arange(nc, dtype=np.float32))[:, None]
    keys = ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new")
    grp = native.ChainGroup(layers_of(spec), nc, likelihood=spec.likelihood, seed=seed, chain_id=c0, jit=False)
    try:
        assert "fast3" in grp.kernel_name, grp.kernel_name
        grp.set_data(X, Y); grp.set_state(thetas); grp.set_hypers(etas)
        got = grp.hmc_step(2e-5, 4)
        assert grp.last_transition_path == "per-step", grp.last_transition_path
        g_state = grp.get_state()
    finally:
        grp.close()
    for c in range(nc):
        ch = native.Chain(layers_of(spec), likelihood=spec.likelihood, seed=seed, chain_id=c0 + c, jit=False)
        try:
            ch.set_data(X, Y); ch.set_state(thetas[c]); ch.set_hypers(etas[c])
            want = ch.hmc_step(2e-5, 4)
            assert [got[c][k] for k in keys] == [want[k] for k in keys], (c, got[c], want)
            np.testing.assert_array_equal(g_state[c], ch.get_state())
        finally:
            ch.close()
    assert np.abs(g_state[0] - g_state[1]).max() > 0
