"""CPU: the case table of the many-tiles tests (tests/many_tiles.py).  The row counts reach the trips, the ragged tile and the cooperative
rounds they are meant for, by the kernels' plans restated; the oracle's fp32 arm stays inside HALF of every band of
tests/test_gpu_many_tiles.py on every case, so the bands are a fair demand on an fp32 kernel at these problems; and every run-time library
the device module loads is one an existing module compiles."""
import numpy as np
import pytest

import many_tiles as mt
import tbnn_oracle as o


def test_narrow_row_counts_reach_every_case():
    W = 4 * mt.GRID
    ntiles, trips, in_loop, coop, ragged = mt.split(mt.NARROW_ROWS["ragged-last-trip"], mt.GRID)
    assert ntiles == 24 and trips == [3] * W and coop == 0 and in_loop == (W - 1, 2)            # three trips per wave, ragged last trip
    ntiles, trips, in_loop, coop, ragged = mt.split(mt.NARROW_ROWS["ragged-coop-tile"], mt.GRID)
    assert ntiles == 25 and trips == [3] * W and coop == 1 and ragged == 24 and in_loop is None  # the ragged tile is the cooperative tile
    ntiles, trips, in_loop, coop, ragged = mt.split(mt.NARROW_ROWS["two-coop-rounds"], mt.GRID)
    assert ntiles == 11 and trips == [1] * W and coop == 2 and ragged == 10 and in_loop is None  # one trip, two cooperative rounds
    ntiles, trips, in_loop, coop, ragged = mt.split(mt.NARROW_ROWS["uneven-trips"], mt.GRID)
    assert ntiles == 21 and trips == [3] * 5 + [2] * 3 and coop == 0 and in_loop == (4, 2)       # the ragged tile on an extra trip
    assert all(n % 16 for n in mt.NARROW_ROWS.values())


def test_mid_row_counts_reach_every_case():
    W = 4 * mt.GRID
    plans = {k: mt.mid_plan(n) for k, n in mt.MID_ROWS.items()}
    assert plans["ragged-last-trip"] == ([3] * W, (W - 1, 2), [])
    assert plans["uneven-trips"] == ([3] * 5 + [2] * 3, (4, 2), [5, 6, 7])      # waves 5 .. 7: tile + W past ntiles while 0 .. 4 go on
    assert plans["no-ragged-tile"] == ([3] * W, None, [])
    assert any(max(t) >= 3 for t, _r, _e in plans.values()) and any(r is not None and r[1] >= 1 for _t, r, _e in plans.values())
    assert any(e for _t, _r, e in plans.values())


def test_tall_row_count_walks_groups():
    g, ngroups, per_wg, last_rows = mt.tall_plan(mt.TALL_ROWS)
    print(f"tall: {mt.TALL_ROWS} rows: groups of {g} tile(s), {ngroups} groups, per workgroup {per_wg}, the last group {last_rows} rows")
    assert len(per_wg) == mt.TALL_GRID and min(per_wg) >= 2           # every workgroup walks at least two groups
    assert 0 < last_rows < 16 * g                                     # the last group is partial


def test_the_table_fills_the_cells():
    cells = {(c.family, c.path, c.lik, c.weighted) for c in mt.CASES}
    for fam in ("fast3", "fast"):
        for lik in ("gaussian", "bernoulli", "poisson", "student", "negbin", "hetero", "gamma"):
            assert any(f == fam and l == lik and not w for f, _p, l, w in cells), (fam, lik)
    for lik in ("gaussian", "bernoulli", "poisson", "student", "negbin", "hetero", "gamma"):
        assert any(f == "fast3" and l == lik and w for f, _p, l, w in cells), lik
    assert ("fast3", "valu2", "student", False) in cells and ("fast", "valu2", "gaussian", True) in cells and ("fast", "valu2", "bernoulli", True) in cells
    for lik in ("student", "negbin", "poisson", "hetero", "bernoulli", "gamma"):
        assert any(f == "mid" and p.startswith("valu") and l == lik for f, p, l, _w in cells), lik
    for lik in ("gaussian", "bernoulli", "categorical", "poisson", "student", "negbin", "gamma"):
        assert ("mid", "mfma10", lik, False) in cells, lik
    for lik in ("gaussian", "categorical"):
        assert ("mid", "mfma10", lik, True) in cells and ("wide", "mfma10", lik, True) in cells, lik
    assert {("tall", "valu1", "gaussian", True), ("tall", "valu1", "poisson", False), ("tall", "mfma10", "categorical", True)} <= cells
    # Gamma: every fused family, both narrow output counts, and its three weighted libraries (fast3, fast, the MFMA output tile of mid)
    assert {("fast3", "valu1", "gamma", True), ("fast3", "valu2", "gamma", False), ("fast", "valu1", "gamma", True), ("mid", "mfma10", "gamma", True),
            ("tall", "valu1", "gamma", False), ("wide", "valu1", "gamma", False), ("wide", "mfma10", "gamma", False)} <= cells
    assert any(c.zero_ragged and c.lik == "gamma" and c.family == "fast" and c.rows == 381 for c in mt.CASES)
    assert sum(c.zero_ragged for c in mt.CASES) >= 1
    for c in mt.CASES:
        rows = {"wide": [mt.N_WIDE], "tall": [mt.TALL_ROWS], "mid": list(mt.MID_ROWS.values())}.get(c.family, list(mt.NARROW_ROWS.values()))
        assert c.rows in rows and c.grid == {"wide": None, "tall": mt.TALL_GRID}.get(c.family, mt.GRID)
        if c.zero_ragged:
            w = mt.weights(c)
            assert c.weighted and np.all(w[c.rows - c.rows % 16:] == 0) and np.any(w[:c.rows - c.rows % 16] > 0)


def test_every_library_is_one_an_existing_module_compiles():
    own = mt.owners_jobs()
    jobs = mt.jit_jobs()
    assert jobs and all(j in own for j in jobs), [j for j in jobs if j not in own]


@pytest.mark.parametrize("cid", list(mt.BY_ID))
def test_fp32_arm_inside_half_a_band(cid):
    """the oracle's own formula in fp32 against fp64, with the case's weights and without them: value, gradient per tensor, statistic"""
    c = mt.BY_ID[cid]
    spec, X, Y, theta, eta = mt.problem(c)
    for weighted in ((True, False) if c.weighted else (False,)):
        w = mt.weights(c) if weighted else None
        lp32, g32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32, w=w)
        st32 = mt.statistic(spec, theta, eta, X, Y, np.float32, w)
        ev, eg, es = mt.gaps(c, spec, float(lp32), g32, st32, mt.ref64(c, weighted))
        print(f"[many-tiles] {cid}{' (weights)' if weighted else ''}: fp32 arm over the band: value {ev:.3f} gradient {eg:.3f} statistic {es:.3f}")
        assert np.isfinite(lp32) and np.all(np.isfinite(g32))
        assert ev <= 0.5 and eg <= 0.5 and es <= 0.5, (cid, weighted, ev, eg, es)
