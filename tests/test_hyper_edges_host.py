"""CPU: the yardstick of tests/test_gpu_hyper_edges.py judged before any device is.  The Python restatement of the hyper kernel's wave plan
holds the facts the GPU module relies on; the fp32 oracle sits inside every band at every edge of tests/hyper_edges.py (a case whose fp32
oracle leaves a band is a wrong case, not a wrong band); and every band refuses the mistake it is there for."""
import numpy as np
import pytest

import hyper_edges as he
import tbnn_oracle as o
from tensor_checks import tensor_err

DIMS, ROWS, L = [4, 16, 16, 1], 257, 9
FAMILIES = ["cauchy", "gaussian"]
TARGET_CASES = [(f, d) for f in FAMILIES + ["mix"] for d in (1, 2)]      # the hyper target of the GPU module: two output counts, the mix
STEP_EDGES = he.WEIGHT_STEP_EDGES + he.HANDOVER_EDGES[1:]        # every eta the GPU module starts a weight transition under


# ---------------------------------------------------------------- the wave plan
def test_plan_at_the_register_limit():
    plan, folded = he.hyper_plan(he.PLAN_SHAPES["held_at_limit"])
    assert folded == [] and plan[0]["waves"] == 13 and plan[0]["shares"] == [1280] * 13 and plan[0]["held"] == 13 and plan[0]["reread"] == 0
    assert [p["waves"] for p in plan[1:]] == [1, 1, 1]
    plan, folded = he.hyper_plan(he.PLAN_SHAPES["mixed_paths"])
    assert folded == [] and plan[0]["waves"] == 13 and sorted(plan[0]["shares"]) == [1280] * 12 + [1281]
    assert plan[0]["held"] == 12 and plan[0]["reread"] == 1
    plan, folded = he.hyper_plan(he.PLAN_SHAPES["sixteen_groups"])
    assert folded == [] and len(plan) == 16 and all(p["waves"] == 1 for p in plan)
    by_size = {p["shares"][0]: p for p in plan}
    assert by_size[1280]["held"] == 1 and by_size[1281]["reread"] == 1 and by_size[1952]["reread"] == 1
    plan, folded = he.hyper_plan(he.PLAN_SHAPES["folded"])
    assert folded == [15, 16, 17] and all(p["waves"] == 1 for p in plan[:15]) and all(p["waves"] == 0 for p in plan[15:])
    plan, folded = he.hyper_plan(he.PLAN_SHAPES["empty_waves"])
    assert folded == [] and plan[0]["waves"] == 11 and plan[0]["empty"] == 8 and plan[0]["held"] == 3
    assert sum(p["waves"] for p in plan) == he.HYP_WAVES


def test_plan_restatement_on_the_depth_modules_shapes():
    """tests/test_gpu_depth.py: no fold at 8 layers, groups 15 .. folded from 9 layers on, the wide family's 64 x 64 groups re-read"""
    import test_gpu_depth as d
    for dims in d.EIGHT.values():
        plan, folded = he.hyper_plan(dims)
        assert folded == [] and all(p["waves"] == 1 for p in plan)
    for dims in list(d.NINE.values()) + [d.DEEP[f] for f in ("mid", "wide", "layered")]:
        plan, folded = he.hyper_plan(dims)
        assert folded == list(range(15, 2 * (len(dims) - 1))) and sum(p["waves"] for p in plan) == 15
    for dims in (d.EIGHT["wide"], d.NINE["wide"]):
        plan, _ = he.hyper_plan(dims)
        assert all(p["reread"] == 1 for p, c in zip(plan, he.group_sizes(dims)) if c == 64 * 64 and p["waves"])
    for dims in he.PLAN_SHAPES.values():                            # every share of every shape adds up to its group
        plan, folded = he.hyper_plan(dims)
        assert all(sum(p["shares"]) == c for g, (p, c) in enumerate(zip(plan, he.group_sizes(dims))) if g not in folded)


# ---------------------------------------------------------------- the fp32 oracle inside the bands
def _case(family, edge, dims=DIMS):
    spec, X, Y, theta, eta0 = he.small_problem(dims, ROWS, family)
    return spec, X, Y, theta, he.eta_at(edge, spec, eta0, theta, X, Y)


@pytest.mark.parametrize("edge", list(he.ETA_EDGES))
@pytest.mark.parametrize("family,d_out", TARGET_CASES)
def test_fp32_oracle_meets_the_target_bands(family, d_out, edge):
    spec, X, Y, theta, eta = _case(family, edge, DIMS[:-1] + [d_out])
    with np.errstate(all="ignore"):
        lp32, g32 = o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float32)
        r_v, r_g = he.check_hyper_target(float(lp32), g32, spec, eta, theta, X, Y, (family, edge))
        wl64, wg64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)
        wl32, wg32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)
    e_lp = abs(float(wl32) - wl64) / max(abs(wl64), 1.0)
    e_g = tensor_err(spec, wg32, wg64, 1e-30)
    print(f"{family} d_out {d_out} {edge}: hyper value {r_v:.2e} gradient {r_g:.2e} of their bands; weight target {e_lp:.2e} ({he.LOGP_RTOL}) "
          f"gradient per tensor {e_g:.2e} ({he.GRAD_TOL})")
    assert e_lp <= he.LOGP_RTOL and e_g <= he.GRAD_TOL, (e_lp, e_g)


@pytest.mark.parametrize("edge", he.HYPER_STEP_EDGES)
@pytest.mark.parametrize("family", FAMILIES)
def test_fp32_oracle_meets_the_hyper_transition_bands(family, edge):
    spec, X, Y, theta, eta = _case(family, edge)
    ph = he.momenta(spec)[1]
    eps = he.pick_eps((family, edge, tuple(DIMS)), "hyper", spec, eta, theta, X, Y, L, ph)
    lp64 = float(o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64)[0])
    with np.errstate(all="ignore"):
        r64 = o.hyper_step(spec, eta, theta, X, Y, eps, L, ph, -1e30, np.float64)
        r32 = o.hyper_step(spec, eta, theta, X, Y, eps, L, ph, -1e30, np.float32, energy_dtype=np.float64)
    assert r64.accepted and r32.accepted and np.isfinite(r64.log_accept_ratio)
    d_lar = abs(r32.log_accept_ratio - r64.log_accept_ratio)
    e_eta = float(np.max(np.abs(r32.theta - r64.theta) / np.abs(r64.theta)))
    print(f"{family} {edge}: eps {eps:.3g} lar {r64.log_accept_ratio:.4g} |d lar| {d_lar:.2e} ({he.lar_band(r64.log_accept_ratio, lp64):.2e}) "
          f"eta {e_eta:.2e} (1e-4)")
    assert d_lar <= he.lar_band(r64.log_accept_ratio, lp64)
    assert e_eta <= 1e-4


@pytest.mark.parametrize("edge", STEP_EDGES)
@pytest.mark.parametrize("family", FAMILIES)
def test_fp32_oracle_meets_the_weight_transition_bands(family, edge):
    spec, X, Y, theta, eta = _case(family, edge)
    p0 = he.momenta(spec)[0]
    eps = he.pick_eps((family, edge, tuple(DIMS)), "weight", spec, eta, theta, X, Y, 3, p0)
    lp64 = float(o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[0])
    r64 = o.weight_step(spec, theta, eta, X, Y, eps, 3, p0, -1e30, np.float64)
    r32 = o.weight_step(spec, theta, eta, X, Y, eps, 3, p0, -1e30, np.float32, energy_dtype=np.float64)
    e_tr = float(np.max(np.abs(np.asarray(r32.trace_logp) - r64.trace_logp) / np.maximum(np.abs(r64.trace_logp), 1.0)))
    d_lar = abs(r32.log_accept_ratio - r64.log_accept_ratio)
    e_q = float(np.abs(r32.theta - r64.theta).max() / max(1.0, np.abs(r64.theta).max()))
    print(f"{family} {edge}: eps {eps:.3g} trace {e_tr:.2e} ({he.LOGP_RTOL}) |d lar| {d_lar:.2e} "
          f"({he.lar_band(r64.log_accept_ratio, lp64):.2e}) state {e_q:.2e} (1e-5)")
    assert e_tr <= he.LOGP_RTOL and d_lar <= he.lar_band(r64.log_accept_ratio, lp64) and e_q <= 1e-5


# ---------------------------------------------------------------- every band refuses what it is there for
def _target64(family, edge):
    spec, X, Y, theta, eta = _case(family, edge)
    lp64, g64 = o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64)
    return spec, X, Y, theta, eta, float(lp64), np.array(g64)


@pytest.mark.parametrize("edge", ["default", "tiny", "sd_small", "sd_mle"])
def test_the_gradient_band_refuses_one_entry_off_by_a_thousandth(edge):
    spec, X, Y, theta, eta, lp64, g64 = _target64("cauchy", edge)
    he.check_hyper_target(lp64, g64, spec, eta, theta, X, Y)
    for j in range(g64.size):
        if edge == "sd_mle" and j == g64.size - 1:
            continue                                               # (the entry that cancels: its band is the size of its two terms)
        bad = g64.copy()
        bad[j] *= 1.0 + 1e-3
        with pytest.raises(AssertionError, match="hyper gradient"):
            he.check_hyper_target(lp64, bad, spec, eta, theta, X, Y)


def test_the_gradient_band_refuses_a_cancelling_entry_off_by_a_thousandth_of_a_term():
    """at sd_mle the data entry is the difference of -n/s and S/s^3: an error of 1e-3 of one of them is far outside the band"""
    spec, X, Y, theta, eta, lp64, g64 = _target64("cauchy", "sd_mle")
    T = he.hyper_grad_terms(spec, eta, theta, X, Y)
    assert abs(g64[-1]) < 1e-4 * T[-1]
    bad = g64.copy()
    bad[-1] += 1e-3 * T[-1] / 2
    with pytest.raises(AssertionError, match="hyper gradient"):
        he.check_hyper_target(lp64, bad, spec, eta, theta, X, Y)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_gradient_band_refuses_the_sign_of_a_positive_g(family):
    spec, X, Y, theta, eta, lp64, g64 = _target64(family, "neg_g")
    bad = g64.copy()
    bad[1::2][: 2 * len(spec.layers)] *= -1.0                      # the chain rule's 2 g taken as 2 |g|
    bad[-1] *= -1.0
    assert np.all(g64[1::2] != 0.0)
    with pytest.raises(AssertionError, match="hyper gradient"):
        he.check_hyper_target(lp64, bad, spec, eta, theta, X, Y)
    for j in list(range(1, 4 * len(spec.layers), 2)) + [g64.size - 1]:
        one = g64.copy()
        one[j] *= -1.0
        with pytest.raises(AssertionError, match="hyper gradient"):
            he.check_hyper_target(lp64, one, spec, eta, theta, X, Y)


@pytest.mark.parametrize("edge", ["clamp_lo", "sd_clamp_lo", "sd_clamp_hi"])
def test_the_bands_refuse_a_gradient_where_the_clamp_makes_it_zero(edge):
    """the unclamped formula's value in a clamped entry: -1/s + sum d^2 / s^3 for a Gaussian scale, -n/s + S/s^3 for the data sd"""
    spec, X, Y, theta, eta, lp64, g64 = _target64("gaussian", edge)
    he.check_hyper_target(lp64, g64, spec, eta, theta, X, Y)
    clamped = he.clamped_entries(spec, eta)
    assert clamped
    S, n_el = he.residual_ss(spec, theta, X, Y)
    parts = o.unflatten(spec, theta.astype(np.float64))
    for j in clamped:
        gg = float(eta[j])
        s = min(max(gg * gg, 1e-8), 1e8)
        if j == g64.size - 1:
            leak = (-n_el / s + S / s ** 3) * 2.0 * gg
        else:
            x = parts[j // 4][0 if j % 4 == 1 else 1]
            leak = (-1.0 / s + np.sum((x - float(eta[j - 1])) ** 2) / s ** 3) * 2.0 * gg
        assert leak != 0.0
        bad = g64.copy()
        bad[j] += leak
        with pytest.raises(AssertionError, match="hyper gradient|clamped entry"):
            he.check_hyper_target(lp64, bad, spec, eta, theta, X, Y)
    # and the smallest non-zero fp32 number in the data term's clamped entry
    if g64.size - 1 in clamped:
        bad = g64.copy()
        bad[-1] = 1e-30
        with pytest.raises(AssertionError, match="hyper gradient"):
            he.check_hyper_target(lp64, bad, spec, eta, theta, X, Y)


def test_the_value_and_transition_bands_refuse_a_thousandth():
    spec, X, Y, theta, eta, lp64, g64 = _target64("cauchy", "small")
    with pytest.raises(AssertionError, match="hyper value"):
        he.check_hyper_target(lp64 * (1.0 + 1e-3), g64, spec, eta, theta, X, Y)
    assert abs(lp64) * 1e-3 > he.lar_band(0.0, lp64)               # an energy off by a thousandth leaves the log-accept-ratio band
