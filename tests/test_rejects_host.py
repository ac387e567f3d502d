"""CPU: the plans of the reject tests (tests/rejects.py), judged on the oracle alone, in its fp32 arm (energies in fp64, as the device sums
them) and in its fp64 arm, before any GPU time is spent: T0's proposal is finite; T2's decision is no coin toss; the huge step is finite
and rejected on its merits; the non-finite steps (weights and hypers) are not finite and rejected at -inf; every epoch of the free-running
middle run is a reject.  And the table itself: every family and both transition ends, the Gaussian, Bernoulli, Poisson, Student-t,
negative-binomial and heteroscedastic likelihoods, row weights on a narrow and a mid case, and no run-time
library that an existing module does not compile."""
import numpy as np
import pytest

import rejects as rj
import tbnn_oracle as o

ARMS = {"fp32": np.float32, "fp64": np.float64}
FLT_MAX = float(np.finfo(np.float32).max)


def test_the_table_fills_the_cells():
    cells = {(c.family, c.path) for c in rj.CASES}
    for fam in ("fast3", "fast", "mid", "tall", "wide", "layered", "generic"):
        assert (fam, "per-step") in cells, fam
    assert ("fast3", "trajectory") in cells
    by = rj.BY_ID
    # the unmerged end: more than 32,768 parameters at a few hundred rows, and a narrow case that asks for it
    assert rj.problem(by["wide-unmerged-big-p"])[0].n_params > 32768 and rj.problem(by["wide-unmerged-big-p"])[1].shape[0] <= 1000
    assert by["fast3-unmerged-end"].env["TBNN_MERGE_ENDS"] == "0"
    # the narrow per-step cases keep the trajectory kernel's 1,000 rows and switch it off; the trajectory case fits its 1,200-row limit
    assert by["fast3"].env["TBNN_TRAJ"] == "0" and by["fast3-trajectory"].env["TBNN_TRAJ"] == "1" and rj.problem(by["fast3-trajectory"])[1].shape[0] <= 1200
    liks = [rj.problem(c)[0].likelihood for c in rj.CASES]
    for lik in (o.LIK_BERNOULLI, o.LIK_POISSON, o.LIK_STUDENT_T, o.LIK_NEG_BINOMIAL):
        assert liks.count(lik) == 1, lik
    gauss_families = {c.family for c in rj.CASES if rj.problem(c)[0].likelihood == o.LIK_GAUSSIAN and rj.weights(c) is None}
    assert gauss_families == {"fast3", "fast", "mid", "tall", "wide", "layered", "generic"}
    hetero = {c.family for c in rj.CASES if rj.problem(c)[0].likelihood == o.LIK_HETERO_GAUSSIAN}
    assert hetero == {"fast3", "mid"} and all(rj.problem(c)[0].layers[-1].out_dim == 2 for c in rj.CASES if c.id.endswith("hetero"))
    assert {c.family for c in rj.CASES if rj.weights(c) is not None} == {"fast3", "mid"}
    for c in rj.CASES:
        spec, X, _Y, _theta, _eta = rj.problem(c)
        assert X.shape[0] <= 1000 and spec.n_hypers > 0, c.id              # (every case has hypers: no disturbance is left out anywhere)
    assert set(rj.GROUP_CASES) <= set(by) and {by[k].family for k in rj.GROUP_CASES} == {"fast3", "mid", "tall", "wide"}
    assert {by[k].path for k in rj.GROUP_CASES} == {"per-step", "trajectory"}


def test_every_library_is_one_an_existing_module_compiles():
    own = rj.mt.owners_jobs()
    jobs = rj.jit_jobs()
    assert jobs and all(j in own for j in jobs), [j for j in jobs if j not in own]


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("cid", list(rj.BY_ID))
def test_plan(cid, arm):
    c = rj.BY_ID[cid]
    p = rj.plan(c, ARMS[arm])
    print(f"[rejects] {cid} {arm}: T0 lar {p.t0.log_accept_ratio:.4g}; T2 lar {p.t2.log_accept_ratio:.4g}; huge lar {p.huge.log_accept_ratio:.4g} "
          f"(logp {p.huge.logp_new:.4g}); non-finite logp {p.nan.logp_new} lar {p.nan.log_accept_ratio}; hyper non-finite logp "
          f"{p.hyper_nan.logp_new} lar {p.hyper_nan.log_accept_ratio}; hyper lar {p.hyper_ok.log_accept_ratio:.4g}; T2 after it "
          f"{p.t2_after_hyper.log_accept_ratio:.4g}")
    # T0: a sane, accepted transition
    assert rj.finite(p.t0.theta_proposed) and np.isfinite(p.t0.log_accept_ratio) and p.t0.accepted
    assert np.abs(p.t0.theta - rj.problem(c)[3]).max() > 0
    # T2, and T2 after the accepted hyper step: finite, and the decision has its margin
    for t2 in (p.t2, p.t2_after_hyper):
        assert np.isfinite(t2.log_accept_ratio) and abs(t2.log_accept_ratio - rj.LOG_HALF) > rj.MARGIN, (cid, t2.log_accept_ratio)
        assert rj.finite(t2.trace_logp) and rj.finite(t2.theta_proposed)
    # the bands of the device's anchor (tests/test_gpu_parity.py: test_hmc_step_injected) are a fair demand at these problems: the oracle's
    # own fp32 arm is inside half of them (what rejects._sigma_one is for)
    if arm == "fp32":
        r64 = rj.plan(c, np.float64)
        for a, b in ((p.t2, r64.t2), (p.t2_after_hyper, r64.t2_after_hyper)):
            e_lar = abs(a.log_accept_ratio - b.log_accept_ratio) / (2e-2 + 1e-4 * abs(b.log_accept_ratio))
            e_tr = float(np.max(np.abs(np.asarray(a.trace_logp) - b.trace_logp) / (4e-6 * np.abs(b.trace_logp) + 2e-3)))
            print(f"[rejects] {cid}: the fp32 arm over the anchor's bands: log accept ratio {e_lar:.3f}, trace {e_tr:.3f}")
            assert e_lar <= 0.5 and e_tr <= 0.5, (cid, e_lar, e_tr)
    # the forced reject is a sane transition
    assert np.isfinite(p.forced.log_accept_ratio) and not p.forced.accepted
    # huge and finite: rejected on its merits, and the ratio fits the fp32 field of the record
    assert np.isfinite(p.huge.log_accept_ratio) and -1e-3 * FLT_MAX < p.huge.log_accept_ratio < -1e3, (cid, p.huge.log_accept_ratio)
    assert np.isfinite(p.huge.logp_new) and rj.finite(p.huge.theta_proposed) and not p.huge.accepted
    # not finite: weights and hypers
    for r in (p.nan, p.hyper_nan):
        assert not np.isfinite(r.logp_new) and rj.is_minus_inf(r.log_accept_ratio) and not r.accepted, (cid, r.logp_new, r.log_accept_ratio)
    np.testing.assert_array_equal(p.nan.theta, p.t0.theta)
    np.testing.assert_array_equal(p.hyper_nan.theta, np.asarray(rj.problem(c)[4], ARMS[arm]))
    # the sane hyper step moves eta
    assert p.hyper_ok.accepted and rj.finite(p.hyper_ok.theta) and np.abs(p.hyper_ok.theta - rj.problem(c)[4]).max() > 0


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("cid", list(rj.BY_ID))
def test_free_running_middle_epochs_are_rejects(cid, arm):
    run = rj.free_run(rj.BY_ID[cid], ARMS[arm])
    print(f"[rejects] {cid} {arm}: free-running lar {[r.log_accept_ratio for r in run]} accepted {[r.accepted for r in run]}")
    assert all(np.isfinite(r.log_accept_ratio) for r in run[:2])
    assert all(rj.is_minus_inf(r.log_accept_ratio) and not r.accepted for r in run[2:])
