"""GPU: a rejected or diverged transition leaves the chain untouched -- the cases, disturbances and draws of tests/rejects.py (which says why;
tests/test_rejects_host.py judges the plans on the oracle alone).

Per case (a kernel family and a transition end; the kernel's name and the path of the transitions are asserted) and disturbance:

    baseline   a fresh handle, T0 (accepted), T2 (log u = log 0.5; traced on the per-step paths)
    disturbed  a fresh handle, T0, the disturbance, T2

Straight after the disturbance the state, the hypers, logp_grad() and predict(0) at the chain's own state are what they were before it, bit
for bit; T2's record, its trace, and the state, the hypers and the momentum after it are the baseline's, bit for bit, and T2's logp_old is
T0's logp_new.  Nothing compared is NaN (asserted), so assert_array_equal needs no NaN == NaN.  No path re-orders a sum between the two
runs: a disturbance may drop an image, which k_make_image rebuilds as a copy.  The last disturbance (a non-finite weight step, then an
ACCEPTED hyper step) has the baseline T0, the same hyper step, T2: EN_REFRESH and k_refresh_grad_after_hyper read the cached statistic and
gd_cur while h->pstat holds a diverged proposal's.

So that both runs equally wrong cannot pass, T2 of either baseline is judged against o.weight_step in fp64 from the state (and hypers) the
device holds before it, at the bands of tests/test_gpu_parity.py: test_hmc_step_injected (per-step: trace 4e-6 relative + 2e-3, log accept
ratio 2e-2 + 1e-4 |lar|, the decision where the oracle's margin exceeds 0.1 -- it does in every case, by the host module -- the state 2e-5
of max(1, |theta|_inf), the squared jump 1e-3, the accept probability 2e-2) and of tests/test_gpu_traj.py (trajectory: the log accept
ratio's band with its 4e-7 |logp| term, the decision, the state to rtol 2e-5, atol 2e-6).

A free-running variant per case (the middle hmc_run replaced by set_epoch) and chain groups of three in which chain 1 diverges, in its
weight transitions and in its hyper transition, while chains 0 and 2 must not notice."""
import numpy as np
import pytest

import rejects as rj
import tbnn_oracle as o
from tensor_checks import layers_of

pytestmark = pytest.mark.gpu

ENV = ("TBNN_TRAJ", "TBNN_MERGE_ENDS", "TBNN_MID", "TBNN_TALL", "TBNN_REGISTERED", "TBNN_JIT_SKIP", "TBNN_FAST_GRID", "TBNN_HYPER_FULL_REFRESH")
IDS = list(rj.BY_ID)


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """this module's run-time shapes, before any test touches the GPU (the libraries of the modules that own the shapes: cached, a second
    run compiles nothing)"""
    from tensorbnn_amd import jit
    jobs = rj.jit_jobs()
    assert jit.prebuild(jobs, processes=16) == len(jobs)


_OPEN = []


@pytest.fixture(autouse=True)
def close_handles():
    """every handle a test opened is destroyed when it ends, passed or failed"""
    yield
    while _OPEN:
        _OPEN.pop().close()


def open_handle(native, monkeypatch, c, n_chains=None, **kw):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in rj.env_of(c).items():
        monkeypatch.setenv(k, v)
    spec = rj.problem(c)[0]
    kw = dict(likelihood=spec.likelihood, fixed_sd=spec.fixed_sd, lik_df=spec.lik_df, jit=rj.jit_of(c),
              kernel=native.KERNEL_GENERIC if c.family == "generic" else native.KERNEL_AUTO, **kw)
    h = native.Chain(layers_of(spec), **kw) if n_chains is None else native.ChainGroup(layers_of(spec), n_chains, **kw)
    _OPEN.append(h)
    return h


def stage(h, c, theta=None):
    """the case's rows (and row weights) and start state on a fresh handle; the kernel's name"""
    _spec, X, Y, theta0, eta = rj.problem(c)
    h.set_data(X, Y)
    w = rj.weights(c)
    if w is not None:
        h.set_row_weights(w)
    assert rj.kernel_ok(c, h.kernel_name), (c.id, h.kernel_name)
    h.set_state(theta0 if theta is None else theta)
    h.set_hypers(eta)
    assert h.last_transition_path == "none"


def rec(r):
    return np.array([r[k] for k in rj.REC], dtype=np.float64)


def start(native, monkeypatch, c):
    """a fresh handle after T0: the cache at the current state was made by a commit, not by the bootstrap evaluation"""
    ch = open_handle(native, monkeypatch, c)
    stage(ch, c)
    t0 = ch.hmc_step(c.eps, rj.L, p0=rj.momentum(c, "T0"), log_u=-1e30)
    assert t0["accepted"] == 1 and rj.finite(rec(t0)), (c.id, t0)
    assert ch.last_transition_path == c.path, (c.id, ch.last_transition_path)
    return ch, t0


def snapshot(ch):
    """what the chain shows of its current state: the state, the hypers, logp_grad() and predict(0) at its own state"""
    lp, g, st = ch.logp_grad()
    snap = {"state": ch.get_state(), "hypers": ch.get_hypers(), "logp": np.array([lp, st]), "grad": g, "predict": ch.predict(0)}
    assert all(rj.finite(v) for v in snap.values())
    return snap


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def t2(ch, c):
    """T2 from EPOCH: its record, its trace on the per-step paths, and the state, the hypers and the momentum it leaves"""
    ch.set_epoch(rj.EPOCH)
    traced = c.path == "per-step"
    out = ch.hmc_step(c.eps, rj.L, p0=rj.momentum(c, "T2"), log_u=rj.LOG_HALF, trace=traced)
    assert ch.last_transition_path == c.path, (c.id, ch.last_transition_path)
    end = {"record": rec(out), "state": ch.get_state(), "hypers": ch.get_hypers(), "momentum": ch.debug_momentum()}
    if traced:
        end["trace"] = np.asarray(out["trace_logp"]).copy()
    assert all(rj.finite(v) for v in end.values()), (c.id, out)
    return out, end


def hyper_ok(ch, c):
    out = ch.hyper_step(rj.EPS_H, rj.L_H, p0=rj.momentum(c, "H"), log_u=-1e30)
    assert out["accepted"] == 1 and rj.finite(rec(out)), (c.id, out)
    return out


_BASE = {}


def baseline(native, monkeypatch, c, hyper):
    """the baseline run of a case, computed once and shared: T0, (hyper: the accepted hyper step,) T2"""
    key = (c.id, hyper)
    if key not in _BASE:
        ch, t0 = start(native, monkeypatch, c)
        b = {"t0": t0, "before": snapshot(ch)}
        if hyper:
            b["hyper"] = hyper_ok(ch, c)
            b["after_hyper"] = snapshot(ch)
            assert np.abs(b["after_hyper"]["hypers"] - b["before"]["hypers"]).max() > 0
        b["t2"], b["end"] = t2(ch, c)
        for v in list(b["before"].values()) + list(b["end"].values()) + list(b.get("after_hyper", {}).values()):
            v.setflags(write=False)
        _BASE[key] = b
    return _BASE[key]


# ---- the disturbances: each returns nothing and asserts its own record
def rejected_at_minus_inf(r, what):
    assert r["log_accept_ratio"] == -np.inf and r["accepted"] == 0 and r["sjd"] == 0.0 and r["accept_prob"] == 0.0, (what, r)


def forced_reject(ch, c, t0):
    r = ch.hmc_step(c.eps, rj.L, p0=rj.momentum(c, "D"), log_u=1e30)
    assert r["accepted"] == 0 and r["sjd"] == 0.0 and np.isfinite(r["log_accept_ratio"]) and np.isfinite(r["logp_new"]), (c.id, r)
    assert r["logp_old"] == t0["logp_new"]


def huge_finite(ch, c, t0):
    r = ch.hmc_step(c.eps_huge, rj.L, p0=rj.momentum(c, "D"), log_u=rj.LOG_HALF)
    print(f"[rejects] {c.id} huge-finite: lar {r['log_accept_ratio']:.6g} logp_new {r['logp_new']:.6g} kinetic_new {r['kinetic_new']:.6g}")
    assert r["accepted"] == 0 and r["sjd"] == 0.0 and np.isfinite(r["log_accept_ratio"]) and r["log_accept_ratio"] < -1e3, (c.id, r)
    assert r["logp_old"] == t0["logp_new"]


def non_finite(ch, c, t0):
    r = ch.hmc_step(rj.EPS_NAN, rj.L, p0=rj.momentum(c, "D"), log_u=rj.LOG_HALF)
    rejected_at_minus_inf(r, c.id)
    assert not np.isfinite(r["logp_new"]) or not np.isfinite(r["kinetic_new"]), (c.id, r)
    assert np.isfinite(r["logp_old"]) and r["logp_old"] == t0["logp_new"], (c.id, r)
    assert not rj.finite(ch.debug_momentum())                   # the device really holds what the next transition must not read


def queued_epochs(ch, c, t0):
    recs = ch.hmc_run(rj.EPS_NAN, rj.L, 3)                       # on the device's own draws, no host round trip between the epochs
    for r in recs:
        rejected_at_minus_inf(r, c.id)
        assert r["logp_old"] == t0["logp_new"]


def probes(ch, c, t0):
    """a probe far outside fp32's comfort (1e30 * theta: the second layer overflows) between two sane ones, which must agree"""
    _spec, _X, _Y, theta, eta = rj.problem(c)
    bad, sane = rj.theta_probes(c, theta)
    first = (ch.logp_grad(sane, eta), ch.predict(0, sane))
    lp, g, _st = ch.logp_grad(bad, eta)
    f = ch.predict(0, bad)
    print(f"[rejects] {c.id} probes: logp(theta_bad) {lp}, gradient finite {rj.finite(g)}, predictions finite {rj.finite(f)}")
    again = (ch.logp_grad(sane, eta), ch.predict(0, sane))
    assert np.isfinite(again[0][0]) and rj.finite(again[0][1]) and rj.finite(again[1])
    assert first[0][0] == again[0][0] and first[0][2] == again[0][2]
    np.testing.assert_array_equal(first[0][1], again[0][1])
    np.testing.assert_array_equal(first[1], again[1])


def diverged_hyper_step(ch, c, t0):
    before = ch.get_hypers()
    r = ch.hyper_step(rj.EPS_H_NAN, rj.L_H, p0=rj.momentum(c, "H"), log_u=rj.LOG_HALF)
    rejected_at_minus_inf(r, c.id)
    np.testing.assert_array_equal(ch.get_hypers(), before)


def non_finite_then_hyper_step(ch, c, t0):
    non_finite(ch, c, t0)
    hyper_ok(ch, c)


DISTURB = dict(zip(rj.DISTURBANCES, (forced_reject, huge_finite, non_finite, queued_epochs, probes, diverged_hyper_step, non_finite_then_hyper_step)))


@pytest.mark.parametrize("what", rj.DISTURBANCES)
@pytest.mark.parametrize("cid", IDS)
def test_disturbance_leaves_the_chain_untouched(native, monkeypatch, cid, what):
    c = rj.BY_ID[cid]
    own_baseline = what == "non-finite-then-hyper-step"
    base = baseline(native, monkeypatch, c, own_baseline)
    at = base["after_hyper" if own_baseline else "before"]
    # probed: straight after the disturbance, what the chain shows of its current state is what it showed before (after the baseline's
    # hyper step).  logp_grad() at the chain's own state leaves that state's statistic and gradient slabs behind, which could hide a T2
    # that reads them: the second handle goes from the disturbance straight to T2
    for probed in (True, False):
        ch, t0 = start(native, monkeypatch, c)
        np.testing.assert_array_equal(rec(t0), rec(base["t0"]))
        same(snapshot(ch), base["before"], "before the disturbance")
        DISTURB[what](ch, c, t0)
        if probed:
            same(snapshot(ch), at, f"{cid} after {what}")
        else:
            np.testing.assert_array_equal(ch.get_state(), at["state"])
            np.testing.assert_array_equal(ch.get_hypers(), at["hypers"])
        out, end = t2(ch, c)
        print(f"[rejects] {cid} ({ch.kernel_name}, {ch.last_transition_path}) after {what}{', probed' if probed else ''}: T2 lar "
              f"{out['log_accept_ratio']:.6g} accepted {out['accepted']}")
        same(end, base["end"], f"{cid} T2 after {what}")
        assert out["logp_old"] == (base["t2"]["logp_old"] if own_baseline else t0["logp_new"])


@pytest.mark.parametrize("hyper", [False, True], ids=["T0-T2", "T0-hyper-T2"])
@pytest.mark.parametrize("cid", IDS)
def test_baseline_against_the_oracle(native, monkeypatch, cid, hyper):
    """the independent anchor: T2 of the baseline run against o.weight_step in fp64 from what the device holds before it"""
    c = rj.BY_ID[cid]
    spec, X, Y, _theta, _eta = rj.problem(c)
    base = baseline(native, monkeypatch, c, hyper)
    at = base["after_hyper" if hyper else "before"]
    out, end = base["t2"], base["end"]
    ref = o.weight_step(spec, at["state"], at["hypers"], X, Y, c.eps, rj.L, rj.momentum(c, "T2"), rj.LOG_HALF, np.float64, w=rj.weights(c))
    margin = abs(ref.log_accept_ratio - rj.LOG_HALF)
    d_lar = abs(out["log_accept_ratio"] - ref.log_accept_ratio)
    expect = ref.theta_proposed if out["accepted"] else at["state"]
    d_q = float(np.abs(end["state"] - expect).max())
    print(f"[rejects] {cid} ({c.path}) {'after the hyper step' if hyper else ''}: lar {out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g}, margin "
          f"{margin:.3g}), |d lar| {d_lar:.3e}, state {d_q:.3e}, logp_old {out['logp_old']:.9g} (fp64 {ref.logp_old:.9g})")
    assert margin > rj.MARGIN, (cid, margin)
    assert bool(out["accepted"]) == ref.accepted
    if c.path == "trajectory":
        assert d_lar <= 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(ref.logp_old)
        np.testing.assert_allclose(end["state"], expect, rtol=2e-5, atol=2e-6)
        return
    np.testing.assert_allclose(end["trace"], np.asarray(ref.trace_logp), rtol=4e-6, atol=2e-3)
    assert d_lar <= 2e-2 + 1e-4 * abs(ref.log_accept_ratio)
    np.testing.assert_allclose(end["state"], expect, rtol=0, atol=2e-5 * max(1.0, np.abs(expect).max()))
    if out["accepted"]:
        assert abs(out["sjd"] - ref.sjd) <= 1e-3 * ref.sjd + 1e-12
    else:
        assert out["sjd"] == 0.0
    assert abs(out["accept_prob"] - ref.accept_prob) <= 2e-2


@pytest.mark.parametrize("cid", IDS)
def test_free_running_rejects_are_a_skipped_epoch_counter(native, monkeypatch, cid):
    """hmc_run(eps) + hmc_run(EPS_NAN) + hmc_run(eps) against the same with the middle run replaced by set_epoch: every middle epoch is
    rejected (asserted from the records), so the last run's records and the final state are equal"""
    c = rj.BY_ID[cid]
    runs = {}
    for tag in ("A", "B"):
        ch = open_handle(native, monkeypatch, c, seed=rj.SEED, chain_id=rj.CID)
        stage(ch, c)
        first = ch.hmc_run(c.eps, rj.L, 2)
        if tag == "A":
            for r in ch.hmc_run(rj.EPS_NAN, rj.L, 2):
                rejected_at_minus_inf(r, cid)
        else:
            ch.set_epoch(4)
        last = ch.hmc_run(c.eps, rj.L, 2)
        assert ch.last_transition_path == c.path, (cid, ch.last_transition_path)
        runs[tag] = (np.array([rec(r) for r in first]), np.array([rec(r) for r in last]), ch.get_state(), ch.get_hypers())
        assert all(rj.finite(v) for v in runs[tag])
    for a, b in zip(runs["A"], runs["B"]):
        np.testing.assert_array_equal(a, b)
    print(f"[rejects] {cid} free-running: accepted {runs['A'][0][:, 1]} then {runs['A'][1][:, 1]}")


@pytest.mark.parametrize("cid", rj.GROUP_CASES)
def test_group_neighbours_do_not_notice_a_diverging_chain(native, monkeypatch, cid):
    """a ChainGroup of three at their own (eps, L): chain 1 once sane, once at EPS_NAN with another L (the longest of the group, so the
    lockstep loop goes on for it alone), then a hyper transition in which chain 1's step diverges, then sane transitions for all.  Chains 0
    and 2: records, states and hypers bit for bit the same in both runs; chain 1 stays where it started"""
    c = rj.BY_ID[cid]
    _spec, _X, _Y, _theta, eta = rj.problem(c)
    thetas = rj.group_states(c)
    sane = np.array([c.eps, 0.5 * c.eps, 2.0 * c.eps], dtype=np.float32)
    plans = {"sane": (sane, np.array([3, 4, 2], dtype=np.int32), np.array([1e-4, 2e-4, 5e-5], dtype=np.float32)),
             "diverging": (np.array([c.eps, rj.EPS_NAN, 2.0 * c.eps], dtype=np.float32), np.array([3, 6, 2], dtype=np.int32),
                           np.array([1e-4, rj.EPS_H_NAN, 5e-5], dtype=np.float32))}
    runs = {}
    for tag, (eps, Ls, eps_h) in plans.items():
        grp = open_handle(native, monkeypatch, c, n_chains=3, seed=rj.SEED, chain_id=rj.CID)
        stage(grp, c, thetas)
        r1 = grp.hmc_run_each(eps, Ls, 3)
        assert grp.last_transition_path == c.path, (cid, grp.last_transition_path)
        s1, h1 = grp.get_state(), grp.get_hypers()
        rh = grp.hyper_step_each(eps_h, rj.L_H)
        s2, h2 = grp.get_state(), grp.get_hypers()
        r2 = grp.hmc_run_each(sane, plans["sane"][1], 2)
        runs[tag] = dict(r1=r1, rh=rh, r2=r2, s1=s1, h1=h1, s2=s2, h2=h2, s3=grp.get_state(), h3=grp.get_hypers())
    a, b = runs["sane"], runs["diverging"]
    for k in (0, 2):
        for key in ("r1", "r2"):
            np.testing.assert_array_equal(np.array([rec(r) for r in a[key][k]]), np.array([rec(r) for r in b[key][k]]), err_msg=f"chain {k} {key}")
            assert rj.finite(np.array([rec(r) for r in b[key][k]]))
        np.testing.assert_array_equal(rec(a["rh"][k]), rec(b["rh"][k]))
        for key in ("s1", "h1", "s2", "h2", "s3", "h3"):
            np.testing.assert_array_equal(a[key][k], b[key][k], err_msg=f"chain {k} {key}")
    # chain 1 of the diverging run: rejected at -inf, where it started, hypers too; then sane transitions from the cache its bootstrap made
    for r in b["r1"][1] + [b["rh"][1]]:
        rejected_at_minus_inf(r, cid)
    np.testing.assert_array_equal(b["s2"][1], thetas[1])
    np.testing.assert_array_equal(b["h2"][1], np.asarray(eta, np.float32))
    assert rj.finite(np.array([rec(r) for r in b["r2"][1]])) and rj.finite(b["s3"]) and rj.finite(b["h3"])
    assert b["r2"][1][0]["logp_old"] == b["r1"][1][0]["logp_old"]
    assert any(r["accepted"] for k in (0, 2) for r in b["r1"][k] + b["r2"][k])
    # both runs wrong alike would pass the comparison: after the hyper transition every chain's logp_old against fp64 at the state and the
    # hypers the group shows (4e-6 relative, the band of tests/test_gpu_group_likelihoods.py) -- after an accepted hyper step it is the
    # value EN_REFRESH formed from the cached statistic
    spec, X, Y = rj.problem(c)[:3]
    for k in range(3):
        lp64 = o.target_log_prob_and_grad(spec, b["s2"][k], b["h2"][k], X, Y, np.float64, w=rj.weights(c))[0]
        print(f"[rejects] {cid} group chain {k}: hyper accepted {b['rh'][k]['accepted']}, logp_old {b['r2'][k][0]['logp_old']:.9g} (fp64 {lp64:.9g})")
        assert abs(b["r2"][k][0]["logp_old"] - lp64) <= 4e-6 * max(abs(lp64), 1.0), (cid, k)
    assert any(r["accepted"] for r in a["r1"][1])
