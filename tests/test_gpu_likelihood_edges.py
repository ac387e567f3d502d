"""GPU: the Poisson, Student-t, negative-binomial, heteroscedastic Gaussian and Gamma likelihoods at the edges of their element arithmetic
(csrc/common.hpp log1p_fast, negbin_term, hetero_pair, gamma_term; kernels_fast.hpp lik_delta's Poisson branch), on every kernel family,
against the fp64 arms of the oracle.  The likelihood modules (test_gpu_poisson / _student / _negbin /
_hetero / _gamma) hold one well-conditioned problem per family and check sums over 500 .. 3,000 rows; here every dataset of tests/lik_edge_cases.py
holds ONE band of the quantity the element code branches on, on all of its 301 rows, so a formula that is wrong on one regime is not
diluted: log1p_fast's series and its switch at u = 1/4, negbin_term around t = 0, at |t| = ln 4, where e^-|t| passes through the denormals
and far past the range of exp, hetero_pair just inside, just outside and across the clip within one 16-row tile, the Poisson term with
the rate flushed to 0, around FLT_MIN and with e^f to 1e34, the Gamma term with e^-f to 2e37 against targets down to 1e-37, with e^-f
denormal or 0, and with y e^-f from 1e-30 to 1e20.  The shapes, activations, priors, TBNN_JIT_SKIP strings and environments are the likelihood
modules' own CASES (their make_chain builds the chains and asserts the kernel names), so the run-time libraries are the ones they compile.

(1) test_band: per (likelihood, case, band) logp_grad at the dataset's state -- value, statistic and gradient per tensor against fp64 --
    and forward over the rows at 1e-4 max(1, |f64|); every launch three times, bit-identical; everything finite.
(2) test_negbin_finite_where_promised: an injected transition from a far+ and a deep- dataset on fast3 (per-step kernels) and on the
    trajectory kernel, both decisions against the oracle's weight_step in fp64: never rejected for a non-finite statistic.
(3) test_rejected_where_promised: a momentum that carries the proposal to where the fp32 statistic is not finite (Student-t: u = inf or a
    non-finite f; heteroscedastic Gaussian: r^2 u past fp32 or a NaN g) is rejected whatever log u, and the chain keeps its state bit for bit.
    Gamma: a proposal whose last layer is the dataset's rescaled until log-means lie below -88.8, where e^-f is inf.
    A NaN in a kernel is an ordinary value: nothing here faults.
(4) test_row_weights_at_an_edge: weights all 1 give the unweighted bits, integer weights the fp64 reference with w.
(5) test_denormal_targets: Gamma targets below FLT_MIN, which staging admits, on three families at the project's bands.

Bands (lik_edge_cases.arms): the project's -- value and statistic 4e-6 relative, gradient 1e-4 of each tensor's largest entry (floor
1e-3), forward 1e-4 -- wherever tests/test_likelihood_edges_host.py shows the reference's fp32 arm inside HALF of them; otherwise
max(project band, 8 x the fp32 arm's gap against fp64 at that dataset), the rule of test_gpu_poisson.bands, computed from the references
alone.  The hardware exp flushes denormal results where NumPy's does not: at deep+- a difference below 1e-37 absolute, no band needed.

Measured on an MI355X (NOTES.md has the table per likelihood and band): the device within 0.63 of its band everywhere (`hetero mid
straddle`, value 2.5e-6), Poisson `high` next at 0.48 (value 1.9e-6); every other band below 0.35 (Poisson `flush`, the statistic 1.4e-6).  251 tests in 10.9 s with the
run-time libraries built.  Gamma, added since (NOTES.md): `deep-` on wide10 at 0.78 of its widened band (value 5.7e-5, a = 200), `high` at
0.32, every other Gamma band and the denormal targets below 0.08; 338 tests."""
import numpy as np
import pytest

import lik_edge_cases as E
import negbin_ref as nb
import tbnn_oracle as o
import test_gpu_gamma as tgg
import test_gpu_hetero as tgh
import test_gpu_negbin as tgn
import test_gpu_poisson as tgp
import test_gpu_student as tgs
from tensor_checks import layers_of
from test_gpu_freerun import SEED

pytestmark = pytest.mark.gpu

MODULE = {"student": tgs, "negbin": tgn, "hetero": tgh, "poisson": tgp, "gamma": tgg}
TRAJ_LIKS = ("negbin", "gamma")           # the log-link likelihoods whose transitions here run on the trajectory kernel too
FUSED = tgs.FUSED


def jit_jobs(lik):
    """the run-time instantiations of one likelihood's cases here (the likelihood module's own: same layers, likelihood and skip), the
    weighted fast3 library and, for the negative binomial and Gamma, the trajectory case"""
    mod, jobs = MODULE[lik], []
    for case in E.case_names(lik, traj=lik in TRAJ_LIKS):
        dims, _n, act, prior, fam, _env = E.case_of(lik, case)
        if fam in FUSED or fam == "traj":
            jobs.append(mod.job(E._spec(lik, dims, act, prior), skip=FUSED.get(fam, "")))
    dims, _n, act, prior, _fam, _env = E.case_of(lik, "fast3")
    jobs.append(mod.job(E._spec(lik, dims, act, prior), weighted=True))
    return jobs


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """compile this module's run-time shapes side by side before any test touches the GPU (cached: after the likelihood modules, or a
    second run, nothing compiles)"""
    from tensorbnn_amd import jit
    for lik in E.LIKS:
        jobs = jit_jobs(lik)
        assert len(jobs) <= 16
        assert jit.prebuild(jobs, processes=min(16, len(jobs))) == len(jobs)


def test_cases_are_the_likelihood_modules_own():
    for case in E.CASE_NAMES:
        assert tuple(tgp.CASES[case][:6]) == E.case_of("poisson", case) and tuple(nb.CASES[case][:6]) == E.case_of("negbin", case)
    assert tuple(tgp.TRAJ) == E.case_of("negbin", E.TRAJ)[:4]
    for case in E.CASE_NAMES + (E.TRAJ,):
        assert tuple(tgg.gr.CASES[case][:6]) == E.case_of("gamma", case) and tgg.gr.CASES[case][6] == E.gamma_shape(case)
    assert tgg.FUSED == FUSED and all(j in tgg.jit_jobs() for j in jit_jobs("gamma"))


def make(native, monkeypatch, ds, **kw):
    """the likelihood module's own make_chain: the case's family, environment and skip string, the kernel name asserted"""
    if ds.lik == "gamma":          # (its make_chain takes the shape: the call shape of the Gamma modules)
        return tgg.make_chain(native, monkeypatch, ds.case, ds.spec, ds.par["a"], **kw)
    return MODULE[ds.lik].make_chain(native, monkeypatch, ds.case, ds.spec, **kw)


def launch3(ch, ds):
    """logp_grad and forward at the dataset's state, three times, bit-identical"""
    lp, g, st = ch.logp_grad(ds.theta, ds.eta)
    f = ch.forward(ds.X, ds.theta)
    for _ in range(2):
        lp2, g2, st2 = ch.logp_grad(ds.theta, ds.eta)
        assert lp2 == lp and st2 == st and np.array_equal(g, g2), f"{ds.tag}: a repeated launch differs"
        assert np.array_equal(ch.forward(ds.X, ds.theta), f), f"{ds.tag}: a repeated forward differs"
    return lp, g, st, f


def judge(ds, lp, g, st, w=None, note=""):
    """value, statistic and gradient per tensor against fp64 at the dataset's bands; the figures printed before anything is asserted"""
    a = E.arms(ds, w)
    ev, eg = E.gaps(ds.spec, lp, g, a["lp64"], a["g64"])
    es = abs(st - a["st64"]) / abs(a["st64"])
    wide = "" if (a["bv"], a["bs"], max(a["bg"])) == (4e-6, 4e-6, 1e-4) else " (widened: 8 x the fp32 arm's gap)"
    print(f"[edges] {ds.tag}{note}: logp {lp:.9g} (fp64 {a['lp64']:.9g}) err {ev:.3e} of band {a['bv']:.3e}; statistic err {es:.3e} of band "
          f"{a['bs']:.3e}; gradient err max {max(eg):.3e}, err/band max {max(e / b for e, b in zip(eg, a['bg'])):.3f}{wide}")
    assert np.isfinite(lp) and np.isfinite(st) and np.all(np.isfinite(g)), f"{ds.tag}{note}: not finite"
    assert ev <= a["bv"], f"{ds.tag}{note}: logp {lp} against {a['lp64']}: {ev:.3e} > {a['bv']:.3e}"
    assert es <= a["bs"], f"{ds.tag}{note}: statistic {st} against {a['st64']}: {es:.3e} > {a['bs']:.3e}"
    for k, (e, b) in enumerate(zip(eg, a["bg"])):
        assert e <= b, f"{ds.tag}{note}: gradient of tensor {k}: {e:.3e} > {b:.3e}"


@pytest.mark.parametrize("key", E.all_keys(), ids=lambda k: "-".join(k))
def test_band(native, monkeypatch, key):
    ds = E.dataset(*key)
    ch = make(native, monkeypatch, ds)
    try:
        ch.set_data(ds.X, ds.Y)
        lp, g, st, f = launch3(ch, ds)
    finally:
        ch.close()
    judge(ds, lp, g, st)
    f64 = o.forward(ds.spec, ds.theta.astype(np.float64), ds.X.astype(np.float64), np.float64)
    assert f.shape == f64.shape and np.all(np.isfinite(f)), f"{ds.tag}: forward not finite"
    err = np.abs(f - f64) / np.maximum(1.0, np.abs(f64))
    assert err.max() <= 1e-4, f"{ds.tag}: forward {err.max():.3e} of max(1, |f64|)"


@pytest.mark.parametrize("case", E.DENORMAL_CASES)
def test_denormal_targets(native, monkeypatch, case):
    """include/tbnn.h admits every target > 0, the fp32 denormals too: a dataset whose targets lie below FLT_MIN (lik_edge_cases.MEASURED) is
    staged, and value, statistic and gradient meet the project's bands -- a kernel or a staging constant that took a denormal target for 0
    would turn rho = y e^-f of O(1) into 0 (or log y into -inf)"""
    ds = E.measured(case, "denormal-targets")
    ch = make(native, monkeypatch, ds)
    try:
        ch.set_data(ds.X, ds.Y)
        lp, g, st, _f = launch3(ch, ds)
    finally:
        ch.close()
    judge(ds, lp, g, st)


# ---------------------------------------------------------------------------------------------------------------------- finite where promised
@pytest.mark.parametrize("band", ["far+", "deep-"])
@pytest.mark.parametrize("case", ["fast3", E.TRAJ])
def test_negbin_finite_where_promised(native, monkeypatch, case, band):
    """every finite log-rate gives a finite term: one injected transition from log-rates far past the range of exp (t to 1e6) and from
    the denormal range of e^-|t|, on the per-step kernels and on the trajectory kernel; both decisions, the new state and the log accept
    ratio against fp64; never rejected for a non-finite statistic"""
    ds = E.dataset("negbin", case, band)
    r = ds.par["r"]
    if case == E.TRAJ:
        monkeypatch.setenv("TBNN_TRAJ", "1")
        monkeypatch.setenv("TBNN_JIT_SKIP", "")
        ch = native.Chain(layers_of(ds.spec), likelihood=o.LIK_NEG_BINOMIAL, lik_df=r, jit=True, seed=SEED)
        assert ch.kernel_name.startswith("jit-fast3<") and ",neg-binomial;" in ch.kernel_name, ch.kernel_name
        path = "trajectory"
    else:
        monkeypatch.setenv("TBNN_TRAJ", "0")
        ch = make(native, monkeypatch, ds, seed=SEED, chain_id=2)
        path = "per-step"
    try:
        ch.set_data(ds.X, ds.Y)
        p0 = np.random.default_rng(4).standard_normal(ds.spec.n_params).astype(np.float32)
        # the step: step_size's, shrunk by the ratio of the fp64 gradients' largest entries where the edge dataset's is the larger (far+: a
        # last layer that reaches t = 1e6 makes it 150 .. 5,000 times the ordinary problem's, and at the ordinary step the momentum's square
        # leaves fp32) -- a choice of input from the reference alone, as test_gpu_poisson's large-rate transition makes it; deep-: unchanged
        eps = nb.step_size(case) * min(1.0, np.abs(nb.ref64(case)[1]).max() / np.abs(E.arms(ds)["g64"]).max())
        lp64 = E.arms(ds)["lp64"]
        ref = o.weight_step(ds.spec, ds.theta, ds.eta, ds.X, ds.Y, eps, 4, p0, -1e30, np.float64)
        assert np.isfinite(ref.log_accept_ratio) and np.isfinite(ref.logp_new)
        tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
        # log u on either side of the reference's log accept ratio, two bands away: the kernel's rounding cannot flip the decision
        for log_u, accept in ((ref.log_accept_ratio - 2 * tol, True), (ref.log_accept_ratio + 2 * tol, False)):
            ch.set_state(ds.theta); ch.set_hypers(ds.eta)
            out = ch.hmc_step(eps, 4, p0=p0, log_u=log_u)
            print(f"[edges] {ds.tag} transition ({path}): lar {out['log_accept_ratio']:.9g} (fp64 {ref.log_accept_ratio:.9g}, band {tol:.3g}), "
                  f"logp {out['logp_old']:.9g} -> {out['logp_new']:.9g} (fp64 {lp64:.9g} -> {ref.logp_new:.9g})")
            assert ch.last_transition_path == path, ch.last_transition_path
            assert np.isfinite(out["log_accept_ratio"]) and np.isfinite(out["logp_new"]), f"{ds.tag}: rejected for a non-finite statistic"
            assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= tol, (ds.tag, out["log_accept_ratio"], ref.log_accept_ratio, tol)
            assert bool(out["accepted"]) == accept, (ds.tag, log_u)
            assert abs(out["logp_old"] - lp64) <= 4e-6 * max(abs(lp64), 1.0)
            assert abs(out["logp_new"] - ref.logp_new) <= 4e-6 * max(abs(ref.logp_new), 1.0)
            want = ref.theta_proposed if accept else ds.theta
            assert np.abs(ch.get_state() - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), ds.tag
    finally:
        ch.close()


# ---------------------------------------------------------------------------------------------------------------------- rejected where promised
REJECT = [("student", c) for c in ("fast3", "mid10", "lay_last", "generic")] + [("hetero", c) for c in ("fast3", "mid", "lay_last", "generic")]
REJECT += [("gamma", c) for c in ("fast3", E.TRAJ, "mid10", "lay_last", "generic")]          # (rejected_gamma, below)
EPS_FAR, P_FAR = 1e4, 1e16          # theta moves by ~1e20 per coordinate; the kinetic energy, sum p^2 ~ 1e32 P, stays inside fp32


@pytest.mark.parametrize("lik,case", REJECT, ids=lambda v: v)
def test_rejected_where_promised(native, monkeypatch, lik, case):
    """a momentum that carries the one-step proposal to outputs ~1e20 and beyond: on the CPU, the fp32 arm's statistic at the fp64
    proposal is not finite (Student-t: r^2 k = inf, or f itself past fp32; heteroscedastic Gaussian: r^2 u = inf on a row whose g lies
    below the clip, or a non-finite f, g).  The kernels' statistic is then inf or NaN -- ordinary values -- and k_energy rejects.
    Gamma: rejected_gamma"""
    if lik == "gamma":
        return rejected_gamma(native, monkeypatch, case)
    ds = E.dataset(lik, case, "switch" if lik == "student" else "inside")
    rng = np.random.default_rng(8)
    p0 = (P_FAR * rng.standard_normal(ds.spec.n_params)).astype(np.float32)
    g64 = E.arms(ds)["g64"]
    q1 = ds.theta.astype(np.float64) + EPS_FAR * (p0.astype(np.float64) + 0.5 * EPS_FAR * g64)          # the proposal of ONE leapfrog step
    with np.errstate(over="ignore", invalid="ignore"):
        f1 = o.forward(ds.spec, q1, ds.X.astype(np.float64), np.float64).astype(np.float32)
        stat32 = o.data_statistic(ds.spec, ds.eta, f1, ds.Y, np.float32)
    assert not np.isfinite(stat32), (ds.tag, stat32)
    assert float(np.sum(p0.astype(np.float64) ** 2)) < E.FLT_MAX / 16.0            # the kinetic energy is no reason to reject
    ch = make(native, monkeypatch, ds, seed=SEED)
    try:
        ch.set_data(ds.X, ds.Y); ch.set_state(ds.theta); ch.set_hypers(ds.eta)
        before = ch.logp_grad()
        for log_u in (-1e30, 0.0):
            out = ch.hmc_step(EPS_FAR, 1, p0=p0, log_u=log_u)
            assert out["accepted"] == 0 and out["log_accept_ratio"] == -np.inf, (ds.tag, log_u, out["accepted"], out["log_accept_ratio"])
            assert np.array_equal(ch.get_state(), ds.theta) and np.array_equal(ch.get_hypers(), ds.eta), ds.tag
            after = ch.logp_grad()
            assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.all(np.isfinite(after[1])), ds.tag
        ok = ch.hmc_step(3e-5, 3, p0=(p0 / P_FAR).astype(np.float32), log_u=-1e30)          # and it goes on from there
        assert ok["accepted"] == 1 and np.isfinite(ok["log_accept_ratio"]) and np.isfinite(ok["logp_new"]) and np.all(np.isfinite(ch.get_state()))
    finally:
        ch.close()


GAMMA_FAR, GAMMA_EPS = 1.5, 1e-3          # the last layer's factor: log-means of [-86, -20] become [-129, -30]; the step of the injected proposal


def rejected_gamma(native, monkeypatch, case):
    """include/tbnn.h: a log-mean below the fp32 range of e^-f gives a statistic that is not finite, and the proposal is rejected.  The
    `deep-` dataset with its last layer times 1.5 has log-means below -88.8 on some rows: logp_grad there is not finite (an ordinary
    value: nothing faults), and a one-step transition whose injected momentum carries the chain from the dataset's state to that proposal
    is rejected whatever log u; the state, the hypers and the next logp_grad are bit for bit what they were.  Per-step kernels of four
    families and the one-launch trajectory kernel."""
    ds = E.dataset("gamma", case, "deep-")
    a, spec = ds.par["a"], ds.spec
    ow, _ob = spec.offsets()[-1]
    far = ds.theta.copy()
    far[ow:] *= np.float32(GAMMA_FAR)
    g64 = E.arms(ds)["g64"]
    # the momentum of ONE leapfrog step of size eps from theta to `far`: q1 = theta + eps (p0 + eps / 2 g)
    p0 = ((far.astype(np.float64) - ds.theta) / GAMMA_EPS - 0.5 * GAMMA_EPS * g64).astype(np.float32)
    q1 = ds.theta.astype(np.float64) + GAMMA_EPS * (p0.astype(np.float64) + 0.5 * GAMMA_EPS * g64)
    with np.errstate(over="ignore", invalid="ignore"):
        for q in (far.astype(np.float64), q1):
            f1 = o.forward(spec, q, ds.X.astype(np.float64), np.float64)
            assert (f1 < -88.8).sum() >= 8 and np.all(np.isfinite(f1)), (ds.tag, f1.min())
            assert not np.isfinite(o.data_statistic(spec, ds.eta, f1.astype(np.float32), ds.Y, np.float32)), ds.tag
    assert float(np.sum(p0.astype(np.float64) ** 2)) < E.FLT_MAX / 16.0            # the kinetic energy is no reason to reject
    if case == E.TRAJ:
        monkeypatch.setenv("TBNN_TRAJ", "1")
        monkeypatch.setenv("TBNN_JIT_SKIP", "")
        ch = native.Chain(layers_of(spec), likelihood=o.LIK_GAMMA, lik_df=a, jit=True, seed=SEED)
        assert ch.kernel_name.startswith("jit-fast3<") and ",gamma;" in ch.kernel_name, ch.kernel_name
        path = "trajectory"
    else:
        monkeypatch.setenv("TBNN_TRAJ", "0")
        ch = make(native, monkeypatch, ds, seed=SEED)
        path = "per-step"
    try:
        ch.set_data(ds.X, ds.Y)
        lp_far, _g_far, st_far = ch.logp_grad(far, ds.eta)
        assert not np.isfinite(lp_far) and not np.isfinite(st_far), (ds.tag, lp_far, st_far)
        ch.set_state(ds.theta); ch.set_hypers(ds.eta)
        before = ch.logp_grad()
        assert np.isfinite(before[0]) and np.all(np.isfinite(before[1]))
        for log_u in (-1e30, 0.0):
            out = ch.hmc_step(GAMMA_EPS, 1, p0=p0, log_u=log_u)
            assert ch.last_transition_path == path, ch.last_transition_path
            assert out["accepted"] == 0 and out["log_accept_ratio"] == -np.inf, (ds.tag, log_u, out["accepted"], out["log_accept_ratio"])
            assert np.array_equal(ch.get_state(), ds.theta) and np.array_equal(ch.get_hypers(), ds.eta), ds.tag
            after = ch.logp_grad()
            assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.all(np.isfinite(after[1])), ds.tag
        small = (1e-3 * np.random.default_rng(8).standard_normal(spec.n_params)).astype(np.float32)
        ok = ch.hmc_step(1e-7, 3, p0=small, log_u=-1e30)          # and it goes on from there
        assert ok["accepted"] == 1 and np.isfinite(ok["log_accept_ratio"]) and np.isfinite(ok["logp_new"]) and np.all(np.isfinite(ch.get_state()))
    finally:
        ch.close()


# ---------------------------------------------------------------------------------------------------------------------- row weights at an edge
@pytest.mark.parametrize("case", ["fast3", "lay_last"])
@pytest.mark.parametrize("lik", E.LIKS)
def test_row_weights_at_an_edge(native, monkeypatch, lik, case):
    """one band per likelihood twice: weights all 1 -- the unweighted handle's bits, as csrc/common.hpp promises (a multiplication by the
    weight 1 is exact and nothing is contracted) -- and integer weights 0 .. 3 against the fp64 reference with w"""
    ds = E.dataset(lik, case, E.WEIGHT_BAND[lik])
    n = ds.X.shape[0]
    w = np.random.default_rng(21).integers(0, 4, n).astype(np.float32)
    fused = E.case_of(lik, case)[4] in FUSED
    ch = make(native, monkeypatch, ds)
    try:
        ch.set_data(ds.X, ds.Y)
        plain = ch.logp_grad(ds.theta, ds.eta)
        ch.set_row_weights(np.ones(n, np.float32))
        if fused:
            assert ",weighted;" in ch.kernel_name, ch.kernel_name
        ones = ch.logp_grad(ds.theta, ds.eta)
        if fused or lik != "poisson":          # (test_gpu_poisson: a weighted layered Poisson handle gives the same values, not the bits)
            assert ones[0] == plain[0] and ones[2] == plain[2] and np.array_equal(ones[1], plain[1]), f"{ds.tag}: weight 1 changes the bits"
        judge(ds, ones[0], ones[1], ones[2], note=" weight 1")
        ch.set_row_weights(w)
        lp, g, st = ch.logp_grad(ds.theta, ds.eta)
        again = ch.logp_grad(ds.theta, ds.eta)
        assert again[0] == lp and again[2] == st and np.array_equal(again[1], g)
        judge(ds, lp, g, st, w=w, note=" weights 0 .. 3")
        ch.set_row_weights(None)
        back = ch.logp_grad(ds.theta, ds.eta)
        assert back[0] == plain[0] and np.array_equal(back[1], plain[1])
    finally:
        ch.close()
