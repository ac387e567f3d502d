"""GPU: the leapfrog update kernel (k_update, update_ops.hpp) on the paths its request order and its one-barrier reduction touch, against the
fp64 oracle.

k_update is shared by every kernel family, so the shapes here are chosen for ITS branches and run on whatever family takes them without
run-time instantiation: the prior lookup from registers (layers alternating Cauchy and Gaussian priors, every prior group with its own eta,
P no multiple of 4, the 16-layer stack that fills the 65 hypers of a handle), both block geometries (16 x 32, and 32 x 16 from 8192
parameters on), a column whose first batch of eight slab loads is peeled (the narrow family's 256 slabs) and columns that have none, eta
changing under the kernel (set_hypers, an accepted hyper transition, the per-call override of logp_grad), chain groups (gridDim.y > 1) and
per-chain step control (a chain whose trajectory has ended while the others go on).

Tolerances are the parity ones of tests/test_gpu_depth.py: log-prob 4e-6 relative, gradient 1e-4 of each tensor's inf-norm, the fp32 oracle
inside the same bounds first.  Every launch runs three times and must be bit-identical."""
import numpy as np
import pytest

import tbnn_oracle as o
from tensor_checks import layers_of, tensor_err
from test_gpu_depth import FLOOR, GRAD_TOL, LOGP_RTOL, problem, thrice

pytestmark = pytest.mark.gpu

SEED = 50
SMALL, ROWS = [3, 5, 3, 1], 37                       # P = 42
BIG, BIG_ROWS = [784, 20, 20, 1], 48                 # P = 16141 >= 8192: the 32 x 16 geometry
NARROW, NARROW_ROWS = [5, 50, 50, 50, 1], 16384 + 37  # the ahead-of-time narrow shape at its full grid (1027 row tiles over 256 workgroups
#                                                       of 4 waves): 256 slabs, the peeled first batch of eight loads in every thread
SIXTEEN = [4] + [16] * 15 + [1]                      # 16 layers: H = 65
# name -> (dims, rows, hidden activation, leapfrog step size, environment)
OFF = {"TBNN_TALL": "0", "TBNN_REGISTERED": "0"}     # the generic kernels, whatever another module registered in this process
CASES = {"small": (SMALL, ROWS, o.ACT_TANH, 1e-3, OFF), "big": (BIG, BIG_ROWS, o.ACT_TANH, 1e-4, {}),
         "narrow": (NARROW, NARROW_ROWS, o.ACT_RELU, 1e-5, {}), "sixteen": (SIXTEEN, ROWS, o.ACT_TANH, 5e-6, OFF)}
_made = {}


def distinct(eta, k0=0):
    """every prior group its own location and scale (the likelihood's sigma is left alone)"""
    e = np.array(eta, dtype=np.float64)
    k = np.arange(e.size - 1) + k0
    e[:-1] = e[:-1] * (1.0 + 0.02 * k) + np.where(k % 2 == 0, 0.003 * (1 + k) * (-1.0) ** (k // 2), 0.0)      # (locations: the even slots)
    return e.astype(np.float32)


def case(name):
    """(spec, X, Y, theta, eta, eps): computed once per module, never modified"""
    if name not in _made:
        dims, n, act, eps, _env = CASES[name]
        spec, X, Y, theta, eta = problem(dims, n, acts=[act] * (len(dims) - 2), alternate=True, seed=11)
        _made[name] = (spec, X, Y, theta, distinct(eta), eps)
    return _made[name]


def open_chain(native, monkeypatch, name, spec, n_chains=None, **kw):
    monkeypatch.delenv("TBNN_FAST_GRID", raising=False)
    for k, v in CASES[name][4].items():
        monkeypatch.setenv(k, v)
    generic = CASES[name][4] is OFF
    args = dict(likelihood=spec.likelihood, fixed_sd=spec.fixed_sd, kernel=native.KERNEL_GENERIC if generic else native.KERNEL_AUTO, jit=False, **kw)
    h = native.Chain(layers_of(spec), **args) if n_chains is None else native.ChainGroup(layers_of(spec), n_chains, **args)
    if name == "narrow":
        assert "fast3" in h.kernel_name, h.kernel_name
    return h


def lar_band(ref, lp64):
    return 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)


def check_transition(ch, spec, X, Y, theta, eta, eps, L, p0, prepare, what):
    """an injected transition, accepted and rejected, with its per-step energies against o.weight_step; prepare(ch) -> the eta it runs under"""
    for log_u in (-1e30, 1e30):
        def step():
            ch.set_state(theta); ch.set_hypers(eta)
            used = prepare(ch)
            out = ch.hmc_step(eps, L, p0=p0, log_u=log_u, trace=True)
            return out["log_accept_ratio"], out["accepted"], out["trace_logp"], ch.get_state(), used
        lar, acc, tr, state, used = thrice(step)
        lp64 = o.target_log_prob_and_grad(spec, theta, used, X, Y, np.float64)[0]
        ref = o.weight_step(spec, theta, used, X, Y, eps, L, p0, log_u, np.float64)
        e_tr = float(np.max(np.abs(np.asarray(tr) - ref.trace_logp) / np.maximum(np.abs(ref.trace_logp), 1.0)))
        e_q = float(np.abs(state - ref.theta).max() / max(1.0, np.abs(ref.theta).max()))
        print(f"{ch.kernel_name} {what} log_u {log_u:g}: trace {e_tr:.2e} ({LOGP_RTOL}) |d lar| {abs(lar - ref.log_accept_ratio):.2e} "
              f"({lar_band(ref, lp64):.2e}) state {e_q:.2e} (1e-5)")
        assert e_tr <= LOGP_RTOL, (what, e_tr)
        assert abs(lar - ref.log_accept_ratio) <= lar_band(ref, lp64), (what, lar, ref.log_accept_ratio)
        assert bool(acc) == ref.accepted, what
        assert e_q <= 1e-5, (what, e_q)


@pytest.mark.parametrize("name", list(CASES))
def test_transitions_while_eta_changes(native, monkeypatch, name):
    """L = 3 with injected momentum under the eta of set_hypers, under another eta set afterwards, and under the eta an accepted hyper
    transition leaves behind"""
    spec, X, Y, theta, eta, eps = case(name)
    assert spec.n_hypers == 4 * len(spec.layers) + 1 and len({float(v) for v in eta[:-1]}) == eta.size - 1
    rng = np.random.default_rng(len(spec.layers))
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    ph = rng.standard_normal(spec.n_hypers).astype(np.float32)
    eta2 = distinct(eta, 3)

    def after_hyper_step(ch):
        ch.logp_grad(theta, eta)                                  # the cached statistic the hyper target reads
        out = ch.hyper_step(1e-4, 5, p0=ph, log_u=-1e30)
        assert out["accepted"]
        return ch.get_hypers()

    def second_eta(ch):
        ch.set_hypers(eta2)
        return eta2

    ch = open_chain(native, monkeypatch, name, spec, seed=SEED, chain_id=2)
    try:
        ch.set_data(X, Y)
        check_transition(ch, spec, X, Y, theta, eta, eps, 3, p0, lambda c: eta, "set_hypers")
        check_transition(ch, spec, X, Y, theta, eta, eps, 3, p0, second_eta, "set_hypers again")
        check_transition(ch, spec, X, Y, theta, eta, eps, 3, p0, after_hyper_step, "after a hyper step")
    finally:
        ch.close()


@pytest.mark.parametrize("name", list(CASES))
def test_logp_grad_with_eta_override(native, monkeypatch, name):
    """UPD_GRAD_ONLY under the chain's own eta and under a per-call eta, which must not stay behind"""
    spec, X, Y, theta, eta, _eps = case(name)
    eta2 = distinct(eta, 3)
    ch = open_chain(native, monkeypatch, name, spec)
    try:
        ch.set_data(X, Y); ch.set_state(theta); ch.set_hypers(eta)
        for tag, e, arg in (("own", eta, None), ("override", eta2, eta2), ("own again", eta, None)):
            lp64, g64 = o.target_log_prob_and_grad(spec, theta, e, X, Y, np.float64)[:2]
            lp32, g32 = o.target_log_prob_and_grad(spec, theta, e, X, Y, np.float32)[:2]
            assert abs(lp32 - lp64) <= LOGP_RTOL * max(abs(lp64), 1.0), ("fp32 oracle", lp32, lp64)
            assert tensor_err(spec, g32, g64, FLOOR) <= GRAD_TOL, "fp32 oracle gradient"
            lp, g, _ = thrice(lambda: ch.logp_grad(theta, arg))
            e_lp, e_g = abs(lp - lp64) / max(abs(lp64), 1.0), tensor_err(spec, g, g64, FLOOR)
            print(f"{ch.kernel_name} eta {tag}: logp {e_lp:.2e} ({LOGP_RTOL}) gradient per tensor {e_g:.2e} ({GRAD_TOL})")
            assert e_lp <= LOGP_RTOL, (tag, lp, lp64)
            assert e_g <= GRAD_TOL, (tag, e_g)
    finally:
        ch.close()


def philox_key(chain):
    return SEED & 0xFFFFFFFF, (chain ^ (SEED >> 32)) & 0xFFFFFFFF


@pytest.mark.parametrize("name", ["small", "big"])
def test_chain_group_with_an_eta_per_chain(native, monkeypatch, name):
    """three chains behind one handle (gridDim.y = 3), each with its own state and its own eta, on the device's own draws: every chain's
    transition against the oracle's, and the group bit for bit the solo chains"""
    spec, X, Y, theta, eta, eps = case(name)
    C, c0, L = 3, 7, 3
    rng = np.random.default_rng(2)
    thetas = (theta[None, :] * (1.0 + 0.05 * rng.standard_normal((C, theta.size)))).astype(np.float32)
    etas = np.stack([distinct(eta, 2 * c) for c in range(C)])
    keys = ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new")

    def run(h, th, et):
        def step():
            h.set_epoch(0); h.set_state(th); h.set_hypers(et)
            out = h.hmc_step(eps, L)
            return out, h.get_state()
        return step

    grp = open_chain(native, monkeypatch, name, spec, n_chains=C, seed=SEED, chain_id=c0)
    try:
        grp.set_data(X, Y)
        g_out, g_state = run(grp, thetas, etas)()
        for _ in range(2):
            again, state = run(grp, thetas, etas)()
            assert [[r[k] for k in keys] for r in again] == [[r[k] for k in keys] for r in g_out] and np.array_equal(state, g_state)
    finally:
        grp.close()
    for c in range(C):
        k0, k1 = philox_key(c0 + c)
        p0 = o.philox_normals(spec.n_params, k0, k1, 0, o.PURPOSE_MOMENTUM)
        lu = float(o.philox_log_uniform(k0, k1, 0, o.PURPOSE_LOGU))
        ref = o.weight_step(spec, thetas[c], etas[c], X, Y, eps, L, p0, lu, np.float64)
        lp64 = o.target_log_prob_and_grad(spec, thetas[c], etas[c], X, Y, np.float64)[0]
        assert abs(g_out[c]["log_accept_ratio"] - ref.log_accept_ratio) <= lar_band(ref, lp64), (c, g_out[c], ref.log_accept_ratio)
        assert abs(g_out[c]["logp_new"] - ref.trace_logp[-1]) <= LOGP_RTOL * max(abs(ref.trace_logp[-1]), 1.0), c
        if abs(ref.log_accept_ratio - lu) > lar_band(ref, lp64):             # (a decision inside the band may fall either way)
            assert bool(g_out[c]["accepted"]) == ref.accepted, c
            assert np.abs(g_state[c] - ref.theta).max() <= 1e-5 * max(1.0, np.abs(ref.theta).max()), c
        ch = open_chain(native, monkeypatch, name, spec, seed=SEED, chain_id=c0 + c)
        try:
            ch.set_data(X, Y)
            s_out, s_state = run(ch, thetas[c], etas[c])()
            assert [g_out[c][k] for k in keys] == [s_out[k] for k in keys], (c, g_out[c], s_out)
            np.testing.assert_array_equal(g_state[c], s_state)
        finally:
            ch.close()


@pytest.mark.parametrize("name", ["small", "big"])
def test_step_control_per_chain(native, monkeypatch, name):
    """hmc_run_each with L = 1, 4, 2: chain 0's trajectory has ended while the others integrate on (k_update returns for it); every chain
    against the oracle at ITS (eps, L), and bit for bit the solo chain driven with them"""
    spec, X, Y, theta, eta, eps = case(name)
    C, c0 = 3, 3
    Ls, epss = [1, 4, 2], [eps, 0.5 * eps, 2.0 * eps]
    rng = np.random.default_rng(4)
    thetas = (theta[None, :] * (1.0 + 0.05 * rng.standard_normal((C, theta.size)))).astype(np.float32)
    etas = np.stack([distinct(eta, c) for c in range(C)])
    keys = ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new", "n_leapfrog")

    grp = open_chain(native, monkeypatch, name, spec, n_chains=C, seed=SEED, chain_id=c0)
    try:
        grp.set_data(X, Y)

        def step():
            grp.set_epoch(0); grp.set_state(thetas); grp.set_hypers(etas)
            out = grp.hmc_run_each(epss, Ls, 1)
            return [tuple(out[c][0][k] for k in keys) for c in range(C)], grp.get_state()
        recs, g_state = thrice(step)
    finally:
        grp.close()
    for c in range(C):
        k0, k1 = philox_key(c0 + c)
        p0 = o.philox_normals(spec.n_params, k0, k1, 0, o.PURPOSE_MOMENTUM)
        lu = float(o.philox_log_uniform(k0, k1, 0, o.PURPOSE_LOGU))
        ref = o.weight_step(spec, thetas[c], etas[c], X, Y, np.float32(epss[c]), Ls[c], p0, lu, np.float64)
        lp64 = o.target_log_prob_and_grad(spec, thetas[c], etas[c], X, Y, np.float64)[0]
        lar, acc, _lo, lp_new = recs[c][:4]
        assert recs[c][6] == Ls[c]
        assert abs(lar - ref.log_accept_ratio) <= lar_band(ref, lp64), (c, lar, ref.log_accept_ratio)
        assert abs(lp_new - ref.trace_logp[-1]) <= LOGP_RTOL * max(abs(ref.trace_logp[-1]), 1.0), c
        if abs(ref.log_accept_ratio - lu) > lar_band(ref, lp64):
            assert bool(acc) == ref.accepted, c
            assert np.abs(g_state[c] - ref.theta).max() <= 1e-5 * max(1.0, np.abs(ref.theta).max()), c
        ch = open_chain(native, monkeypatch, name, spec, seed=SEED, chain_id=c0 + c)
        try:
            ch.set_data(X, Y); ch.set_state(thetas[c]); ch.set_hypers(etas[c])
            s = ch.hmc_step(float(np.float32(epss[c])), Ls[c])
            assert recs[c] == tuple(s[k] for k in keys), (c, recs[c], s)
            np.testing.assert_array_equal(g_state[c], ch.get_state())
        finally:
            ch.close()
