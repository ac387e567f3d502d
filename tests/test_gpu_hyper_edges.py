"""GPU: every kernel that reads the hyper vector eta, away from the values a chain starts from, against the fp64 oracle.

The edges are those of tests/hyper_edges.py: a negative g, moved locations, scales from 2^-28 to 2^28 on either side of the clamps of
(1e-8, 1e8), the likelihood's sd from 1e-8 to 1e8 and at the data's own residual scale, where the data term's hyper gradient cancels.
  (a) k_hyper's value and gradient (hyp_term's hardware reciprocal and log, the fp32 partial sums of the register-held path, hyper_finish's
      clamps and its 2 g chain rule) at every edge, one and two outputs, Cauchy, Gaussian and alternating priors;
  (b) the wave plan at the register limit of 1280 elements per wave: all shares at the limit, one share of 1281 beside twelve of 1280 in one
      group, sixteen and eighteen groups, waves without elements;
  (c) an injected hyper transition at every edge, accepted and rejected;
  (d) k_hyper_probs with the edges as its saved networks, under the chain's priors and under the other family, and with a 784 x 20 layer;
  (e) the weight target of every kernel family at every edge: prior_logp_partial, prior_grad in UPD_GRAD_ONLY, lik_sigma and each family's
      own 1 / s^2;
  (f) injected weight transitions on every family, the trajectory kernel's own prior_grad and gd = g s^2, and the hand-over across an
      accepted hyper step that moves the sd (k_refresh_grad_after_hyper with s_old != s_new), also from either clamp of the sd;
  (g) chain groups with an edge per chain, and the optimiser under a negative, a tiny and a clamped scale;
  (h) a Cauchy scale of 2^-80 (z^2 past the fp32 range) and of 0: non-finite values, no error, both transitions reject and leave the state
      bit for bit, and the handle works on.

Bands: tests/hyper_edges.py states them; tests/test_hyper_edges_host.py holds the fp32 oracle inside them first.  Every launch runs three
times and must be bit-identical.  Dropped cases: the hyper transition at sd_small and sd_in_lo (hyper_edges.HYPER_STEP_DROPPED says why); they
stay in (a), (e) and (f).

Largest error over its band, as an MI355X printed them (DESIGN.md section 4 has them too): hyper value 0.059 (Cauchy, g = 2^-5) and hyper
gradient 0.0085 (the cancelling data entry at sd_mle with two outputs; 0.0007 at neg_g and at the clamps); the hyper transition's log accept
ratio 0.59 (in_hi, clamp_hi) and 0.75 on the wave plan's 18 groups, eta after it 5.2e-7 (1e-4); k_hyper_probs 1.0e-7 relative (4e-6); the weight
target 2.7e-6 relative (generic, Cauchy, tiny; 4e-6; every fused family below 9e-7) and 4.1e-7 of a tensor's gradient (1e-4); traced weight
transitions 1.5e-6 (4e-6); the optimiser's theta 3.8e-6 lr (1e-5).  No kernel left a band."""
import numpy as np
import pytest

import edge_shapes as es
import hyper_edges as he
import optim_ref as R
import tbnn_oracle as o
from tensor_checks import layers_of, tensor_err, tensor_errs
from test_gpu_depth import FLOOR, thrice
from test_gpu_layered import scaled_problem
from test_gpu_update_paths import check_transition

pytestmark = pytest.mark.gpu

SEED = 50
ROWS, FUSED_ROWS, L_H = 257, 1007, 9
EDGES = list(he.ETA_EDGES)
# family -> (dims, rows, hidden activation, run-time instantiation, kernel-name prefix): shapes that are ahead-of-time instantiations or that
# tests/jit_shapes.json lists with likelihood 0
FAMILIES = {
    "fast3": ([5, 50, 50, 50, 1], FUSED_ROWS, o.ACT_RELU, False, "fast3<"),
    "fast": ([9, 160, 16], FUSED_ROWS, o.ACT_TANH, True, "jit-fast<"),
    "mid": ([20, 100, 48, 2], FUSED_ROWS, o.ACT_TANH, True, "jit-mid"),
    "tall": ([100, 64, 32, 1], FUSED_ROWS, o.ACT_TANH, True, "jit-tall"),
    "wide": ([10, 200, 256, 1], FUSED_ROWS, o.ACT_TANH, True, "jit-wide"),
    "layered": ([7, 17, 33, 2], ROWS, o.ACT_TANH, False, "layered<"),
    "generic": ([4, 16, 16, 1], ROWS, o.ACT_TANH, False, "generic"),
    "traj": ([1, 10, 10, 1], 100, o.ACT_RELU, False, "fast3<"),          # narrow and small enough for the trajectory kernel
}
_problems = {}


def family_problem(fam, prior=o.PRIOR_CAUCHY):
    """(spec, X, Y, theta, default eta) of a family's shape: computed once, never modified"""
    if (fam, prior) not in _problems:
        dims, n, act, _jit, _pre = FAMILIES[fam]
        spec, X, Y, theta, eta = scaled_problem(dims, n, [act] * (len(dims) - 2), prior, o.LIK_GAUSSIAN, seed=31)
        _problems[(fam, prior)] = (spec, X, Y, theta, o.default_hypers(spec, 0.1))
    return _problems[(fam, prior)]


def open_family(native, monkeypatch, fam, spec, n_chains=None, **kw):
    _dims, _n, _act, jit, prefix = FAMILIES[fam]
    monkeypatch.setenv("TBNN_JIT_SKIP", es.SKIP.get(fam, ""))
    monkeypatch.setenv("TBNN_TRAJ", "1")
    if fam in ("fast3", "fast", "mid", "tall"):
        monkeypatch.setenv("TBNN_FAST_GRID", "3")                   # 1007 rows = 63 row tiles over 3 workgroups
    else:
        monkeypatch.delenv("TBNN_FAST_GRID", raising=False)
    if fam in ("layered", "generic"):
        monkeypatch.setenv("TBNN_TALL", "0")
        monkeypatch.setenv("TBNN_REGISTERED", "0")
    args = dict(likelihood=spec.likelihood, fixed_sd=spec.fixed_sd, jit=jit,
                kernel=native.KERNEL_GENERIC if fam == "generic" else native.KERNEL_AUTO, **kw)
    h = native.Chain(layers_of(spec), **args) if n_chains is None else native.ChainGroup(layers_of(spec), n_chains, **args)
    assert h.kernel_name.startswith(prefix), f"{fam}: runs on {h.kernel_name}"
    return h


def open_generic(native, monkeypatch, spec, **kw):
    return open_family(native, monkeypatch, "generic", spec, **kw)


# ---------------------------------------------------------------- (a) the hyper target
@pytest.mark.parametrize("prior", list(he.PRIORS))
@pytest.mark.parametrize("d_out", [1, 2])
def test_hyper_target_at_every_edge(native, monkeypatch, d_out, prior):
    spec, X, Y, theta, eta0 = he.small_problem([4, 16, 16, d_out], ROWS, prior)
    ch = open_generic(native, monkeypatch, spec)
    worst = {}
    try:
        ch.set_data(X, Y); ch.set_state(theta); ch.set_hypers(eta0)
        for edge in EDGES:
            eta = he.eta_at(edge, spec, eta0, theta, X, Y)
            lp, g = thrice(lambda: ch.hyper_logp_grad(eta))
            T = he.hyper_grad_terms(spec, eta, theta, X, Y)
            lp64, g64 = o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64)
            print(f"{prior} d_out {d_out} {edge}: hyper value {abs(lp - lp64) / he.hyper_value_band(lp64):.2e} gradient "
                  f"{he.hyper_grad_ratio(g, g64, T):.2e} of their bands")
            worst[edge] = he.check_hyper_target(lp, g, spec, eta, theta, X, Y, edge)
        # the same through the chain's own eta: set_hypers, then no override
        for edge in he.KEEP:
            eta = he.eta_at(edge, spec, eta0, theta, X, Y)
            ch.set_hypers(eta)
            lp, g = thrice(lambda: ch.hyper_logp_grad())
            he.check_hyper_target(lp, g, spec, eta, theta, X, Y, edge + " (set_hypers)")
    finally:
        ch.close()
    print(f"{prior} d_out {d_out}: largest value {max(v for v, _ in worst.values()):.2e}, largest gradient "
          f"{max(g for _, g in worst.values()):.2e} of their bands")


# ---------------------------------------------------------------- (b) the wave plan at the register limit
def hyper_transition(ch, spec, X, Y, theta, eta, eps, ph, what):
    """an injected hyper transition, accepted and rejected, against o.hyper_step; -> the largest |d lar| over its band"""
    lp64 = float(o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64)[0])
    worst = 0.0
    for log_u in (-1e30, 1e30):
        def step():
            ch.set_state(theta); ch.set_hypers(eta)
            out = ch.hyper_step(eps, L_H, p0=ph, log_u=log_u)
            return out["log_accept_ratio"], out["accepted"], ch.get_hypers()
        lar, acc, hyp = thrice(step)
        with np.errstate(all="ignore"):
            ref = o.hyper_step(spec, eta, theta, X, Y, eps, L_H, ph, log_u, np.float64)
        band = he.lar_band(ref.log_accept_ratio, lp64)
        r = abs(lar - ref.log_accept_ratio) / band
        worst = max(worst, r)
        assert np.isfinite(ref.log_accept_ratio) and r <= 1.0, (what, lar, ref.log_accept_ratio, band)
        assert bool(acc) == ref.accepted == (log_u < 0), (what, log_u)
        if ref.accepted:
            e_eta = float(np.max(np.abs(hyp - ref.theta) / np.abs(ref.theta)))
            print(f"{what}: eps {eps:.3g} lar {ref.log_accept_ratio:.4g} |d lar| {r:.2e} of its band, eta {e_eta:.2e} (1e-4)")
            assert e_eta <= 1e-4, (what, hyp, ref.theta)
        else:
            assert np.array_equal(hyp, eta), (what, "a rejected hyper step changed eta")
    return worst


@pytest.mark.parametrize("prior", ["cauchy", "gaussian"])
@pytest.mark.parametrize("shape", list(he.PLAN_SHAPES))
def test_wave_plan_at_the_register_limit(native, monkeypatch, shape, prior):
    dims = he.PLAN_SHAPES[shape]
    plan, folded = he.hyper_plan(dims)
    want = {"held_at_limit": lambda: plan[0]["shares"] == [1280] * 13 and plan[0]["reread"] == 0,
            "mixed_paths": lambda: (plan[0]["held"], plan[0]["reread"]) == (12, 1) and max(plan[0]["shares"]) == 1281,
            "sixteen_groups": lambda: not folded and sorted(s for p in plan for s in p["shares"])[-3:] == [1280, 1281, 1952],
            "folded": lambda: folded == [15, 16, 17],
            "empty_waves": lambda: plan[0]["waves"] == 11 and plan[0]["empty"] == 8}
    assert want[shape](), (shape, plan, folded)
    spec, X, Y, theta, eta0 = he.small_problem(dims, 64, prior)
    ph = he.momenta(spec)[1]
    ch = open_generic(native, monkeypatch, spec)
    try:
        ch.set_data(X, Y); ch.set_state(theta); ch.set_hypers(eta0)
        for edge in ("default", "small", "neg_g"):
            eta = he.eta_at(edge, spec, eta0, theta, X, Y)
            lp, g = thrice(lambda: ch.hyper_logp_grad(eta))
            r_v, r_g = he.check_hyper_target(lp, g, spec, eta, theta, X, Y, (shape, edge))
            print(f"{shape} {prior} {edge}: hyper value {r_v:.2e} gradient {r_g:.2e} of their bands")
        eps = he.pick_eps((shape, prior, "default"), "hyper", spec, eta0, theta, X, Y, L_H, ph)
        hyper_transition(ch, spec, X, Y, theta, eta0, eps, ph, f"{shape} {prior} default")
    finally:
        ch.close()


# ---------------------------------------------------------------- (c) the hyper transition
@pytest.mark.parametrize("edge", he.HYPER_STEP_EDGES)
@pytest.mark.parametrize("prior", ["cauchy", "gaussian"])
def test_hyper_transition_at_every_edge(native, monkeypatch, prior, edge):
    dims = [4, 16, 16, 1]
    spec, X, Y, theta, eta0 = he.small_problem(dims, ROWS, prior)
    eta = he.eta_at(edge, spec, eta0, theta, X, Y)
    ph = he.momenta(spec)[1]
    eps = he.pick_eps((prior, edge, tuple(dims)), "hyper", spec, eta, theta, X, Y, L_H, ph)
    ch = open_generic(native, monkeypatch, spec)
    try:
        ch.set_data(X, Y)
        hyper_transition(ch, spec, X, Y, theta, eta, eps, ph, f"{prior} {edge}")
    finally:
        ch.close()


# ---------------------------------------------------------------- (d) saved networks
def hyper_probs_want(spec, judge, thetas, etas, dtype=np.float64):
    want = []
    for th, et in zip(thetas, etas):
        parts = o.unflatten(spec, th.astype(dtype))
        want.append(sum(float(o.layer_hyper_log_prob(o.DenseSpec(l.in_dim, l.out_dim, l.act, p), et[4 * k:4 * k + 4].astype(dtype), W, b, dtype))
                        for k, (l, p, (W, b)) in enumerate(zip(spec.layers, judge, parts))))
    return np.asarray(want)


@pytest.mark.parametrize("dims", [[4, 16, 16, 1], [784, 20, 20, 1]], ids=["small", "784x20"])
@pytest.mark.parametrize("prior", ["cauchy", "gaussian"])
def test_hyper_probs_many_with_the_edges_as_networks(native, monkeypatch, prior, dims):
    """one launch whose m networks are the edges, under the chain's own priors and judged under the other family; 784 x 20: a group spans
    many trips of the 256-thread loop"""
    spec, X, Y, theta, eta0 = he.small_problem(dims, 64, prior)
    rng = np.random.default_rng(17)
    etas = np.stack([he.eta_at(e, spec, eta0, theta, X, Y) for e in EDGES])
    # (weights three times their start: at a chain's starting scale the Cauchy sum of log(1 + z^2) cancels against its normaliser, and a
    # value near 0 has no relative error to speak of)
    thetas = (3.0 * theta[None, :] * (1.0 + 0.2 * rng.standard_normal((len(EDGES), theta.size)))).astype(np.float32)
    own = [l.prior for l in spec.layers]
    other = [o.PRIOR_GAUSSIAN if p == o.PRIOR_CAUCHY else o.PRIOR_CAUCHY for p in own]
    ch = open_generic(native, monkeypatch, spec)
    try:
        for tag, arg, judge in (("own priors", None, own), ("the other family", other, other)):
            got = thrice(lambda: (ch.hyper_probs_many(thetas, etas, priors=arg),))[0]
            want = hyper_probs_want(spec, judge, thetas, etas)
            with np.errstate(all="ignore"):                            # the fp32 oracle inside the band first
                want32 = hyper_probs_want(spec, judge, thetas, etas, np.float32)
            assert np.all(np.abs(want32 - want) <= 4e-6 * np.abs(want) + 1e-6), ("fp32 oracle", tag, dict(zip(EDGES, np.abs(want32 - want) / np.abs(want))))
            err = np.abs(got - want) / np.abs(want)
            print(f"hyper_probs_many {prior} {dims} under {tag}: worst {err.max():.2e} relative (4e-6) at {EDGES[int(err.argmax())]}")
            assert np.all(np.isfinite(want)) and np.all(np.abs(got - want) <= 4e-6 * np.abs(want) + 1e-6), (tag, dict(zip(EDGES, err)))
    finally:
        ch.close()


# ---------------------------------------------------------------- (e) the weight target
def weight_target(ch, spec, X, Y, theta, eta, what):
    lp64, g64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[:2]
    # the fp32 oracle inside the bounds first: the case is conditioned well enough to judge the device
    lp32, g32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)[:2]
    assert abs(lp32 - lp64) <= he.LOGP_RTOL * max(abs(lp64), 1.0), ("fp32 oracle", what, lp32, lp64)
    assert tensor_err(spec, g32, g64, FLOOR) <= he.GRAD_TOL, ("fp32 oracle gradient", what)
    lp, g, _ = thrice(lambda: ch.logp_grad(theta, eta))
    e_lp, e_g = abs(lp - lp64) / max(abs(lp64), 1.0), tensor_err(spec, g, g64, FLOOR)
    print(f"{ch.kernel_name} {what}: logp {e_lp:.2e} ({he.LOGP_RTOL}) gradient per tensor {e_g:.2e} ({he.GRAD_TOL})")
    assert e_lp <= he.LOGP_RTOL, (what, lp, lp64)
    assert e_g <= he.GRAD_TOL, (what, tensor_errs(spec, g, g64, FLOOR))
    return e_lp, e_g


@pytest.mark.parametrize("prior", ["cauchy", "gaussian"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_weight_target_at_every_edge(native, monkeypatch, fam, prior):
    spec, X, Y, theta, eta0 = family_problem(fam, he.PRIORS[prior])
    ch = open_family(native, monkeypatch, fam, spec)
    try:
        ch.set_data(X, Y); ch.set_state(theta); ch.set_hypers(eta0)
        errs = [weight_target(ch, spec, X, Y, theta, he.eta_at(e, spec, eta0, theta, X, Y), f"{prior} {e}") for e in EDGES]
    finally:
        ch.close()
    print(f"{fam} {prior}: largest logp {max(e for e, _ in errs):.2e} ({he.LOGP_RTOL}), largest gradient {max(g for _, g in errs):.2e} ({he.GRAD_TOL})")


# ---------------------------------------------------------------- (f) the weight transition
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_weight_transition_at_the_edges(native, monkeypatch, fam):
    """hmc_step with its per-step energies at a negative g, a small scale and a small sd, accepted and rejected"""
    spec, X, Y, theta, eta0 = family_problem(fam)
    p0 = he.momenta(spec)[0]
    ch = open_family(native, monkeypatch, fam, spec, seed=SEED, chain_id=2)
    try:
        ch.set_data(X, Y)
        for edge in he.WEIGHT_STEP_EDGES:
            eta = he.eta_at(edge, spec, eta0, theta, X, Y)
            eps = he.pick_eps((fam, edge), "weight", spec, eta, theta, X, Y, 3, p0)
            check_transition(ch, spec, X, Y, theta, eta, eps, 3, p0, lambda c: eta, f"{edge} eps {eps:.3g}")
    finally:
        ch.close()


def test_trajectory_kernel_at_the_edges(native, monkeypatch):
    """the whole trajectory in one launch: kernels_traj.hpp's own prior_grad and its gd = g s^2"""
    spec, X, Y, theta, eta0 = family_problem("traj")
    p0 = he.momenta(spec)[0]
    ch = open_family(native, monkeypatch, "traj", spec, seed=SEED, chain_id=2)
    try:
        ch.set_data(X, Y)
        for edge in he.WEIGHT_STEP_EDGES:
            eta = he.eta_at(edge, spec, eta0, theta, X, Y)
            eps = he.pick_eps(("traj", edge), "weight", spec, eta, theta, X, Y, 3, p0)
            lp64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[0]
            for log_u in (-1e30, 1e30):
                def step():
                    ch.set_state(theta); ch.set_hypers(eta)
                    out = ch.hmc_step(eps, 3, p0=p0, log_u=log_u)
                    return out["log_accept_ratio"], out["accepted"], ch.get_state()
                lar, acc, state = thrice(step)
                assert ch.last_transition_path == "trajectory", ch.last_transition_path
                ref = o.weight_step(spec, theta, eta, X, Y, eps, 3, p0, log_u, np.float64)
                band = he.lar_band(ref.log_accept_ratio, lp64)
                e_q = float(np.abs(state - ref.theta).max() / max(1.0, np.abs(ref.theta).max()))
                print(f"trajectory {edge} log_u {log_u:g}: |d lar| {abs(lar - ref.log_accept_ratio):.2e} ({band:.2e}) state {e_q:.2e} (1e-5)")
                assert abs(lar - ref.log_accept_ratio) <= band, (edge, lar, ref.log_accept_ratio)
                assert bool(acc) == ref.accepted and e_q <= 1e-5, (edge, acc, e_q)
            # the gradient the trajectory's tail left (g and gd = g s^2) starts the next transition, behind an accepted hyper step
            ch.set_state(theta); ch.set_hypers(eta)
            ch.hmc_step(eps, 3, p0=p0, log_u=-1e30)
            assert ch.last_transition_path == "trajectory"
            q1 = ch.get_state()
            ph = he.momenta(spec)[1]
            eps_h = he.pick_eps(("traj", edge, "behind"), "hyper", spec, eta, q1, X, Y, L_H, ph)
            assert ch.hyper_step(eps_h, L_H, p0=ph, log_u=-1e30)["accepted"]
            used = ch.get_hypers()
            out = ch.hmc_step(eps, 3, p0=p0, log_u=-1e30)
            ref = o.weight_step(spec, q1, used, X, Y, eps, 3, p0, -1e30, np.float64)
            lp1 = o.target_log_prob_and_grad(spec, q1, used, X, Y, np.float64)[0]
            assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= he.lar_band(ref.log_accept_ratio, lp1), (edge, "behind a hyper step")
            assert np.abs(ch.get_state() - ref.theta).max() <= 1e-5 * max(1.0, np.abs(ref.theta).max())
    finally:
        ch.close()


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_hand_over_across_a_hyper_step_that_moves_the_sd(native, monkeypatch, fam):
    """k_refresh_grad_after_hyper: the cached data gradient gd = g s_old^2 times 1 / s_new^2, from a small sd (s_new / s_old a real factor) and
    from either clamp of the sd (both sides clamp alike)"""
    spec, X, Y, theta, eta0 = family_problem(fam)
    p0, ph = he.momenta(spec)
    ch = open_family(native, monkeypatch, fam, spec, seed=SEED, chain_id=2)
    try:
        ch.set_data(X, Y)
        for edge in he.HANDOVER_EDGES:
            eta = he.eta_at(edge, spec, eta0, theta, X, Y)
            eps_h = he.pick_eps((fam, edge), "hyper", spec, eta, theta, X, Y, L_H, ph)
            moved = []

            def after_hyper_step(c):
                c.logp_grad(theta, eta)                                # the gradient and the statistic under the old sd
                assert c.hyper_step(eps_h, L_H, p0=ph, log_u=-1e30)["accepted"]
                moved.append(c.get_hypers())
                return moved[-1]
            with np.errstate(all="ignore"):
                new64 = o.hyper_step(spec, eta, theta, X, Y, eps_h, L_H, ph, -1e30, np.float64).theta
            eps = he.pick_eps((fam, edge, "behind"), "weight", spec, new64.astype(np.float32), theta, X, Y, 3, p0)
            check_transition(ch, spec, X, Y, theta, eta, eps, 3, p0, after_hyper_step, f"behind a hyper step from {edge}")
            ratio = float(moved[-1][-1] / eta[-1]) ** 4                 # s_new^2 / s_old^2 before the clamp
            print(f"{fam} {edge}: the hyper step took the sd root from {eta[-1]:.6g} to {moved[-1][-1]:.6g} (variance x {ratio:.5f})")
            if edge == "sd_small":
                assert abs(ratio - 1.0) >= 1e-3, "the sd did not move by a factor the bands would see"
    finally:
        ch.close()


# ---------------------------------------------------------------- (g) groups and the optimiser
GROUP_EDGES = ("neg_g", "small", "in_lo", "sd_large")


def philox_draws(spec, chain, hyper):
    pm, pu = (o.PURPOSE_HYPER_MOMENTUM, o.PURPOSE_HYPER_LOGU) if hyper else (o.PURPOSE_MOMENTUM, o.PURPOSE_LOGU)
    n = spec.n_hypers if hyper else spec.n_params
    return o.philox_normals(n, SEED, chain, 0, pm), float(o.philox_log_uniform(SEED, chain, 0, pu))


@pytest.mark.parametrize("fam", ["fast3", "generic"])
def test_chain_group_with_an_edge_per_chain(native, monkeypatch, fam):
    """four chains behind one handle, each at another edge and its own step sizes, on the device's draws: hyper_step_each then a weight
    transition, bit for bit the four solo chains; chains 1 and 3 against the oracle"""
    spec, X, Y, theta, eta0 = family_problem(fam)
    C, c0 = len(GROUP_EDGES), 5
    etas = np.stack([he.eta_at(e, spec, eta0, theta, X, Y) for e in GROUP_EDGES])
    eps_h, eps_w = [], []
    for c, edge in enumerate(GROUP_EDGES):
        ph = philox_draws(spec, c0 + c, True)[0]
        pw = philox_draws(spec, c0 + c, False)[0]
        eps_h.append(he.pick_eps((fam, edge, "group", c), "hyper", spec, etas[c], theta, X, Y, L_H, ph))
        eps_w.append(he.pick_eps((fam, edge, "group", c), "weight", spec, etas[c], theta, X, Y, 3, pw) / 4)   # (behind a hyper step that moved eta)
    keys = ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new")
    grp = open_family(native, monkeypatch, fam, spec, n_chains=C, seed=SEED, chain_id=c0)
    try:
        grp.set_data(X, Y)

        def run():
            grp.set_epoch(0); grp.set_state(theta); grp.set_hypers(etas)
            gh = grp.hyper_step_each(eps_h, L_H)
            hyp = grp.get_hypers()
            gw = grp.hmc_step_each(eps_w, [3] * C)
            return [[r[k] for k in keys] for r in gh], hyp, [[r[k] for k in keys] for r in gw], grp.get_state()
        gh, g_hyp, gw, g_state = thrice(run)
    finally:
        grp.close()
    for c, edge in enumerate(GROUP_EDGES):
        ch = open_family(native, monkeypatch, fam, spec, seed=SEED, chain_id=c0 + c)
        try:
            ch.set_data(X, Y); ch.set_epoch(0); ch.set_state(theta); ch.set_hypers(etas[c])
            sh = ch.hyper_step(eps_h[c], L_H)
            s_hyp = ch.get_hypers()
            sw = ch.hmc_step(eps_w[c], 3)
            assert gh[c] == [sh[k] for k in keys] and gw[c] == [sw[k] for k in keys], (edge, gh[c], sh, gw[c], sw)
            np.testing.assert_array_equal(g_hyp[c], s_hyp)
            np.testing.assert_array_equal(g_state[c], ch.get_state())
        finally:
            ch.close()
        if c not in (1, 3):
            continue
        ph, lu_h = philox_draws(spec, c0 + c, True)
        pw, lu_w = philox_draws(spec, c0 + c, False)
        with np.errstate(all="ignore"):
            rh = o.hyper_step(spec, etas[c], theta, X, Y, eps_h[c], L_H, ph, lu_h, np.float64)
        lp_h = float(o.hyper_log_prob_and_grad(spec, etas[c], theta, X, Y, np.float64)[0])
        band_h = he.lar_band(rh.log_accept_ratio, lp_h)
        assert abs(gh[c][0] - rh.log_accept_ratio) <= band_h, (edge, gh[c][0], rh.log_accept_ratio)
        if abs(rh.log_accept_ratio - lu_h) > band_h:                   # (a decision inside the band may fall either way)
            assert bool(gh[c][1]) == rh.accepted, edge
        if gh[c][1]:
            assert np.max(np.abs(g_hyp[c] - rh.theta_proposed) / np.abs(rh.theta_proposed)) <= 1e-4, edge
        else:
            assert np.array_equal(g_hyp[c], etas[c]), edge
        used = g_hyp[c]                                                # the weight transition under the eta the device's hyper step left
        rw = o.weight_step(spec, theta, used, X, Y, eps_w[c], 3, pw, lu_w, np.float64)
        lp_w = o.target_log_prob_and_grad(spec, theta, used, X, Y, np.float64)[0]
        band_w = he.lar_band(rw.log_accept_ratio, lp_w)
        print(f"{fam} chain {c} ({edge}): hyper |d lar| {abs(gh[c][0] - rh.log_accept_ratio):.2e} ({band_h:.2e}), weight |d lar| "
              f"{abs(gw[c][0] - rw.log_accept_ratio):.2e} ({band_w:.2e})")
        assert abs(gw[c][0] - rw.log_accept_ratio) <= band_w, (edge, gw[c][0], rw.log_accept_ratio)
        assert abs(gw[c][3] - rw.trace_logp[-1]) <= he.LOGP_RTOL * max(abs(rw.trace_logp[-1]), 1.0), edge
        if abs(rw.log_accept_ratio - lu_w) > band_w:
            assert bool(gw[c][1]) == rw.accepted, edge
            assert np.abs(g_state[c] - rw.theta).max() <= 1e-5 * max(1.0, np.abs(rw.theta).max()), edge


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("edge", ["neg_g", "tiny", "clamp_lo"])
@pytest.mark.parametrize("fam", ["fast3", "generic"])
def test_three_adam_steps_under_an_edge(native, monkeypatch, fam, edge):
    """Chain.optimize on the posterior under Gaussian priors with a negative, a tiny and a clamped scale (k_optim's prior_grad, k_optim_logp's
    prior_logp_partial), at the bands of tests/test_gpu_optimize.py's step arithmetic: the moments to 4 fp32 ulps and the new theta to
    1e-5 lr from the device's own gradient, that gradient to 1e-4 of each tensor (floor 1e-3), the checked objective to 4e-6"""
    spec, X, Y, theta0, eta0 = family_problem(fam, o.PRIOR_GAUSSIAN)
    eta = he.eta_at(edge, spec, eta0, theta0, X, Y)
    lr = R.F32(0.05)
    ch = open_family(native, monkeypatch, fam, spec)
    try:
        ch.set_data(X, Y); ch.set_state(theta0); ch.set_hypers(eta)
        P = spec.n_params
        th, m, v, vh = theta0.copy(), np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32)
        for t in range(1, 4):
            out = ch.optimize(1, lr=lr, check_every=1, keep="last", reset=(t == 1))
            st, new = ch.optim_state(), ch.get_state()
            assert st["t"] == t and out["diverged"] == 0 and np.all(np.isfinite(out["trace"])) and np.abs(new).max() < 8.0
            g = st["g"].astype(np.float64)
            th64, m64, v64, vh64 = R.adam_step(th, g, m, v, vh, t, lr, dtype=np.float64)
            m_mag = np.maximum(np.abs(m64), np.maximum(np.abs(R.B1 * m.astype(np.float64)), np.abs((1.0 - R.B1) * g)))
            for k, ref, mag in (("m", m64, m_mag), ("v", v64, v64), ("vhat", vh64, vh64)):
                err = np.abs(st[k].astype(np.float64) - ref)
                assert np.all(err <= 4 * ulp32(mag)), (edge, t, k, float((err / ulp32(mag)).max()))
            e_th = np.abs(new.astype(np.float64) - th64).max() / lr
            lp64, g64 = o.target_log_prob_and_grad(spec, th, eta, X, Y, np.float64)
            e_g = max(tensor_errs(spec, st["g"], g64, 1e-3))
            e_lp = abs(out["trace"][0] - lp64) / abs(lp64)
            print(f"{ch.kernel_name} {edge} step {t}: theta {e_th:.2e} lr (1e-5) gradient per tensor {e_g:.2e} (1e-4) objective {e_lp:.2e} (4e-6)")
            assert e_th <= 1e-5 and e_g <= 1e-4 and e_lp <= 4e-6, (edge, t, e_th, e_g, e_lp)
            th, m, v, vh = new, st["m"], st["v"], st["vhat"]
    finally:
        ch.close()


# ---------------------------------------------------------------- (h) non-finite, contained
@pytest.mark.parametrize("g_bad", [2.0 ** -40, 0.0], ids=["g=2^-40", "g=0"])
def test_a_non_finite_prior_term_is_contained(native, monkeypatch, g_bad):
    """a Cauchy layer whose z^2 passes the fp32 range (the fp32 oracle gives inf too) or whose scale is 0: arithmetic on inf and NaN in
    loops of fixed length, no address depends on a value"""
    spec, X, Y, theta, eta0 = he.small_problem([4, 16, 16, 1], ROWS, "cauchy")
    bad = eta0.copy()
    bad[1] = np.float32(g_bad)
    with np.errstate(all="ignore"):
        assert not np.isfinite(o.hyper_log_prob_and_grad(spec, bad, theta, X, Y, np.float32)[0])
        assert not np.isfinite(o.target_log_prob_and_grad(spec, theta, bad, X, Y, np.float32)[0])
    p0, ph = he.momenta(spec)
    ch = open_generic(native, monkeypatch, spec, seed=SEED, chain_id=1)
    try:
        ch.set_data(X, Y); ch.set_state(theta); ch.set_hypers(bad)
        runs = [(ch.hyper_logp_grad(bad), ch.logp_grad(theta, bad)[:2]) for _ in range(3)]
        (lp_h, _gh), (lp_w, _gw) = runs[0]
        assert not np.isfinite(lp_h) and not np.isfinite(lp_w), (lp_h, lp_w)
        for again in runs[1:]:                                         # the same bits, NaN included
            assert all(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) for x, y in zip(runs[0], again) for a, b in zip(x, y))
        for log_u in (-1e30, 1e30):
            out = ch.hyper_step(1e-5, L_H, p0=ph, log_u=log_u)
            assert not out["accepted"] and np.array_equal(ch.get_hypers(), bad), out
            out = ch.hmc_step(1e-4, 3, p0=p0, log_u=log_u)
            assert not out["accepted"] and np.array_equal(ch.get_state(), theta) and np.array_equal(ch.get_hypers(), bad), out
        # the handle works on: the default eta meets (a)'s bands, and a transition under it the oracle
        ch.set_hypers(eta0)
        lp, g = thrice(lambda: ch.hyper_logp_grad(eta0))
        he.check_hyper_target(lp, g, spec, eta0, theta, X, Y, "behind a non-finite eta")
        eps = he.pick_eps(("cauchy", "default", (4, 16, 16, 1)), "hyper", spec, eta0, theta, X, Y, L_H, ph)
        hyper_transition(ch, spec, X, Y, theta, eta0, eps, ph, "behind a non-finite eta")
    finally:
        ch.close()
