"""GPU: every kernel family at network depths up to the C ABI's 16 dense layers, against the fp64 oracle.

The depth-dependent paths no other module reaches: the fused families at 9 layers and at the deepest depth each admits (tests/edge_shapes.py's
depth walks), the hyper transition's wave plan past 16 prior groups (k_hyper: groups 15 .. 2 nl - 1 folded into wave 15, shares above
HYP_REG * 64 re-read from memory; 16 layers with a Gaussian likelihood fill HYP_MAXH = 65), k_hyper_probs, the wide family's weight ring past
its four slots, the layered family's fused tail over every trailing layer, the packed per-layer activation code at its nine layers, and the
categorical likelihood behind deep stacks.

Tolerances are the parity ones, with no looser tier: log-prob 4e-6 relative, gradient 1e-4 of each W_l / b_l's own inf-norm (the early layers of
a deep network have small gradients), forward 2e-5.  The problems keep their activations O(1) (test_gpu_layered.scaled_problem) and the fp32
oracle must sit inside the same bounds before the device is judged.  Every launch runs three times and must be bit-identical."""
import numpy as np
import pytest

import edge_shapes as es
import tbnn_oracle as o
from tensor_checks import layers_of, tensor_err
from test_gpu_layered import scaled_problem

pytestmark = pytest.mark.gpu

LOGP_RTOL, GRAD_TOL, FWD_TOL = 4e-6, 1e-4, 2e-5
PREFIX = {"fast3": "jit-fast3", "fast": "jit-fast<", "mid": "jit-mid", "tall": "jit-tall", "wide": "jit-wide", "layered": "layered<",
          "generic": "generic", "layered_jit": "layered<"}        # layered_jit: the layered family reached with run-time instantiation on
SKIP = dict(es.SKIP, layered="", generic="")
GRID = 3                          # TBNN_FAST_GRID: 1007 rows = 63 row tiles over 3 workgroups
N_ROWS, N_WIDE = 1007, 17009      # wide: 1064 row tiles, waves walk more than one


def _edge(name):
    return next(c["dims"] for c in es.cases() if c["name"] == name)


def _stack(d_in, width, nl, d_out):
    return [d_in] + [width] * (nl - 1) + [d_out]


# the deepest shape each family admits (tests/edge_shapes.py depth walks) and a 9-layer shape
DEEP = {"fast3": _edge("narrow-depth"), "fast": _edge("narrow-depth-fast"), "mid": _edge("mid-depth"), "tall": _edge("tall-depth"),
        "wide": _edge("wide-depth"), "layered": _stack(4, 16, 16, 1), "generic": _stack(4, 16, 16, 1)}
# (a process registers one kernel library per shape: the narrow and mid cases of one depth differ in their fan-in)
NINE = {"fast3": _stack(4, 16, 9, 1), "fast": _stack(5, 16, 9, 1), "mid": _stack(6, 16, 9, 1), "tall": _stack(300, 16, 9, 2),
        "wide": _stack(10, 64, 9, 1), "layered": _stack(4, 16, 9, 1), "generic": _stack(4, 16, 9, 1)}
EIGHT = {"fast3": _stack(4, 16, 8, 1), "fast": _stack(5, 16, 8, 1), "mid": _stack(6, 16, 8, 1), "tall": _stack(300, 16, 8, 2),
         "wide": _stack(10, 64, 8, 1), "layered": _stack(4, 16, 8, 1)}
CASES = [(f, "nine", NINE[f]) for f in NINE] + [(f, "deep", DEEP[f]) for f in DEEP]
# the hyper transition: 8 layers (16 groups, one wave each, no fold), 9 (groups 15 .. 17 folded into wave 15), and 16 layers where the family
# takes them (H = 65).  The wide shapes' 64 x 64 weight groups exceed HYP_REG * 64 = 1280: the memory pass, beside the fold.
HYPER = ([(f, "eight", EIGHT[f]) for f in EIGHT] + [(f, "nine", NINE[f]) for f in EIGHT]
         + [(f, "deep", DEEP[f]) for f in ("mid", "wide", "layered")])
# nine hidden layers, the activation changing from each layer to the next and a non-zero code in the ninth slot (bits 24 .. 26 of the
# packed code); one exp layer, behind a bounded one
MIXED_ACTS = [o.ACT_TANH, o.ACT_RELU, o.ACT_SIGMOID, o.ACT_ELU, o.ACT_TANH, o.ACT_EXP, o.ACT_TANH, o.ACT_RELU, o.ACT_ELU]
MIXED = {"fast3": _stack(4, 16, 10, 1), "mid": _stack(6, 16, 10, 1), "wide": _stack(10, 32, 10, 1)}
# 9 layers of 8 units: the deepest narrow stack whose trajectory kernel (kernels_traj.hpp, 4 waves) fits
TRAJ = _stack(4, 8, 9, 1)
CATEGORICAL = {"mid": _edge("mid-depth-outputs"), "wide": _stack(10, 64, 16, 10)}


def _id(fam, tag, dims):
    return f"{fam}-{tag}-{len(dims) - 1}layers"


def problem(dims, n, acts=None, alternate=False, lik=o.LIK_GAUSSIAN, seed=0):
    """O(1) activations at any depth (He-scaled weights, inputs scaled by the fan-in); alternate: Cauchy and Gaussian priors layer by layer"""
    spec, X, Y, theta, eta = scaled_problem(dims, n, acts or [o.ACT_TANH] * (len(dims) - 2), o.PRIOR_CAUCHY, lik, seed=seed)
    if alternate:
        for k, l in enumerate(spec.layers):
            l.prior = o.PRIOR_GAUSSIAN if k % 2 else o.PRIOR_CAUCHY
        eta = o.default_hypers(spec, 0.1)
    return spec, X, Y, theta, eta


def setenv(monkeypatch, fam):
    monkeypatch.setenv("TBNN_JIT_SKIP", SKIP[fam])
    if fam in ("wide", "layered", "generic"):
        monkeypatch.delenv("TBNN_FAST_GRID", raising=False)
    else:
        monkeypatch.setenv("TBNN_FAST_GRID", str(GRID))
    if fam in ("layered", "generic"):
        monkeypatch.setenv("TBNN_TALL", "0")
        monkeypatch.setenv("TBNN_REGISTERED", "0")        # nor a kernel library another module registered in this process


def make_chain(native, spec, fam, likelihood=None, **kw):
    lik = spec.likelihood if likelihood is None else likelihood
    if fam == "generic":
        ch = native.Chain(layers_of(spec), likelihood=lik, fixed_sd=spec.fixed_sd, kernel=native.KERNEL_GENERIC, **kw)
    else:
        ch = native.Chain(layers_of(spec), likelihood=lik, fixed_sd=spec.fixed_sd, jit=fam != "layered", **kw)
    assert ch.kernel_name.startswith(PREFIX[fam]), f"{fam}: runs on {ch.kernel_name}"
    return ch


FLOOR = 1e-30                     # of a tensor's inf-norm in tensor_err: none of these gradients is all but zero


def fwd_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(1.0, np.abs(want).max()))


def thrice(f):
    """f() three times: the results must be bit-identical; returns the first"""
    first = f()
    for _ in range(2):
        again = f()
        for a, b in zip(first, again):
            assert np.array_equal(np.asarray(a), np.asarray(b)), "a repeated launch differs"
    return first


def value_gradient_forward(native, spec, X, Y, theta, eta, fam):
    lp64, g64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[:2]
    th2 = np.stack([theta, (theta * np.float32(0.97)).astype(np.float32)])
    f64 = [o.forward(spec, t, X, np.float64) for t in th2]
    # the fp32 oracle inside the bounds first: the problem is conditioned well enough to judge the device
    lp32, g32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)[:2]
    assert abs(lp32 - lp64) <= LOGP_RTOL * max(abs(lp64), 1.0), ("fp32 oracle", lp32, lp64)
    assert tensor_err(spec, g32, g64, FLOOR) <= GRAD_TOL, ("fp32 oracle gradient", tensor_err(spec, g32, g64, FLOOR))
    assert fwd_err(o.forward(spec, theta, X, np.float32), f64[0]) <= FWD_TOL, "fp32 oracle forward"
    ch = make_chain(native, spec, fam)
    try:
        name = ch.kernel_name
        ch.set_data(X, Y)
        lp, g, _ = thrice(lambda: ch.logp_grad(theta, eta))
        f, pr, fm = thrice(lambda: (ch.forward(X, theta), ch.predict(0, theta), ch.forward_many(th2, None, which=0)))
    finally:
        ch.close()
    e_lp = abs(lp - lp64) / max(abs(lp64), 1.0)
    e_g = tensor_err(spec, g, g64, FLOOR)
    e_f = max(fwd_err(f, f64[0]), fwd_err(pr, f64[0]), fwd_err(fm[0], f64[0]), fwd_err(fm[1], f64[1]))
    print(f"{name}: logp {e_lp:.2e} ({LOGP_RTOL}) gradient per tensor {e_g:.2e} ({GRAD_TOL}) forward {e_f:.2e} ({FWD_TOL})")
    assert e_lp <= LOGP_RTOL, f"{name}: logp {lp} against {lp64} ({e_lp:.2e} relative)"
    assert e_g <= GRAD_TOL, f"{name}: gradient {e_g:.3e} of a tensor's inf-norm"
    assert e_f <= FWD_TOL, f"{name}: forward / predict / forward_many {e_f:.3e}"


@pytest.mark.parametrize("fam,tag,dims", CASES, ids=[_id(*c) for c in CASES])
def test_deep_value_gradient_forward(native, monkeypatch, fam, tag, dims):
    setenv(monkeypatch, fam)
    spec, X, Y, theta, eta = problem(dims, N_WIDE if fam == "wide" else N_ROWS)
    value_gradient_forward(native, spec, X, Y, theta, eta, fam)


@pytest.mark.parametrize("tail", ["1", "0"])
def test_layered_sixteen_narrow_layers_with_and_without_the_fused_tail(native, monkeypatch, tail):
    """k_lay_tail spans all 16 layers of a 16-wide network in one launch; TBNN_LAY_TAIL=0: one launch per layer and direction"""
    setenv(monkeypatch, "layered")
    monkeypatch.setenv("TBNN_LAY_TAIL", tail)
    spec, X, Y, theta, eta = problem(DEEP["layered"], N_ROWS + 2000, seed=1)
    value_gradient_forward(native, spec, X, Y, theta, eta, "layered")


@pytest.mark.parametrize("fam,tag,dims", CASES, ids=[_id(*c) for c in CASES])
def test_deep_transitions_traced(native, monkeypatch, fam, tag, dims):
    """an injected weight transition with its per-step energies, accepted and rejected, against o.weight_step"""
    setenv(monkeypatch, fam)
    spec, X, Y, theta, eta = problem(dims, N_ROWS, seed=2)
    rng = np.random.default_rng(len(dims))
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    eps, L = 5e-6, 3              # (the deep problems' gradients are large: a small step keeps the energy error, and its fp32 rounding, small)
    lp64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[0]
    ch = make_chain(native, spec, fam, seed=50, chain_id=2)
    try:
        ch.set_data(X, Y)
        for log_u in (-1e30, 1e30):
            def step():
                ch.set_state(theta); ch.set_hypers(eta)
                out = ch.hmc_step(eps, L, p0=p0, log_u=log_u, trace=True)
                return out["log_accept_ratio"], out["accepted"], out["trace_logp"], ch.get_state()
            lar, acc, tr, state = thrice(step)
            ref = o.weight_step(spec, theta, eta, X, Y, eps, L, p0, log_u, np.float64)
            e_tr = float(np.max(np.abs(np.asarray(tr) - ref.trace_logp) / np.maximum(np.abs(ref.trace_logp), 1.0)))
            assert e_tr <= LOGP_RTOL, (ch.kernel_name, e_tr)
            assert abs(lar - ref.log_accept_ratio) <= 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64), (lar, ref.log_accept_ratio)
            assert bool(acc) == ref.accepted
            assert np.abs(state - ref.theta).max() <= 1e-5 * max(1.0, np.abs(ref.theta).max())
            print(f"{ch.kernel_name} log_u {log_u:g}: trace {e_tr:.2e}, |d lar| {abs(lar - ref.log_accept_ratio):.2e}")
    finally:
        ch.close()


def test_deep_trajectory_kernel_against_the_per_step_path(native, monkeypatch):
    """a 9-layer narrow network within traj_max_rows: the whole trajectory in one launch against the per-step kernels and the oracle"""
    setenv(monkeypatch, "fast3")
    spec, X, Y, theta, eta = problem(TRAJ, 100, seed=3)
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    lp64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[0]
    for L in (1, 9):
        ref = o.weight_step(spec, theta, eta, X, Y, 2e-4, L, p0, -1e30, np.float64)
        got = {}
        for traj in (True, False):
            monkeypatch.setenv("TBNN_TRAJ", "1" if traj else "0")
            ch = make_chain(native, spec, "fast3")
            ch.set_data(X, Y)

            def step():
                ch.set_state(theta); ch.set_hypers(eta)
                out = ch.hmc_step(2e-4, L, p0=p0, log_u=-1e30)
                return out["log_accept_ratio"], ch.get_state()
            lar, state = thrice(step)
            assert ch.last_transition_path == ("trajectory" if traj else "per-step"), ch.last_transition_path
            ch.close()
            assert abs(lar - ref.log_accept_ratio) <= 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64), (traj, L)
            np.testing.assert_allclose(state, ref.theta, rtol=2e-5, atol=2e-6)
            got[traj] = state
        np.testing.assert_allclose(got[True], got[False], rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("fam,tag,dims", HYPER, ids=[_id(*c) for c in HYPER])
def test_deep_hyper_transition(native, monkeypatch, fam, tag, dims):
    """k_hyper's wave plan at 16, 18 and 32 prior groups, Cauchy and Gaussian layers alternating, the data term from the family's cached
    statistic: hyper_logp_grad against o.hyper_log_prob_and_grad, an injected hyper transition both ways against o.hyper_step"""
    setenv(monkeypatch, fam)
    spec, X, Y, theta, eta = problem(dims, N_ROWS, alternate=True, seed=4)
    assert spec.n_hypers == 4 * (len(dims) - 1) + 1
    rng = np.random.default_rng(3)
    eta2 = (eta + 0.05 * rng.standard_normal(eta.size)).astype(np.float32)
    ph = rng.standard_normal(spec.n_hypers).astype(np.float32)
    ch = make_chain(native, spec, fam)
    try:
        ch.set_data(X, Y); ch.set_state(theta); ch.set_hypers(eta)
        ch.logp_grad(theta, eta)                                     # the cached statistic the hyper target reads
        lp, g = thrice(lambda: ch.hyper_logp_grad(eta2))
        lp64, g64 = o.hyper_log_prob_and_grad(spec, eta2, theta, X, Y, np.float64)
        assert abs(lp - lp64) <= LOGP_RTOL * abs(lp64) + 1e-3, (lp, lp64)
        np.testing.assert_allclose(g, g64, rtol=2e-4, atol=1e-3 + 2e-6 * np.abs(g64).max())
        worst = 0.0
        for log_u in (-1e30, 1e30):
            def step():
                ch.set_state(theta); ch.set_hypers(eta)
                ch.logp_grad(theta, eta)
                out = ch.hyper_step(1e-4, 9, p0=ph, log_u=log_u)
                return out["log_accept_ratio"], out["accepted"], ch.get_hypers()
            lar, acc, hyp = thrice(step)
            ref = o.hyper_step(spec, eta, theta, X, Y, 1e-4, 9, ph, log_u, np.float64)
            worst = max(worst, abs(lar - ref.log_accept_ratio))
            assert abs(lar - ref.log_accept_ratio) <= 2e-2 + 1e-3 * abs(ref.log_accept_ratio), (lar, ref.log_accept_ratio)
            assert bool(acc) == ref.accepted
            np.testing.assert_allclose(hyp, ref.theta, rtol=1e-4, atol=1e-5)
        print(f"{ch.kernel_name}: hyper value {abs(lp - lp64) / abs(lp64):.2e} gradient {np.abs(g - g64).max():.2e} "
              f"(of {np.abs(g64).max():.2e}) |d lar| {worst:.2e}")
    finally:
        ch.close()


def test_sixteen_layer_group_is_the_solo_chains(native, monkeypatch):
    """a ChainGroup of 16-layer chains (per-chain H / P offsets in k_hyper, H = 65): its weight and hyper transitions bit for bit those of
    solo chains"""
    setenv(monkeypatch, "mid")
    spec, X, Y, theta, eta = problem(DEEP["mid"], N_ROWS, alternate=True, seed=5)
    C, c0, seed = 3, 7, 50
    rng = np.random.default_rng(2)
    thetas = (theta[None, :] * (1.0 + 0.05 * rng.standard_normal((C, theta.size)))).astype(np.float32)
    etas = np.tile(eta, (C, 1)).astype(np.float32) * (1.0 + 0.01 * np.arange(C, dtype=np.float32))[:, None]
    grp = native.ChainGroup(layers_of(spec), C, likelihood=spec.likelihood, seed=seed, chain_id=c0, jit=True)
    try:
        assert grp.kernel_name.startswith(PREFIX["mid"]), grp.kernel_name
        grp.set_data(X, Y); grp.set_state(thetas); grp.set_hypers(etas)
        g1 = grp.hmc_step(2e-5, 4)
        gh = grp.hyper_step(1e-4, 7)
        g2 = grp.hmc_step(2e-5, 3)
        g_state, g_hyp = grp.get_state(), grp.get_hypers()
    finally:
        grp.close()
    keys = ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new")
    for c in range(C):
        ch = native.Chain(layers_of(spec), likelihood=spec.likelihood, seed=seed, chain_id=c0 + c, jit=True)
        try:
            ch.set_data(X, Y); ch.set_state(thetas[c]); ch.set_hypers(etas[c])
            s1 = ch.hmc_step(2e-5, 4)
            sh = ch.hyper_step(1e-4, 7)
            s2 = ch.hmc_step(2e-5, 3)
            for got, want in ((g1[c], s1), (gh[c], sh), (g2[c], s2)):
                assert [got[k] for k in keys] == [want[k] for k in keys], (c, got, want)
            np.testing.assert_array_equal(g_state[c], ch.get_state())
            np.testing.assert_array_equal(g_hyp[c], ch.get_hypers())
        finally:
            ch.close()
    assert np.abs(g_hyp[0] - g_hyp[1]).max() > 0


def test_hyper_probs_many_sixteen_layers(native, monkeypatch):
    """k_hyper_probs over 16 layers, judged under per-layer priors, against o.layer_hyper_log_prob summed per network"""
    setenv(monkeypatch, "mid")
    dims = DEEP["mid"]
    spec, X, Y, theta, eta = problem(dims, 64, alternate=True, seed=6)
    judge = [o.PRIOR_CAUCHY if k % 3 else o.PRIOR_GAUSSIAN for k in range(len(spec.layers))]
    jspec = problem(dims, 64, seed=6)[0]
    for l, p in zip(jspec.layers, judge):
        l.prior = p
    rng = np.random.default_rng(17)
    m = 23
    thetas = (theta[None, :] * (1.0 + 0.2 * rng.standard_normal((m, theta.size)))).astype(np.float32)
    etas = (eta[None, :] * (1.0 + 0.05 * rng.standard_normal((m, eta.size))) + 0.01 * rng.standard_normal((m, eta.size))).astype(np.float32)
    ch = make_chain(native, spec, "mid")
    try:
        got = thrice(lambda: (ch.hyper_probs_many(thetas, etas, priors=judge),))[0]
    finally:
        ch.close()
    worst = 0.0
    for i in range(m):
        parts = o.unflatten(jspec, thetas[i].astype(np.float64))
        want = sum(float(o.layer_hyper_log_prob(l, etas[i, 4 * k:4 * k + 4].astype(np.float64), W, b, np.float64))
                   for k, (l, (W, b)) in enumerate(zip(jspec.layers, parts)))
        worst = max(worst, abs(got[i] - want) / abs(want))
        assert abs(got[i] - want) <= 4e-6 * abs(want) + 1e-6, (i, got[i], want)
    print(f"hyper_probs_many over 16 layers: {worst:.2e} relative")


@pytest.mark.parametrize("fam", list(MIXED))
def test_nine_mixed_hidden_activations(native, monkeypatch, fam):
    setenv(monkeypatch, fam)
    spec, X, Y, theta, eta = problem(MIXED[fam], N_WIDE if fam == "wide" else N_ROWS, acts=MIXED_ACTS, seed=7)
    from tensorbnn_amd import jit
    hact = jit.shape_of(layers_of(spec), spec.likelihood)[1]
    assert hact & jit.ACT_PACKED and (hact >> 24) & 7 == MIXED_ACTS[8]
    value_gradient_forward(native, spec, X, Y, theta, eta, fam)


def test_ten_mixed_hidden_activations_run_on_layered(native, monkeypatch):
    """the packed code holds nine hidden layers: ten go to the layered family, with a warning"""
    monkeypatch.delenv("TBNN_JIT_SKIP", raising=False)
    monkeypatch.delenv("TBNN_FAST_GRID", raising=False)
    spec, X, Y, theta, eta = problem(_stack(4, 16, 11, 1), N_ROWS, acts=MIXED_ACTS + [o.ACT_TANH], seed=8)
    with pytest.warns(RuntimeWarning, match="layered"):
        value_gradient_forward(native, spec, X, Y, theta, eta, "layered_jit")


@pytest.mark.parametrize("fam", list(CATEGORICAL))
def test_deep_categorical(native, monkeypatch, fam):
    """ten classes behind a deep mid and a deep wide stack: the softmax on the MFMA output tile"""
    setenv(monkeypatch, fam)
    dims = CATEGORICAL[fam]
    spec, X, Yg, theta, eta = problem(dims, N_ROWS, seed=9)
    spec.likelihood = o.LIK_CATEGORICAL
    eta = np.asarray(eta[:spec.n_hypers], dtype=np.float32)              # no likelihood hyper
    Y = np.eye(dims[-1], dtype=np.float32)[np.argmax(Yg, axis=1)]
    lp64, g64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)
    ch = make_chain(native, spec, fam, likelihood=o.LIK_CATEGORICAL)
    try:
        assert ",categorical;" in ch.kernel_name, ch.kernel_name
        ch.set_data(X, Y)
        lp, g, _ = thrice(lambda: ch.logp_grad(theta, eta))
        f = thrice(lambda: (ch.forward(X, theta),))[0]
    finally:
        ch.close()
    e_lp, e_g = abs(lp - lp64) / max(abs(lp64), 1.0), tensor_err(spec, g, g64, FLOOR)
    e_f = fwd_err(f, o.forward(spec, theta, X, np.float64))
    print(f"{fam} categorical: logp {e_lp:.2e} gradient per tensor {e_g:.2e} forward {e_f:.2e}")
    assert e_lp <= LOGP_RTOL and e_g <= GRAD_TOL and e_f <= FWD_TOL, (e_lp, e_g, e_f)


def jit_jobs():
    """the run-time instantiations this module asks for, as jit.prebuild takes them (tests/jit_shapes.json holds them)"""
    jobs = []

    def add(spec, fam, lik=None):
        if fam in ("layered", "generic"):
            return
        job = {"layers": [list(map(int, l)) for l in layers_of(spec)], "likelihood": int(spec.likelihood if lik is None else lik),
               "skip": SKIP[fam], "flags": ""}
        if job not in jobs:
            jobs.append(job)
    for fam, _t, dims in CASES + HYPER:
        add(problem(dims, 8)[0], fam)
    for fam, dims in MIXED.items():
        add(problem(dims, 8, acts=MIXED_ACTS)[0], fam)
    add(problem(TRAJ, 8)[0], "fast3")
    for fam, dims in CATEGORICAL.items():
        add(problem(dims, 8)[0], fam, o.LIK_CATEGORICAL)
    return jobs
