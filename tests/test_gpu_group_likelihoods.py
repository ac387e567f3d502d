"""GPU: chain groups (tbnn_create_multi) under the categorical and the Poisson likelihood and under row weights, on every kernel family.

The group modules (test_gpu_multichain.py and the group legs of the depth, mixed-activation, multi-output, one-hidden, trajectory and
free-running modules) run Gaussian, fixed-Gaussian and Bernoulli chains; the categorical, Poisson and row-weight modules run one-chain
handles (but for one narrow trainChains run each).  Here the two meet: a wrong chain offset in a likelihood path -- the statistic slot
pstat + c * PSTAT_CAP, chain c's eta, its weight image, its gradient slabs, its (eps, L) -- would leave chain 0 right and chains 1 onwards
plausibly wrong, and no solo test would notice.

Shapes: the CASES tables of test_gpu_categorical.py and test_gpu_poisson.py (imported, not restated; the run-time compiled libraries are
the ones those modules, test_gpu_row_weights.py and test_gpu_edges.py ask for) at reduced, ragged row counts (no multiple of 16) at which a
chain still spans several workgroups in x: 517 and 333 (narrow, mid: 64 rows per workgroup; generic: 256), 209 (tall: groups of at most 8 row
tiles; wide; layered).  Problems: the likelihood module's own problem_of / problem (the categorical module's `problem` takes its row count
from its table: its first rows are the problem of that many rows, synth_problem draws X row by row).

Cells, per likelihood (kernel family x likelihood path):
    Poisson:      fast3 (one output), fast3 (two outputs), fast (MFMA output tile), mid (VALU last layer), mid (MFMA output tile), tall,
                  wide (one output), wide (MFMA output tile), k_lay_tail, k_lay_last, k_lay_lik, generic
    categorical:  mid (MFMA output tile), tall (MFMA output tile), wide (MFMA output tile), k_lay_tail, k_lay_last, k_lay_lik, generic
Cells that cannot exist: categorical on fast3, on fast, on mid's / tall's / wide's VALU last layer (one or two outputs): cat_delta4 lives on
the MFMA output tile of 3 .. 16 outputs only (jit.families) -- such networks run on the layered family, which the three k_lay_* cells cover.
Left out on purpose: the Poisson module's large-rate case (the same kernel as mid10; its own band rule is therefore not reached here).

Per cell, with C = 4 chains, chain ids from 7 and a seed with a high word, every chain at its own perturbed theta (under Poisson: its last
layer scaled back by problem_of's own rule where the perturbation took a log-rate past 5) and its own eta:
  1. the group is its solo chains bit for bit over hmc_run, a diverging hmc_run (rejects; non-finite proposals under Poisson), a hyper
     transition, one more transition;
  2. every chain at its own (eps, L), one of them diverging, one at L = 1: bit for bit the solo chains, n_leapfrog included;
  3. the LAST chain's free-running transition against the fp64 oracle on its own Philox draws, at the bands of the likelihood module's
     test_transitions (log accept ratio 2e-2 + 1e-4 |lar| + 4e-7 |logp|, state 1e-5 of max(1, |theta|_inf), logp_old 4e-6 relative), the
     decision too: the oracle's own |lar - log u| exceeds 0.05 in every cell (asserted from the oracle alone; the smallest over the cells at EPOCH: 0.68).
     logp_old and the state are the sharp assertions there; see the test's docstring.  (Those modules keep their bands inline in their
     tests, so they are restated here, value for value, and not imported.)
The per-cell handles are created with TBNN_TRAJ=0: at these row counts the narrow shapes would otherwise take the one-launch trajectory
kernel, and the cell is about the per-step kernel its name says (asserted: last_transition_path).  The trajectory kernel has its own test.
Beyond the cells: one chain of four overflowing under Poisson (batched and chain-by-chain family); the trajectory kernel under Poisson and
Bernoulli with per-chain (eps, L) against solo chains, the oracle and the per-step kernels; weighted groups (a fused family with its
weighted library, and the layered fallback) against weighted solo chains and the oracle's w=, and back to unweighted."""
import numpy as np
import pytest

import tbnn_oracle as o
import test_gpu_categorical as cat
import test_gpu_edges as edges
import test_gpu_poisson as poi
import test_gpu_row_weights as rw
from tensor_checks import layers_of
from test_gpu_multichain import REC

pytestmark = pytest.mark.gpu

MOD = {"poisson": poi, "categorical": cat}
LIK = {"poisson": o.LIK_POISSON, "categorical": o.LIK_CATEGORICAL}
CELLS = [
    # likelihood, the case of that module's CASES, rows
    ("poisson", "fast3", 517), ("poisson", "fast3_two_outputs", 333), ("poisson", "fast", 333), ("poisson", "mid1", 517),
    ("poisson", "mid10", 333), ("poisson", "tall", 209), ("poisson", "wide1", 209), ("poisson", "wide10", 209),
    ("poisson", "lay_tail", 209), ("poisson", "lay_last", 209), ("poisson", "lay_separate", 209), ("poisson", "generic", 517),
    ("categorical", "mid10", 333), ("categorical", "tall10", 209), ("categorical", "wide10", 209), ("categorical", "lay_tail", 209),
    ("categorical", "lay_last", 209), ("categorical", "lay_separate", 209), ("categorical", "generic", 517),
]
IDS = [f"{lik}-{name}" for lik, name, _n in CELLS]
# weighted groups: a fused family with a registered weighted library, and the layered fallback
WEIGHTED = [("poisson", "fast3"), ("categorical", "mid10"), ("poisson", "lay_last"), ("categorical", "lay_tail")]

C, CID = 4, 7
SEED = (3 << 32) | 50                                        # the high word is folded into the Philox key: key1 = chain_id ^ (seed >> 32)
EPS, L = 3e-5, 4                                             # the step of both modules' test_transitions
EPOCH = 3                                                    # of the oracle transitions: chosen with SEED so that every cell has its margin
MARGIN = 0.05                                                # the oracle's |lar - log u| below which a decision is not compared
TRAJ_BERN = [2, 12, 1]                                       # test_gpu_edges.test_saturated_transition_on_the_trajectory_kernel's network


def jit_jobs():
    """the run-time instantiations this module loads: 15 jobs, 14 of them jobs of test_gpu_poisson.jit_jobs(), test_gpu_categorical.jit_jobs()
    or test_gpu_row_weights.jit_jobs().  The fifteenth, the narrow Bernoulli library of [2, 12, 1], belongs to test_gpu_edges, which has no
    jit_jobs() of its own: its shapes are listed in tests/jit_shapes.json, which the build compiles ahead, and that file is what this job
    was compared with"""
    jobs = []
    for lik, name, _n in CELLS:
        m = MOD[lik]
        dims, _rows, act, prior, fam = m.CASES[name][:5]
        if fam in m.FUSED:
            jobs.append(poi.job(m.spec_of(dims, act, prior), lik=LIK[lik], skip=m.FUSED[fam]))
    jobs.append(poi.job(poi.spec_of(*poi.TRAJ[:1], *poi.TRAJ[2:])))
    jobs.append(poi.job(traj_bern_spec(), lik=o.LIK_BERNOULLI, skip=edges.FAM["fast3"][0]))
    for lik, name in WEIGHTED:
        m = MOD[lik]
        dims, _rows, act, prior, fam = m.CASES[name][:5]
        if fam in m.FUSED:
            jobs.append(poi.job(m.spec_of(dims, act, prior), lik=LIK[lik], skip=m.FUSED[fam], weighted=True))
    return [j for i, j in enumerate(jobs) if j not in jobs[:i]]


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """this module's run-time shapes, before any test touches the GPU (cached by the modules that own them: nothing compiles here)"""
    from tensorbnn_amd import jit
    jobs = jit_jobs()
    assert len(jobs) <= 16
    assert jit.prebuild(jobs) == len(jobs)


_OPEN = []


@pytest.fixture(autouse=True)
def close_handles():
    """every handle a test opened is destroyed when it ends, passed or failed"""
    yield
    while _OPEN:
        _OPEN.pop().close()


def traj_bern_spec():
    return o.make_spec(TRAJ_BERN, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_BERNOULLI, o.ACT_SIGMOID)


_PROBLEMS = {}


def problem(lik, name, n):
    """(spec, X, Y, theta, eta) of a cell at n rows, computed once and shared (the arrays are read-only)"""
    key = (lik, name, n)
    if key not in _PROBLEMS:
        if lik == "poisson":
            dims, _rows, act, prior, _fam, _env, kind = poi.CASES[name]
            spec, X, Y, theta, eta = poi.problem_of(dims, n, act, prior, kind)
        else:
            spec, X, Y, theta, eta = cat.problem(name)
            X, Y = X[:n], Y[:n]
        out = (spec,) + tuple(np.ascontiguousarray(a) for a in (X, Y, theta, eta))
        for a in out[1:]:
            a.setflags(write=False)
        _PROBLEMS[key] = out
    return _PROBLEMS[key]


def chain_states(spec, X, theta, eta, n_chains, poisson):
    """every chain its own theta (a perturbed copy, as test_gpu_multichain.py) and its own eta (the base eta scaled per chain).  Poisson:
    where the perturbation carries a log-rate past 5, the chain's last layer is scaled back by problem_of's own rule, so that every chain
    stays in the range the Poisson module's bands were derived for"""
    rng = np.random.default_rng(2)
    thetas = (theta[None, :] * (1.0 + 0.05 * rng.standard_normal((n_chains, theta.size)))).astype(np.float32)
    if poisson:
        ow, _ob = spec.offsets()[-1]
        for c in range(n_chains):
            f = o.forward(spec, thetas[c].astype(np.float64), X.astype(np.float64), np.float64)
            if np.abs(f).max() > 5.0:
                thetas[c, ow:] = (thetas[c, ow:].astype(np.float64) * (5.0 / np.abs(f).max())).astype(np.float32)
            assert np.abs(o.forward(spec, thetas[c].astype(np.float64), X.astype(np.float64), np.float64)).max() <= 5.01
    etas = (np.tile(eta, (n_chains, 1)) * (1.0 + 0.01 * np.arange(n_chains))[:, None]).astype(np.float32)
    return thetas, etas


def open_handle(native, monkeypatch, lik, name, spec, n_chains=None, traj="0", **kw):
    """a ChainGroup of n_chains (None: a Chain) on the cell's kernel family, as the likelihood module's make_chain selects it; the kernel
    name is asserted"""
    m = MOD[lik]
    fam, env = m.CASES[name][4], m.CASES[name][5]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("TBNN_TRAJ", traj)
    make = native.Chain if n_chains is None else (lambda *a, **k: native.ChainGroup(a[0], n_chains, *a[1:], **k))
    if fam in m.FUSED:
        monkeypatch.setenv("TBNN_JIT_SKIP", m.FUSED[fam])
        h = make(layers_of(spec), likelihood=LIK[lik], jit=True, **kw)
        _OPEN.append(h)
        assert h.kernel_name.startswith(f"jit-{fam}<") and f",{lik};" in h.kernel_name, h.kernel_name
    elif fam == "layered":
        monkeypatch.setenv("TBNN_TALL", "0")
        monkeypatch.setenv("TBNN_REGISTERED", "0")
        h = make(layers_of(spec), likelihood=LIK[lik], jit=False, **kw)
        _OPEN.append(h)
        assert h.kernel_name.startswith("layered<"), h.kernel_name
    else:
        h = make(layers_of(spec), likelihood=LIK[lik], kernel=native.KERNEL_GENERIC, **kw)
        _OPEN.append(h)
        assert h.kernel_name == "generic", h.kernel_name
    assert h.H == 4 * len(spec.layers)                       # no likelihood hyper: H differs from the Gaussian handle's of the same layers
    return h


def rec(r):
    return np.array([r[k] for k in REC], dtype=np.float64)


def same_records(got, want, leapfrog=False):
    """transition records bit for bit (NaN == NaN: a diverged proposal's energies)"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(rec(g), rec(w))
        if leapfrog:
            assert g["n_leapfrog"] == w["n_leapfrog"]


def philox_key(chain):
    """(seed, chain_id) as tbnn_create folds the 64-bit seed into the 32-bit Philox key"""
    return SEED & 0xFFFFFFFF, (chain ^ (SEED >> 32)) & 0xFFFFFFFF


def oracle_transition(spec, theta, eta, X, Y, chain, epoch, eps, n_leapfrog, w=None):
    """the fp64 transition of chain `chain` at `epoch` on the device's own Philox draws; (result, log u, the oracle's |lar - log u|)"""
    k0, k1 = philox_key(chain)
    p0 = o.philox_normals(spec.n_params, k0, k1, epoch, o.PURPOSE_MOMENTUM)
    lu = float(o.philox_log_uniform(k0, k1, epoch, o.PURPOSE_LOGU))
    ref = o.weight_step(spec, theta, eta, X, Y, eps, n_leapfrog, p0, lu, np.float64, w=w)
    return ref, lu, abs(ref.log_accept_ratio - lu)


def lar_band(ref, lp64):
    """the log accept ratio's band of test_gpu_categorical / test_gpu_poisson / test_gpu_traj"""
    return 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)


# ------------------------------------------------------------------------------------------------------------------- 1. group == solo chains
@pytest.mark.parametrize("lik,name,n", CELLS, ids=IDS)
def test_group_chains_are_the_solo_chains(native, monkeypatch, lik, name, n):
    spec, X, Y, theta, eta = problem(lik, name, n)
    thetas, etas = chain_states(spec, X, theta, eta, C, lik == "poisson")

    def run(h):
        out = [h.hmc_run(EPS, L, 3), h.hmc_run(0.3, 3, 2), h.hyper_step(1e-4, 7), h.hmc_step(EPS, L)]
        assert h.last_transition_path == "per-step"
        return out

    grp = open_handle(native, monkeypatch, lik, name, spec, C, seed=SEED, chain_id=CID)
    grp.set_data(X, Y); grp.set_state(thetas); grp.set_hypers(etas)
    g1, g2, gh, g3 = run(grp)
    g_state, g_hyp, kname = grp.get_state(), grp.get_hypers(), grp.kernel_name
    grp.close()
    acc_seen = set()
    for c in range(C):
        ch = open_handle(native, monkeypatch, lik, name, spec, seed=SEED, chain_id=CID + c)
        assert ch.kernel_name == kname
        ch.set_data(X, Y); ch.set_state(thetas[c]); ch.set_hypers(etas[c])
        s1, s2, sh, s3 = run(ch)
        same_records(g1[c] + g2[c] + [gh[c], g3[c]], s1 + s2 + [sh, s3])
        acc_seen.update(int(r["accepted"]) for r in s1 + s2 + [s3])
        if lik == "poisson":                                 # the diverging run's proposals leave the fp32 range of exp
            assert all(r["log_accept_ratio"] == -np.inf and r["accepted"] == 0 for r in s2)
        np.testing.assert_array_equal(g_state[c], ch.get_state())
        np.testing.assert_array_equal(g_hyp[c], ch.get_hypers())
        ch.close()
    assert acc_seen == {0, 1}, acc_seen                      # both decisions occurred
    assert all(np.abs(g_state[a] - g_state[b]).max() > 0 for a in range(C) for b in range(a))      # and the chains are different chains
    assert np.all(np.isfinite(g_state)) and np.all(np.isfinite(g_hyp))


# ------------------------------------------------------------------------------------------------------------------- 2. own (eps, L) per chain
@pytest.mark.parametrize("lik,name,n", CELLS, ids=IDS)
def test_group_chains_at_their_own_step_size_and_leapfrog_count(native, monkeypatch, lik, name, n):
    """a chain past its own L is skipped while its neighbours go on (the batched kernels' blocks exit, the chain-by-chain backends skip it
    on the host): bit for bit the solo chain driven with its values"""
    spec, X, Y, theta, eta = problem(lik, name, n)
    thetas, etas = chain_states(spec, X, theta, eta, C, lik == "poisson")
    eps = np.array([EPS, 0.5 * EPS, 2.0 * EPS, 0.3], dtype=np.float32)              # (the last one diverges)
    Ls = np.array([3, 7, 1, 4], dtype=np.int32)
    eps_h = np.array([1e-4, 3e-4, 5e-5, 2e-4], dtype=np.float32)
    grp = open_handle(native, monkeypatch, lik, name, spec, C, seed=SEED, chain_id=CID)
    grp.set_data(X, Y); grp.set_state(thetas); grp.set_hypers(etas)
    g1 = grp.hmc_run_each(eps, Ls, 2)
    gh = grp.hyper_step_each(eps_h, 6)
    g2 = grp.hmc_step_each(eps[::-1].copy(), Ls[::-1].copy())
    assert grp.last_transition_path == "per-step"
    g_state, g_hyp = grp.get_state(), grp.get_hypers()
    grp.close()
    for c in range(C):
        ch = open_handle(native, monkeypatch, lik, name, spec, seed=SEED, chain_id=CID + c)
        ch.set_data(X, Y); ch.set_state(thetas[c]); ch.set_hypers(etas[c])
        s1 = ch.hmc_run(float(eps[c]), int(Ls[c]), 2)
        sh = ch.hyper_step(float(eps_h[c]), 6)
        s2 = ch.hmc_step(float(eps[C - 1 - c]), int(Ls[C - 1 - c]))
        same_records(g1[c] + [gh[c], g2[c]], s1 + [sh, s2], leapfrog=True)
        assert [r["n_leapfrog"] for r in g1[c]] == [int(Ls[c])] * 2 and g2[c]["n_leapfrog"] == int(Ls[C - 1 - c])
        np.testing.assert_array_equal(g_state[c], ch.get_state())
        np.testing.assert_array_equal(g_hyp[c], ch.get_hypers())
        ch.close()
    assert all(r["accepted"] == 0 for r in g1[C - 1]) and g2[0]["accepted"] == 0      # the diverging step size rejects
    assert any(r["accepted"] for c in range(C - 1) for r in g1[c])


# ------------------------------------------------------------------------------------------------------------------- 3. the last chain vs fp64
@pytest.mark.parametrize("lik,name,n", CELLS, ids=IDS)
def test_last_chain_against_the_oracle(native, monkeypatch, lik, name, n):
    """bit-equality with a solo chain proves nothing where both index wrongly alike: chain C - 1's free-running transition against fp64.

    What carries the weight at this step (EPS = 3e-5, L = 4, the likelihood modules' own): logp_old at 4e-6 relative -- chain C - 1's
    statistic slot, eta, weight image and targets -- and the state at 1e-5, which pins the chain's momentum draw (its Philox key) and, where
    the gradient's step eps^2 / 2 |g| reaches the tolerance, its gradient slabs.  The log accept ratio is below 0.04 in absolute value in
    every cell, against a band of 2e-2 and more, and every cell accepts with a margin of about |log u| (0.68 .. 0.73): these two assertions
    catch a chain that diverges or whose energies come from another chain's statistic slot (a slot perturbed on purpose shows in the log
    accept ratio first), not a small indexing error in the gradient.  Under the categorical likelihood the
    gradient's share of the state is below the state's tolerance: the gradient slabs of those cells rest on tests 1 and 2"""
    spec, X, Y, theta, eta = problem(lik, name, n)
    thetas, etas = chain_states(spec, X, theta, eta, C, lik == "poisson")
    c = C - 1
    ref, lu, margin = oracle_transition(spec, thetas[c], etas[c], X, Y, CID + c, EPOCH, EPS, L)
    lp64 = ref.logp_old
    print(f"[group] {lik}-{name}: oracle lar {ref.log_accept_ratio:.6g}, log u {lu:.6g}, margin {margin:.4g}, logp {lp64:.9g}")
    assert margin > MARGIN, (lik, name, margin)              # a precondition, from the oracle alone
    grp = open_handle(native, monkeypatch, lik, name, spec, C, seed=SEED, chain_id=CID)
    grp.set_data(X, Y); grp.set_state(thetas); grp.set_hypers(etas)
    grp.set_epoch(EPOCH)
    out = grp.hmc_step(EPS, L)[c]
    state = grp.get_state()[c]
    assert grp.last_transition_path == "per-step"
    print(f"[group] {lik}-{name}: device lar {out['log_accept_ratio']:.6g} (band {lar_band(ref, lp64):.3g}), logp_old {out['logp_old']:.9g}")
    assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= lar_band(ref, lp64)
    assert bool(out["accepted"]) == ref.accepted
    assert abs(out["logp_old"] - lp64) <= 4e-6 * max(abs(lp64), 1.0)
    assert np.abs(state - ref.theta).max() <= 1e-5 * max(1.0, np.abs(ref.theta).max())


# ------------------------------------------------------------------------------------------------------------------- 4. one chain overflows
@pytest.mark.parametrize("name", ["mid10", "lay_last"])          # a batched family and a chain-by-chain one
def test_one_chain_overflows_its_neighbours_do_not(native, monkeypatch, name):
    """Poisson: chain 2's last layer scaled until its state's log-rates reach 40 -- rates of 2e17, finite in fp32, whose gradient carries
    the first leapfrog position's log-rates far past log(FLT_MAX) = 88.7 (asserted on the fp64 oracle: the kick eps^2 / 2 g dwarfs the
    momentum draw).  That chain's log accept ratio is -inf and its state stays; chains 0, 1 and 3 are bit for bit those of the group in
    which chain 2 is well-behaved"""
    n = dict((nm, rows) for lk, nm, rows in CELLS if lk == "poisson")[name]
    spec, X, Y, theta, eta = problem("poisson", name, n)
    thetas, etas = chain_states(spec, X, theta, eta, C, True)
    X64 = X.astype(np.float64)
    bad = thetas.copy()
    ow, _ob = spec.offsets()[-1]
    f = o.forward(spec, bad[2].astype(np.float64), X64, np.float64)
    assert f.max() > 1.0
    bad[2, ow:] = (bad[2, ow:].astype(np.float64) * (40.0 / f.max())).astype(np.float32)
    # preconditions, from the oracle alone: the state is finite in fp32, the first leapfrog position of chain 2's own draw is not
    lp32, g32 = o.target_log_prob_and_grad(spec, bad[2], etas[2], X, Y, np.float32)
    assert np.isfinite(lp32) and np.all(np.isfinite(g32))
    k0, k1 = philox_key(CID + 2)
    p0 = o.philox_normals(spec.n_params, k0, k1, 0, o.PURPOSE_MOMENTUM).astype(np.float64)
    g64 = o.target_log_prob_and_grad(spec, bad[2], etas[2], X, Y, np.float64)[1]
    f1 = o.forward(spec, bad[2].astype(np.float64) + EPS * (p0 + 0.5 * EPS * g64), X64, np.float64)
    assert f1.max() > 1000.0
    runs = {}
    for tag, th in (("bad", bad), ("good", thetas)):
        grp = open_handle(native, monkeypatch, "poisson", name, spec, C, seed=SEED, chain_id=CID)
        grp.set_data(X, Y); grp.set_state(th); grp.set_hypers(etas)
        runs[tag] = ([grp.hmc_step(EPS, L), grp.hmc_step(EPS, L)], grp.get_state(), grp.get_hypers())
        grp.close()
    (b_rec, b_state, b_hyp), (g_rec, g_state, _g_hyp) = runs["bad"], runs["good"]
    for r in b_rec:
        assert r[2]["log_accept_ratio"] == -np.inf and r[2]["accepted"] == 0 and np.isfinite(r[2]["logp_old"])
    np.testing.assert_array_equal(b_state[2], bad[2])
    np.testing.assert_array_equal(b_hyp, etas)
    for c in (0, 1, 3):
        same_records([r[c] for r in b_rec], [r[c] for r in g_rec])
        assert all(np.isfinite(r[c]["log_accept_ratio"]) for r in b_rec)
        np.testing.assert_array_equal(b_state[c], g_state[c])
    assert any(r[c]["accepted"] for r in b_rec for c in (0, 1, 3))


# ------------------------------------------------------------------------------------------------------------------- 5. the trajectory kernel
def traj_problem(which):
    if which == "poisson":
        dims, _rows, act, prior = poi.TRAJ
        return (o.LIK_POISSON, "") + poi.problem_of(dims, 333, act, prior)
    spec = traj_bern_spec()
    _s, X, Y, theta, eta = o.synth_problem(TRAJ_BERN, 301, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_BERNOULLI)
    return (o.LIK_BERNOULLI, edges.FAM["fast3"][0], spec, X, Y, theta, eta)


@pytest.mark.parametrize("which", ["poisson", "bernoulli"])
def test_trajectory_kernel_group_at_its_own_step_sizes(native, monkeypatch, which):
    """whole trajectories in one launch (kernels_traj.hpp: one workgroup per chain, its StepCtl (eps, L)) under a non-Gaussian lik_delta:
    a group of three against its solo chains bit for bit, every chain against the oracle on its own Philox draws at test_gpu_traj.py's
    bands, and against the per-step kernels to rtol 2e-5, atol 2e-6"""
    lik, skip, spec, X, Y, theta, eta = traj_problem(which)
    assert X.shape[0] <= 380 and X.shape[0] % 16
    n_chains = 3
    thetas, etas = chain_states(spec, X, theta, eta, n_chains, which == "poisson")
    eps_c = np.array([2e-4, 3e-4, 1e-4], dtype=np.float32)
    L_c = np.array([5, 11, 8], dtype=np.int32)
    monkeypatch.setenv("TBNN_JIT_SKIP", skip)
    tag = ",poisson;" if which == "poisson" else ",sigmoid,bernoulli;"

    def run(traj, c=None):
        """the group (c None) or solo chain c: its first transition from EPOCH, the state after it, two more transitions, the last state"""
        monkeypatch.setenv("TBNN_TRAJ", "1" if traj else "0")
        if c is None:
            h = native.ChainGroup(layers_of(spec), n_chains, likelihood=lik, seed=SEED, chain_id=CID, jit=True)
        else:
            h = native.Chain(layers_of(spec), likelihood=lik, seed=SEED, chain_id=CID + c, jit=True)
        _OPEN.append(h)
        assert h.kernel_name.startswith("jit-fast3<") and tag in h.kernel_name, h.kernel_name
        h.set_data(X, Y)
        h.set_state(thetas if c is None else thetas[c]); h.set_hypers(etas if c is None else etas[c])
        h.set_epoch(EPOCH)
        out = h.hmc_step_each(eps_c, L_c) if c is None else h.hmc_step(float(eps_c[c]), int(L_c[c]))
        assert h.last_transition_path == ("trajectory" if traj else "per-step")
        first = h.get_state()
        more = h.hmc_run_each(eps_c, L_c, 2) if c is None else h.hmc_run(float(eps_c[c]), int(L_c[c]), 2)
        last = h.get_state()
        h.close()
        return out, first, more, last

    g_out, g_first, g_more, g_last = run(True)
    p_out, p_first, _p_more, _p_last = run(False)
    assert [r["n_leapfrog"] for r in g_out] == [int(x) for x in L_c]
    for c in range(n_chains):
        s_out, s_first, s_more, s_last = run(True, c)
        same_records([g_out[c]] + g_more[c], [s_out] + s_more, leapfrog=True)
        np.testing.assert_array_equal(g_first[c], s_first)
        np.testing.assert_array_equal(g_last[c], s_last)
        # the first transition against fp64
        ref, lu, margin = oracle_transition(spec, thetas[c], etas[c], X, Y, CID + c, EPOCH, float(eps_c[c]), int(L_c[c]))
        print(f"[group] trajectory {which} chain {c}: lar {s_out['log_accept_ratio']:.6g} (fp64 {ref.log_accept_ratio:.6g}), log u {lu:.6g}, margin {margin:.4g}")
        assert margin > MARGIN, (which, c, margin)           # a precondition, from the oracle alone
        assert abs(g_out[c]["log_accept_ratio"] - ref.log_accept_ratio) <= lar_band(ref, ref.logp_old), c
        assert bool(g_out[c]["accepted"]) == ref.accepted
        np.testing.assert_allclose(g_first[c], ref.theta, rtol=2e-5, atol=2e-6)
        # the per-step kernels sum the gradient in another order: the same transition to fp32 rounding
        assert p_out[c]["accepted"] == g_out[c]["accepted"]
    np.testing.assert_allclose(g_first, p_first, rtol=2e-5, atol=2e-6)
    assert all(np.abs(g_last[a] - g_last[b]).max() > 0 for a in range(n_chains) for b in range(a))


# ------------------------------------------------------------------------------------------------------------------- 6. weighted groups
@pytest.mark.parametrize("lik,name", WEIGHTED, ids=[f"{a}-{b}" for a, b in WEIGHTED])
def test_weighted_group(native, monkeypatch, lik, name):
    """tbnn_set_row_weights on a group: the weighted targets [Y | w] are one buffer all chains read.  The group against its weighted solo
    chains bit for bit, the last chain's logp_old against the oracle's w= at test_gpu_row_weights.py's band (4e-6), and after clearing
    the weights the unweighted solo chains again"""
    n = dict(((lk, nm), rows) for lk, nm, rows in CELLS)[(lik, name)]
    spec, X, Y, theta, eta = problem(lik, name, n)
    thetas, etas = chain_states(spec, X, theta, eta, C, lik == "poisson")
    w = rw.real_weights(n, 4)
    assert np.any(w == 0) and np.any(w != np.round(w))
    fused = MOD[lik].CASES[name][4] in MOD[lik].FUSED

    def run(h, th, et):
        h.set_state(th); h.set_hypers(et)
        h.set_epoch(0)
        out = [h.hmc_run(EPS, L, 2), h.hyper_step(1e-4, 5), h.hmc_step(EPS, 2)]
        assert h.last_transition_path == "per-step"
        return out, h.get_state(), h.get_hypers()

    grp = open_handle(native, monkeypatch, lik, name, spec, C, seed=SEED, chain_id=CID)
    grp.set_data(X, Y)
    plain = grp.kernel_name
    grp.set_row_weights(w)
    if fused:
        assert grp.kernel_name == plain.replace(";", ",weighted;", 1) and f",{lik},weighted;" in grp.kernel_name, grp.kernel_name
    else:
        assert grp.kernel_name == plain[:-1] + ",weighted>", grp.kernel_name
    (gw1, gwh, gw2), gw_state, gw_hyp = run(grp, thetas, etas)
    wname = grp.kernel_name
    grp.set_row_weights(None)
    assert grp.kernel_name == plain
    (gu1, guh, gu2), gu_state, gu_hyp = run(grp, thetas, etas)
    grp.close()
    for c in range(C):
        ch = open_handle(native, monkeypatch, lik, name, spec, seed=SEED, chain_id=CID + c)
        ch.set_data(X, Y)
        ch.set_row_weights(w)
        assert ch.kernel_name == wname
        (s1, sh, s2), s_state, s_hyp = run(ch, thetas[c], etas[c])
        same_records(gw1[c] + [gwh[c], gw2[c]], s1 + [sh, s2])
        np.testing.assert_array_equal(gw_state[c], s_state)
        np.testing.assert_array_equal(gw_hyp[c], s_hyp)
        ch.set_row_weights(None)
        assert ch.kernel_name == plain
        (s1, sh, s2), s_state, s_hyp = run(ch, thetas[c], etas[c])
        same_records(gu1[c] + [guh[c], gu2[c]], s1 + [sh, s2])
        np.testing.assert_array_equal(gu_state[c], s_state)
        np.testing.assert_array_equal(gu_hyp[c], s_hyp)
        ch.close()
    c = C - 1
    lp_w = o.target_log_prob_and_grad(spec, thetas[c], etas[c], X, Y, np.float64, w=w)[0]
    lp_u = o.target_log_prob_and_grad(spec, thetas[c], etas[c], X, Y, np.float64)[0]
    print(f"[group] weighted {lik}-{name}: logp_old {gw1[c][0]['logp_old']:.9g} (fp64 {lp_w:.9g}); unweighted {gu1[c][0]['logp_old']:.9g} (fp64 {lp_u:.9g})")
    assert abs(lp_w - lp_u) > 1e-3 * abs(lp_u)               # the weights matter
    assert abs(gw1[c][0]["logp_old"] - lp_w) <= 4e-6 * max(abs(lp_w), 1.0)
    assert abs(gu1[c][0]["logp_old"] - lp_u) <= 4e-6 * max(abs(lp_u), 1.0)
