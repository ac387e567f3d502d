"""GPU: every likelihood and the row weights where a wave walks many row tiles -- the cases of tests/many_tiles.py (which says why, and where
the shapes, libraries and problems come from).

Per case, on the small grid of TBNN_FAST_GRID (wide: enough rows): the kernel's name carries the family, the likelihood and `weighted`; the
launch really has the small grid (Chain.stat_partials); logp_grad three times bit for bit; value, statistic and gradient per tensor
against the fp64 oracle under the case's weights; then, on the same handle, the weights cleared (the unweighted fp64 target) and all-ones
weights (the unweighted result).  Per (family, likelihood): one injected, traced transition with both decisions against o.weight_step on
the per-step kernels.  A two-chain group on a weighted count-likelihood fast3 library against its solo chains, bit for bit.  The same rows
at the default grid and at the small one.

Bands: the project's -- value 4e-6 of max(|logp|, 1), gradient 1e-4 of each tensor's inf-norm (floor 1e-3), the statistic by its
likelihood module's rule (many_tiles.stat_gap); tests/test_many_tiles_host.py shows the oracle's fp32 arm inside half of each on every case.
Transitions: those of tests/test_gpu_update_paths.py (check_transition)."""
import numpy as np
import pytest

import many_tiles as mt
from tensor_checks import layers_of
from test_gpu_depth import thrice
from test_gpu_update_paths import check_transition

pytestmark = pytest.mark.gpu

SEED = 50
EPS, L = 2e-5, 3                          # the injected transitions (tests/test_gpu_row_weights.py's step)
KEYS = ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new")


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """this module's run-time shapes, before any test touches the GPU (the libraries of the modules that own the shapes: cached, a second
    run compiles nothing)"""
    from tensorbnn_amd import jit
    jobs = mt.jit_jobs()
    assert jit.prebuild(jobs, processes=16) == len(jobs)


_OPEN = []


@pytest.fixture(autouse=True)
def close_handles():
    """every handle a test opened is destroyed when it ends, passed or failed"""
    yield
    while _OPEN:
        _OPEN.pop().close()


def setenv(monkeypatch, c, grid=True):
    table = mt.OWNERS[c.owner][0]
    env = table[c.name][5]
    if isinstance(env, dict):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    monkeypatch.setenv("TBNN_JIT_SKIP", mt.skip_of(c))
    monkeypatch.setenv("TBNN_TRAJ", "0")
    if grid and c.grid is not None:
        monkeypatch.setenv("TBNN_FAST_GRID", str(c.grid))      # read when the rows (or the weights) are staged
    else:
        monkeypatch.delenv("TBNN_FAST_GRID", raising=False)


def open_handle(native, monkeypatch, c, n_chains=None, grid=True, **kw):
    setenv(monkeypatch, c, grid)
    spec = mt.spec_of(c)
    kw = dict(likelihood=spec.likelihood, fixed_sd=spec.fixed_sd, lik_df=spec.lik_df, jit=True, **kw)
    h = native.Chain(layers_of(spec), **kw) if n_chains is None else native.ChainGroup(layers_of(spec), n_chains, **kw)
    _OPEN.append(h)
    return h


def check_name(h, c, weighted):
    """family, likelihood tag and `weighted` (csrc/fused_ops.hpp: prefix<hidden,last[,likelihood][,weighted];dims>)"""
    name = h.kernel_name
    if mt.aot(c) and not weighted:
        assert name == "fast3<relu;5,50,50,50,1>", name                  # the ahead-of-time table
        return
    assert name.startswith((f"jit-{c.family}<", f"jit-{c.family}(")), (c.id, name)
    tokens = name[name.index("<") + 1:name.index(";")].split(",")
    want = ([mt.TAG[c.lik]] if mt.TAG[c.lik] else []) + (["weighted"] if weighted else [])
    assert tokens[2:] == want, (c.id, name)


def check_grid(h, c):
    if c.grid is not None:
        assert h.stat_partials == c.grid < mt.default_grid(c), (c.id, h.stat_partials)


def judge(c, spec, what, got, ref):
    lp, g, st = got
    ev, eg, es = mt.gaps(c, spec, lp, g, st, ref)
    print(f"[many-tiles] {c.id} {what}: over the band: value {ev:.3f} gradient {eg:.3f} statistic {es:.3f}")
    assert np.isfinite(lp) and np.isfinite(st) and np.all(np.isfinite(g)), (c.id, what)
    assert ev <= 1.0, (c.id, what, "value", lp, ref[0])
    assert eg <= 1.0, (c.id, what, "gradient", eg)
    assert es <= 1.0, (c.id, what, "statistic", st, ref[2])


@pytest.mark.parametrize("cid", list(mt.BY_ID))
def test_value_statistic_gradient(native, monkeypatch, cid):
    c = mt.BY_ID[cid]
    spec, X, Y, theta, eta = mt.problem(c)
    ch = open_handle(native, monkeypatch, c)
    ch.set_data(X, Y)
    check_name(ch, c, False)
    if c.weighted:
        ch.set_row_weights(mt.weights(c))
    check_name(ch, c, c.weighted)
    check_grid(ch, c)
    judge(c, spec, "weighted" if c.weighted else "plain", thrice(lambda: ch.logp_grad(theta, eta)), mt.ref64(c))
    if not c.weighted:
        return
    # the same handle: the weights cleared, then all-ones weights
    ch.set_row_weights(None)
    check_name(ch, c, False)
    check_grid(ch, c)
    plain = thrice(lambda: ch.logp_grad(theta, eta))
    judge(c, spec, "weights cleared", plain, mt.ref64(c, False))
    ch.set_row_weights(np.ones(c.rows, np.float32))
    check_name(ch, c, True)
    check_grid(ch, c)
    judge(c, spec, "weights of one against the unweighted result", thrice(lambda: ch.logp_grad(theta, eta)),
          (plain[0], plain[1].astype(np.float64), plain[2]))


def _first_per_family_and_likelihood():
    seen, out = set(), []
    for c in mt.CASES:
        if not c.weighted and (c.family, c.lik) not in seen:
            seen.add((c.family, c.lik))
            out.append(c.id)
    return out


@pytest.mark.parametrize("cid", _first_per_family_and_likelihood())
def test_transition(native, monkeypatch, cid):
    """an injected transition of L = 3, accepted and rejected, with its per-step energies against o.weight_step"""
    c = mt.BY_ID[cid]
    spec, X, Y, theta, eta = mt.problem(c)
    p0 = np.random.default_rng(4).standard_normal(spec.n_params).astype(np.float32)
    ch = open_handle(native, monkeypatch, c, seed=SEED, chain_id=2)
    ch.set_data(X, Y)
    check_name(ch, c, False)
    check_grid(ch, c)
    check_transition(ch, spec, X, Y, theta, eta, EPS, L, p0, lambda _ch: eta, c.id)
    assert ch.last_transition_path == "per-step"


def test_two_chain_group_is_the_solo_chains(native, monkeypatch):
    """gridDim.y = 2 on the weighted Poisson fast3 library at 381 rows: blockIdx.y's offsets meet Wq -- each chain's records and state bit
    for bit the solo chain's"""
    c = mt.BY_ID["fast3-valu1-poisson-weighted-381rows"]
    spec, X, Y, theta, eta = mt.problem(c)
    w = mt.weights(c)
    nc, c0 = 2, 3
    rng = np.random.default_rng(4)
    thetas = (theta[None, :] * (1.0 + 0.01 * rng.standard_normal((nc, theta.size)))).astype(np.float32)
    etas = (np.tile(eta, (nc, 1)) * (1.0 + 0.01 * np.arange(nc))[:, None]).astype(np.float32)

    def run(h, th, et):
        h.set_data(X, Y)
        h.set_row_weights(w)
        check_name(h, c, True)
        check_grid(h, c)
        h.set_state(th); h.set_hypers(et)
        recs = [h.hmc_step(EPS, L) for _ in range(2)]
        assert h.last_transition_path == "per-step"
        return recs, h.get_state()

    g_recs, g_state = run(open_handle(native, monkeypatch, c, n_chains=nc, seed=SEED, chain_id=c0), thetas, etas)
    g_state = g_state.reshape(nc, -1)
    for k in range(nc):
        s_recs, s_state = run(open_handle(native, monkeypatch, c, seed=SEED, chain_id=c0 + k), thetas[k], etas[k])
        for gr, sr_ in zip(g_recs, s_recs):
            assert [gr[k][key] for key in KEYS] == [sr_[key] for key in KEYS], (k, gr[k], sr_)
        np.testing.assert_array_equal(g_state[k], s_state)
    assert np.abs(g_state[0] - g_state[1]).max() > 0


@pytest.mark.parametrize("cid", ["fast3-valu1-student-weighted-381rows", "fast-valu2-gaussian-weighted-381rows",
                                 "mid-mfma10-categorical-weighted-381rows", "tall-valu1-gaussian-weighted-1007rows",
                                 "fast-valu1-gamma-weighted-381rows", "mid-mfma10-gamma-weighted-381rows"])
def test_default_grid_and_small_grid(native, monkeypatch, cid):
    """the same rows and weights on the launch the library sizes itself and on the small one: both inside the bands, and the second one
    really small"""
    c = mt.BY_ID[cid]
    spec, X, Y, theta, eta = mt.problem(c)
    ch = open_handle(native, monkeypatch, c, grid=False)
    ch.set_data(X, Y)
    ch.set_row_weights(mt.weights(c))
    check_name(ch, c, True)
    assert ch.stat_partials == mt.default_grid(c) > c.grid, (cid, ch.stat_partials)
    big = thrice(lambda: ch.logp_grad(theta, eta))
    judge(c, spec, f"{ch.stat_partials} workgroups", big, mt.ref64(c))
    monkeypatch.setenv("TBNN_FAST_GRID", str(c.grid))
    ch.set_data(X, Y)
    ch.set_row_weights(mt.weights(c))
    assert ch.stat_partials == c.grid, (cid, ch.stat_partials)
    small = thrice(lambda: ch.logp_grad(theta, eta))
    judge(c, spec, f"{ch.stat_partials} workgroups", small, mt.ref64(c))
