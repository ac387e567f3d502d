"""GPU: per-row likelihood weights (tbnn_set_row_weights) on every kernel family -- narrow fast3 and fast, mid, tall, wide, the layered
family on each of its likelihood kernels (k_lay_tail, k_lay_last, k_lay_lik) and the generic kernel -- with the Gaussian, Bernoulli and
categorical likelihoods.  All-ones weights against the unweighted handle bit for bit (value, gradient, a traced injected weight transition,
an injected hyper transition); integer weights against the rows repeated; real weights against the fp64 oracle's weighted targets
(o.target_log_prob_and_grad and o.hyper_step with w=: value, gradient per tensor, a Gaussian hyper transition that depends on the
weighted S and on W); the
refusals of bad weights, of a TBNN_KERNEL_FAST handle without a weighted table (which keeps its kernels) and of row sharding in either
order; clearing, and set_data dropping them; an untraced small weighted problem on the per-step kernels; several chains behind one handle
against solo chains; trainChains against solo train runs; an imbalanced Bernoulli fit."""
import numpy as np
import pytest

import tbnn_oracle as o
from tensor_checks import layers_of, tensor_err
from test_gpu_freerun import SEED

pytestmark = pytest.mark.gpu

NARROW3, NARROW = "fast,mid,tall,wide", "fast3,mid,tall,wide"
MID, TALL, WIDE = "fast3,fast,tall,wide", "fast3,fast,mid,wide", "fast3,fast,mid,tall"

CASES = {
    # dims, rows, hidden activation, likelihood, family, TBNN_JIT_SKIP / layered environment
    "fast3_configs1": ([5, 50, 50, 50, 1], 3001, o.ACT_RELU, o.LIK_GAUSSIAN, "fast3", NARROW3),   # the unweighted side: the ahead-of-time table
    "fast3_bern": ([4, 32, 32, 1], 2001, o.ACT_TANH, o.LIK_BERNOULLI, "fast3", NARROW3),
    "fast_gauss": ([4, 24, 24, 2], 1001, o.ACT_RELU, o.LIK_GAUSSIAN, "fast", NARROW),
    "fast_bern": ([4, 24, 24, 2], 1001, o.ACT_RELU, o.LIK_BERNOULLI, "fast", NARROW),
    "mid_gauss": ([30, 80, 80, 10], 3001, o.ACT_RELU, o.LIK_GAUSSIAN, "mid", MID),
    "mid_bern": ([20, 64, 64, 2], 1999, o.ACT_RELU, o.LIK_BERNOULLI, "mid", MID),
    "mid_cat": ([30, 80, 80, 10], 3001, o.ACT_RELU, o.LIK_CATEGORICAL, "mid", MID),
    "tall_gauss": ([784, 20, 20, 1], 1205, o.ACT_RELU, o.LIK_GAUSSIAN, "tall", TALL),
    "tall_cat": ([784, 20, 20, 10], 1205, o.ACT_RELU, o.LIK_CATEGORICAL, "tall", TALL),
    "tall_bern": ([784, 20, 20, 2], 1205, o.ACT_RELU, o.LIK_BERNOULLI, "tall", TALL),
    "wide_gauss": ([10, 200, 200, 10], 3001, o.ACT_RELU, o.LIK_GAUSSIAN, "wide", WIDE),
    "wide_cat": ([10, 200, 200, 10], 3001, o.ACT_RELU, o.LIK_CATEGORICAL, "wide", WIDE),
    "wide_bern": ([10, 200, 200, 2], 3001, o.ACT_RELU, o.LIK_BERNOULLI, "wide", WIDE),
    "lay_tail_gauss": ([784, 20, 20, 10], 1205, o.ACT_RELU, o.LIK_GAUSSIAN, "layered", {}),                      # k_lay_tail
    "lay_tail_bern": ([784, 20, 20, 10], 1205, o.ACT_RELU, o.LIK_BERNOULLI, "layered", {}),
    "lay_tail_cat": ([784, 20, 20, 10], 1205, o.ACT_RELU, o.LIK_CATEGORICAL, "layered", {}),                              # cat_delta<TT, true>
    "lay_tail_cat_k20": ([9, 30, 20], 450, o.ACT_TANH, o.LIK_CATEGORICAL, "layered", {}),                                # k_lay_tail, two tiles
    "lay_last_cat": ([784, 100, 100, 10], 1205, o.ACT_RELU, o.LIK_CATEGORICAL, "layered", {}),                             # k_lay_last
    "lay_last_gauss": ([784, 100, 100, 10], 1205, o.ACT_RELU, o.LIK_GAUSSIAN, "layered", {}),
    "lay_last_bern": ([784, 100, 100, 10], 1205, o.ACT_RELU, o.LIK_BERNOULLI, "layered", {}),
    "lay_lik_gauss": ([784, 100, 100, 10], 1205, o.ACT_RELU, o.LIK_GAUSSIAN, "layered", {"TBNN_LAY_LAST": "0"}),  # k_lay_lik
    "lay_lik_bern": ([784, 100, 100, 10], 1205, o.ACT_RELU, o.LIK_BERNOULLI, "layered", {"TBNN_LAY_LAST": "0"}),  # k_lay_lik
    "lay_lik_cat": ([20, 64, 64, 20], 1500, o.ACT_TANH, o.LIK_CATEGORICAL, "layered", {}),                                 # k_lay_lik, K > 16
    "generic_gauss": ([5, 16, 16, 4], 517, o.ACT_TANH, o.LIK_GAUSSIAN, "generic", {}),
    "generic_bern": ([5, 16, 16, 1], 517, o.ACT_TANH, o.LIK_BERNOULLI, "generic", {}),
    "generic_cat": ([5, 16, 16, 4], 517, o.ACT_TANH, o.LIK_CATEGORICAL, "generic", {}),
}


def spec_of(name):
    dims, _n, act, lik, _f, _e = CASES[name]
    final = o.ACT_SIGMOID if lik == o.LIK_BERNOULLI else o.ACT_NONE
    return o.make_spec(dims, act, o.PRIOR_CAUCHY, lik, final)


def jit_jobs():
    """the run-time instantiations this module asks for (jit.prebuild's job format): both sides of every fused case"""
    jobs = []
    for name, (dims, _n, act, lik, fam, skip) in CASES.items():
        if fam in ("layered", "generic"):
            continue
        layers = [list(l) for l in layers_of(spec_of(name))]
        jobs.append({"layers": layers, "likelihood": lik, "skip": skip, "flags": "", "weighted": True})
        if name != "fast3_configs1":
            jobs.append({"layers": layers, "likelihood": lik, "skip": skip, "flags": ""})
    for spec, lik in ((blob_spec(), o.LIK_CATEGORICAL), (bern_spec(), o.LIK_BERNOULLI)):
        for w in (True, False):
            jobs.append({"layers": [list(l) for l in layers_of(spec)], "likelihood": lik, "skip": "", "flags": "", "weighted": w})
    jobs.append({"layers": [list(l) for l in layers_of(traj_spec())], "likelihood": o.LIK_GAUSSIAN, "skip": NARROW3, "flags": "", "weighted": True})
    return jobs


def traj_spec():
    """configs[0]: a small problem the unweighted ahead-of-time table runs on the trajectory kernel"""
    return o.make_spec([1, 10, 10, 1], o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, o.ACT_NONE)


def blob_spec():
    return o.make_spec([2, 16, 16, 3], o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_CATEGORICAL, o.ACT_NONE)


def bern_spec():
    return o.make_spec([2, 16, 16, 1], o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_BERNOULLI, o.ACT_SIGMOID)


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """compile this module's run-time shapes side by side before any test touches the GPU (cached: a second run compiles nothing)"""
    from tensorbnn_amd import jit
    jobs = jit_jobs()
    assert jit.prebuild(jobs) == len(jobs)


def problem(name, n=None):
    dims, rows, act, lik, _f, _e = CASES[name]
    n = rows if n is None else n
    _s, X, Y, theta, eta = o.synth_problem(dims, n, act, o.PRIOR_CAUCHY, o.LIK_BERNOULLI if lik == o.LIK_BERNOULLI else o.LIK_GAUSSIAN)
    spec = spec_of(name)
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1)
    if lik == o.LIK_CATEGORICAL:
        Y = np.eye(dims[-1], dtype=np.float32)[np.argmax(Y, axis=1)]
        eta = eta[:spec.n_hypers]
    return spec, X, np.asarray(Y, np.float32), theta, np.asarray(eta, np.float32)


_OPEN = []


@pytest.fixture(autouse=True)
def close_chains():
    """every handle a test opened is destroyed when it ends, passed or failed (not at interpreter exit)"""
    yield
    while _OPEN:
        _OPEN.pop().close()


def make_chain(native, monkeypatch, name, weighted, **kw):
    """a chain on the case's family; weighted: ITS weighted table (set_row_weights registers it) -- the caller sets the weights"""
    _d, _n, _a, lik, fam, env = CASES[name]
    spec = spec_of(name)
    if fam in ("layered", "generic"):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("TBNN_TALL", "0")
        monkeypatch.setenv("TBNN_REGISTERED", "0")
        kern = native.KERNEL_GENERIC if fam == "generic" else native.KERNEL_AUTO
        ch = native.Chain(layers_of(spec), likelihood=lik, jit=False, kernel=kern, **kw)
    else:
        monkeypatch.setenv("TBNN_JIT_SKIP", env)
        ch = native.Chain(layers_of(spec), likelihood=lik, jit=True, **kw)
    _OPEN.append(ch)
    return ch


TIMING = ("device_us", "fwdbwd_us")          # wall-clock fields of a transition record


def record(out):
    return {k: v for k, v in out.items() if k not in TIMING}


def check_family(name, ch_u, ch_w):
    fam = CASES[name][4]
    ku, kw = ch_u.kernel_name, ch_w.kernel_name
    if fam == "layered":
        assert ku.startswith("layered<") and kw == ku[:-1] + ",weighted>", (ku, kw)
    elif fam == "generic":
        assert ku == "generic" and kw == "generic<weighted>", (ku, kw)
    elif name == "fast3_configs1":
        assert ku == "fast3<relu;5,50,50,50,1>" and kw.startswith("jit-fast3<") and ",weighted;" in kw, (ku, kw)
    else:
        assert kw.startswith(f"jit-{fam}") and kw.replace(",weighted", "") == ku, (ku, kw)


def both(native, monkeypatch, name, X, Y, w, **kw):
    ch_u = make_chain(native, monkeypatch, name, False, **kw)
    ch_w = make_chain(native, monkeypatch, name, True, **kw)
    ch_u.set_data(X, Y)
    ch_w.set_data(X, Y)
    ch_w.set_row_weights(w)
    return ch_u, ch_w


@pytest.mark.parametrize("name", list(CASES))
def test_ones_equal_unweighted_bit_for_bit(native, monkeypatch, name):
    spec, X, Y, theta, eta = problem(name)
    ch_u, ch_w = both(native, monkeypatch, name, X, Y, np.ones(len(X), np.float32), seed=SEED, chain_id=3)
    check_family(name, ch_u, ch_w)
    lu, gu, su = ch_u.logp_grad(theta, eta)
    lw, gw, sw = ch_w.logp_grad(theta, eta)
    assert lu == lw and su == sw and np.array_equal(gu, gw), (name, lu, lw)
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    for ch in (ch_u, ch_w):
        ch.set_state(theta); ch.set_hypers(eta)
    ou = ch_u.hmc_step(2e-5, 3, p0=p0, log_u=-0.5, trace=True)
    ow = ch_w.hmc_step(2e-5, 3, p0=p0, log_u=-0.5, trace=True)
    assert ch_w.last_transition_path == "per-step"
    tu, tw = ou.pop("trace_logp"), ow.pop("trace_logp")
    assert np.array_equal(tu, tw) and record(ou) == record(ow), (name, ou, ow)
    assert np.array_equal(ch_u.get_state(), ch_w.get_state())
    ph = rng.standard_normal(len(eta)).astype(np.float32)
    hu, hw = ch_u.hyper_step(1e-3, 3, p0=ph, log_u=-0.5), ch_w.hyper_step(1e-3, 3, p0=ph, log_u=-0.5)
    assert record(hu) == record(hw) and np.array_equal(ch_u.get_hypers(), ch_w.get_hypers()), (name, hu, hw)
    ch_u.close(); ch_w.close()


def test_untraced_weighted_transition_takes_the_per_step_kernels(native, monkeypatch):
    """a small narrow problem: untraced, the unweighted handle takes the trajectory kernel, the weighted one (no trajectory kernel in a
    weighted table) the per-step kernels"""
    spec = traj_spec()
    _s, X, Y, theta, eta = o.synth_problem([1, 10, 10, 1], 1000, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN)
    monkeypatch.setenv("TBNN_TRAJ", "1")
    monkeypatch.setenv("TBNN_JIT_SKIP", NARROW3)
    chs = [native.Chain(layers_of(spec), likelihood=o.LIK_GAUSSIAN, jit=True, seed=SEED, chain_id=1) for _ in range(2)]
    _OPEN.extend(chs)
    ch_u, ch_w = chs
    for ch in chs:
        ch.set_data(X, Y); ch.set_state(theta); ch.set_hypers(eta)
    ch_w.set_row_weights(np.random.default_rng(2).gamma(0.7, 1.5, len(X)).astype(np.float32))
    assert ch_u.kernel_name == "fast3<relu;1,10,10,1>" and ch_w.kernel_name.startswith("jit-fast3<") and ",weighted;" in ch_w.kernel_name
    ch_u.hmc_step(3e-4, 10)
    ch_w.hmc_step(3e-4, 10)
    assert ch_u.last_transition_path == "trajectory"
    assert ch_w.last_transition_path == "per-step"
    rec = ch_w.hmc_run(3e-4, 10, 3)
    assert ch_w.last_transition_path == "per-step" and all(np.isfinite(r["log_accept_ratio"]) for r in rec)


def test_refused_fast_handle_keeps_its_kernels(native, monkeypatch):
    """TBNN_KERNEL_FAST and no weighted table to select (TBNN_REGISTERED=0): the call is refused and the handle stays as it was -- its
    kernel, and its unweighted value and gradient bit for bit"""
    from tensorbnn_amd._native import TbnnError
    name = "fast3_configs1"
    spec, X, Y, theta, eta = problem(name, 2000)
    monkeypatch.setenv("TBNN_REGISTERED", "0")
    ch = native.Chain(layers_of(spec), likelihood=o.LIK_GAUSSIAN, kernel=native.KERNEL_FAST, jit=False, seed=SEED, chain_id=1)
    _OPEN.append(ch)
    ch.set_data(X, Y)
    base = ch.kernel_name
    l0, g0, s0 = ch.logp_grad(theta, eta)
    with pytest.raises(TbnnError, match="TBNN_KERNEL_FAST"):
        ch.set_row_weights(real_weights(len(X)))
    assert ch.kernel_name == base and not ch.row_weighted
    l1, g1, s1 = ch.logp_grad(theta, eta)
    assert l1 == l0 and s1 == s0 and np.array_equal(g1, g0)
    ch.set_state(theta); ch.set_hypers(eta)
    out = ch.hmc_step(2e-5, 3)
    assert np.isfinite(out["log_accept_ratio"]) and np.all(np.isfinite(ch.get_state()))


@pytest.mark.parametrize("name", ["fast3_configs1", "fast_gauss", "mid_bern", "mid_cat", "tall_gauss", "wide_cat", "lay_tail_bern",
                                  "lay_last_cat", "lay_lik_bern", "generic_gauss"])
def test_integer_weights_equal_repeated_rows(native, monkeypatch, name):
    spec, X, Y, theta, eta = problem(name)
    w = np.random.default_rng(11).integers(0, 4, len(X)).astype(np.float32)
    w[0] = 2.0
    Xr, Yr = np.repeat(X, w.astype(int), axis=0), np.repeat(Y, w.astype(int), axis=0)
    ch_w = make_chain(native, monkeypatch, name, True, seed=SEED, chain_id=1)
    ch_w.set_data(X, Y)
    ch_w.set_row_weights(w)
    ch_r = make_chain(native, monkeypatch, name, False, seed=SEED, chain_id=1)
    ch_r.set_data(Xr, Yr)
    lw, gw, _ = ch_w.logp_grad(theta, eta)
    lr, gr, _ = ch_r.logp_grad(theta, eta)
    assert abs(lw - lr) <= 1e-5 * max(abs(lr), 1.0), (name, lw, lr)
    assert tensor_err(spec, gw, gr, 1e-3) <= 1e-4, name
    p0 = np.random.default_rng(6).standard_normal(spec.n_params).astype(np.float32)
    for log_u in (-1e30, 1e30):
        for ch in (ch_w, ch_r):
            ch.set_state(theta); ch.set_hypers(eta)
        a, b = ch_w.hmc_step(2e-5, 3, p0=p0, log_u=log_u), ch_r.hmc_step(2e-5, 3, p0=p0, log_u=log_u)
        assert a["accepted"] == b["accepted"] == (log_u < 0)
    ch_w.close(); ch_r.close()


def real_weights(n, seed=3):
    w = np.random.default_rng(seed).gamma(0.7, 1.5, n).astype(np.float32)
    w[::7] = 0.0                                   # zero-weight rows add nothing
    return w


# (mid_bern saturates: rows whose fp32 sigmoid lands past the clip bound have no gradient in fp32 and a huge one in fp64 -- the unweighted
# kernels' own behaviour at the clip edge; its weighting is checked against repeated rows and all-ones weights above)
@pytest.mark.parametrize("name", ["fast3_configs1", "fast3_bern", "fast_gauss", "mid_gauss", "mid_cat", "tall_gauss", "tall_cat",
                                  "wide_gauss", "wide_cat", "lay_tail_gauss", "lay_tail_cat", "lay_tail_cat_k20", "lay_last_cat",
                                  "lay_lik_bern", "lay_lik_gauss", "lay_lik_cat", "generic_bern", "generic_cat"])
def test_real_weights_against_fp64(native, monkeypatch, name):
    spec, X, Y, theta, eta = problem(name)
    w = real_weights(len(X))
    ch = make_chain(native, monkeypatch, name, True)
    ch.set_data(X, Y)
    ch.set_row_weights(w)
    assert "weighted" in ch.kernel_name
    lp, g, _ = ch.logp_grad(theta, eta)
    assert np.array_equal(g, ch.logp_grad(theta, eta)[1])
    lp64, g64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64, w=w)
    assert np.isfinite(lp) and abs(lp - lp64) <= 4e-6 * max(abs(lp64), 1.0), (name, lp, lp64)
    assert tensor_err(spec, g, g64, 1e-3) <= 1e-4, name
    ch.close()


@pytest.mark.parametrize("name", ["mid_gauss", "lay_tail_gauss", "generic_gauss"])
def test_weighted_gaussian_hyper_transition(native, monkeypatch, name):
    """the hyper transition's data term: the S cached by the weight transition (sum w r^2) and W in place of the row count"""
    spec, X, Y, theta, eta = problem(name)
    w = real_weights(len(X), 9)
    ch = make_chain(native, monkeypatch, name, True, seed=SEED, chain_id=2)
    ch.set_data(X, Y)
    ch.set_row_weights(w)
    f = o.forward(spec, theta, X, np.float64)
    y = np.asarray(Y, np.float64).reshape(f.shape[1], -1).T
    S, W_, d = float(np.sum(w * (y - f) ** 2)), float(np.sum(w, dtype=np.float64)), f.shape[0]
    eta = eta.copy()
    eta[-1] = np.float32((S / (W_ * d)) ** 0.25)          # sd near its weighted optimum: a gentle trajectory fp32 and fp64 agree on
    ch.set_state(theta); ch.set_hypers(eta)
    ph = np.random.default_rng(8).standard_normal(len(eta)).astype(np.float32)
    for log_u in (-1e30, 1e30):
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hyper_step(1e-5, 4, p0=ph, log_u=log_u)
        ref = o.hyper_step(spec, eta, theta, X, Y, 1e-5, 4, ph, log_u, np.float64, S=S, w=w)
        assert bool(out["accepted"]) == ref.accepted == (log_u < 0)
        assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= 1e-2 + 1e-4 * abs(ref.log_accept_ratio)
        assert np.abs(ch.get_hypers() - ref.theta).max() <= 1e-5 * max(1.0, np.abs(ref.theta).max())
    ch.close()


def test_refusals_and_clearing(native, monkeypatch):
    from tensorbnn_amd._native import TbnnError
    name = "mid_gauss"
    spec, X, Y, theta, eta = problem(name, 500)
    ch = make_chain(native, monkeypatch, name, True)
    with pytest.raises(TbnnError, match="set_data"):
        ch.set_row_weights(np.ones(len(X), np.float32))                  # no rows staged yet
    ch.set_data(X, Y)
    base = ch.kernel_name
    for bad, what in ((-np.ones(len(X), np.float32), "negative"), (np.full(len(X), np.nan, np.float32), "finite"),
                      (np.zeros(len(X), np.float32), "zero"), (np.ones(len(X) - 1, np.float32), "does not match")):
        with pytest.raises(TbnnError, match=what):
            ch.set_row_weights(bad)
        assert ch.kernel_name == base
    lu = ch.logp_grad(theta, eta)[0]
    w = real_weights(len(X))
    ch.set_row_weights(w)
    assert ch.kernel_name == base.replace(";", ",weighted;", 1)
    lw = ch.logp_grad(theta, eta)[0]
    assert lw != lu
    ch.set_row_weights(None)                                            # cleared: the unweighted table again
    assert ch.kernel_name == base and ch.logp_grad(theta, eta)[0] == lu
    ch.set_row_weights(w)
    ch.set_data(X, Y)                                                   # new rows drop the weights
    assert ch.kernel_name == base and not ch.row_weighted and ch.logp_grad(theta, eta)[0] == lu
    ch.close()


SHARD_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = sys.argv[1:4]
import tbnn_oracle as o
from tensorbnn_amd import _native as nat, parallel
from tensorbnn_amd._native import TbnnError
from test_gpu_row_weights import problem, spec_of, real_weights
from tensor_checks import layers_of
from test_gpu_freerun import SEED


def refused(fn, what):
    try:
        fn()
    except TbnnError as e:
        assert what in str(e), str(e)
        return
    raise AssertionError("not refused: " + what)


spec, X, Y, theta, eta = problem("fast3_configs1", 2000)
ch = nat.Chain(layers_of(spec), likelihood=o.LIK_GAUSSIAN, jit=True, seed=SEED, chain_id=1)
ch.set_data(X, Y)
lp0 = ch.logp_grad(theta, eta)[0]
comm = parallel.make_comm(ch)
w = real_weights(len(X))
ch.set_row_weights(w)
refused(lambda: ch.set_row_shard(comm, len(X)), "row weights")
refused(lambda: parallel.shard_rows(ch, X, Y, comm), "row weights")
assert ch.row_weighted and "weighted" in ch.kernel_name
ch.set_row_weights(None)
assert parallel.shard_rows(ch, X, Y, comm) == (0, len(X))
refused(lambda: ch.set_row_weights(w), "row-sharded")
lp1 = ch.logp_grad(theta, eta)[0]                 # the sharded pass and its all-reduce
assert abs(lp1 - lp0) <= 1e-9 * abs(lp0), (lp1, lp0)
ch.set_row_shard(None)
assert ch.logp_grad(theta, eta)[0] == lp0
comm.close()
ch.close()
print("row-shard refusals ok")
"""


def test_row_shard_refused_in_either_order(tmp_path):
    """tbnn_set_row_shard refuses a weighted handle, parallel.shard_rows a weighted chain, tbnn_set_row_weights a sharded handle; cleared,
    the chain shards with the unsharded value.  A communicator of one rank over the stand-in collective library (tests/stubccl, as the
    world-2 tests use it), in a child process of its own: libtbnn binds its collective library once per process"""
    import os
    import subprocess
    import sys
    from test_gpu_multirank import build_stub
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    script = tmp_path / "shard_child.py"
    script.write_text(SHARD_CHILD)
    env = dict(os.environ, TBNN_RCCL_LIB=build_stub(), TBNN_JIT_SKIP=NARROW3)
    p = subprocess.run([sys.executable, str(script), root, os.path.join(root, "oracle"), here], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "row-shard refusals ok" in p.stdout, (p.returncode, (p.stdout + p.stderr)[-3000:])


def test_chain_group_equals_solo_chains(native, monkeypatch):
    name = "fast3_bern"
    spec, X, Y, theta, eta = problem(name)
    w = real_weights(len(X), 4)
    C, cid = 3, 5
    monkeypatch.setenv("TBNN_JIT_SKIP", NARROW3)
    grp = native.ChainGroup(layers_of(spec), C, likelihood=o.LIK_BERNOULLI, seed=SEED, chain_id=cid, jit=True)
    _OPEN.append(grp)
    grp.set_data(X, Y)
    grp.set_row_weights(w)
    assert ",weighted;" in grp.kernel_name
    grp.set_state(theta); grp.set_hypers(eta)
    for _ in range(2):
        grp.hmc_step(1e-3, 5)
    gh = grp.hyper_step(1e-3, 3)
    states = grp.get_state().reshape(C, -1)
    for c in range(C):
        ch = native.Chain(layers_of(spec), likelihood=o.LIK_BERNOULLI, seed=SEED, chain_id=cid + c, jit=True)
        _OPEN.append(ch)
        ch.set_data(X, Y)
        ch.set_row_weights(w)
        ch.set_state(theta); ch.set_hypers(eta)
        for _ in range(2):
            ch.hmc_step(1e-3, 5)
        h = ch.hyper_step(1e-3, 3)
        assert np.array_equal(ch.get_state(), states[c]) and h["log_accept_ratio"] == gh[c]["log_accept_ratio"], c


def test_train_chains_weighted_equal_solo_runs(tmp_path, monkeypatch, native):
    from test_gpu_categorical import blobs, make_net
    from tensorbnn_amd.likelihood import CategoricalLikelihood
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, Y = blobs(600, 1)
    Xv, Yv = blobs(200, 2)
    w = real_weights(len(X), 12)

    def net_of(chain_id=0):
        net = make_net(X, Y, Xv, Yv, chain_id)
        net.trainWeights = w               # (as network(..., trainWeights=w) stages them; make_net builds the layers)
        return net
    C, EPOCHS = 2, 8
    rec = net_of().trainChains(C, EPOCHS, 4, CategoricalLikelihood(), adjustHypers=True, folderName="multi", networksPerFile=2)
    for c in range(C):
        net = net_of(c)
        solo = net.train(EPOCHS, 4, CategoricalLikelihood(), adjustHypers=True, folderName="solo%d" % c, networksPerFile=2, verbose=False)
        assert net._chain.kernel_name.startswith("jit-mid<") and ",categorical,weighted;" in net._chain.kernel_name
        for rg, rs in zip(rec, solo):
            assert rg["eps"][c] == rs["eps"] and rg["L"][c] == rs["L"]
            for k in ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new", "sjd"):
                assert rg["main"][c][k] == rs["main"][k], (c, rg["iter"], k)
            assert rg["hyper"][c]["log_accept_ratio"] == rs["hyper"]["log_accept_ratio"]


def test_imbalanced_bernoulli_train(tmp_path, monkeypatch, native):
    from tensorbnn_amd.activationFunctions import Relu, Sigmoid
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.likelihood import BernoulliLikelihood
    from tensorbnn_amd.network import network
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    rng = np.random.default_rng(21)
    n = 800
    Y = (rng.random(n) < 0.1).astype(np.float32)                      # 10 % positives
    X = (rng.standard_normal((n, 2)) + 1.5 * Y[:, None]).astype(np.float32)
    w = np.where(Y == 1, 9.0, 1.0).astype(np.float32)                   # class weights
    net = network(np.float32, 2, X, Y, X[:100], Y[:100], trainWeights=w)
    net.add(DenseLayer(2, 16, seed=1000)); net.add(Relu())
    net.add(DenseLayer(16, 16, seed=2000)); net.add(Relu())
    net.add(DenseLayer(16, 1, seed=3000)); net.add(Sigmoid())
    net.setupMCMC(stepSizeStart=2e-3, stepSizeMin=5e-4, stepSizeMax=1e-2, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=5, averagingSteps=2, randomSteps=2)
    rec = net.train(12, 4, BernoulliLikelihood(), folderName="imb", networksPerFile=2, verbose=False)
    assert len(rec) == 12 and net._chain.row_weighted
    assert net._chain.kernel_name.startswith("jit-fast3<") and ",bernoulli,weighted;" in net._chain.kernel_name
    assert all(np.isfinite(r["main"]["logp_new"]) for r in rec)
    p = net.predict(True).reshape(-1)
    assert np.all(np.isfinite(p)) and p[Y == 1].mean() > p[Y == 0].mean()
