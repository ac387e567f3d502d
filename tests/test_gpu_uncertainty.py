"""GPU: classification uncertainty over an ensemble's network axis (tbnn_ensemble_uncertainty, Chain.ensemble_uncertainty,
predictor.predictUncertainty / calibration) against tests/uncertainty_ref.py applied to the fp32 predictions Chain.forward_many returns for
the same handle, thetas and rows: both paths see the same f_i bit for bit, so the test isolates the reduction.  Every test here fails
without the entry point (missing symbol / attribute).

Bounds (U = 2^-53, u = 2^-24, m networks; the sums after the per-network fp32 values are fp64 in a fixed order, the reference's are
np.longdouble):

  probs, votes.  Sums of m terms in [0, 1] divided by W: 4 m U absolute, the derivation of tests/test_gpu_ensemble.py's docstring (the
  sequential-summation bound, the products, the division).  Bernoulli: the fp32 p is the input itself.  Categorical: the fp32 softmax
  enters each p_ik with XFORM_ULP["softmax"] ulp32 (the bound tests/test_gpu_ensemble.py holds the same expressions to) and 2^-126 where
  it may be flushed; the mean takes the weighted mean of those.  A vote is compared on every row but those where, under some network,
  the two largest fp64 probabilities lie closer than that softmax bound (the arg-max of the fp32 values may then differ): fewer than 2 %
  of the rows may be left out (a cap; none are on these generators), and with equal weights the kept rows' counts are exact integers.

  Bernoulli entropies.  16 U (1 + |H|) per network term (two logs, two products, a sum), (m + 16) U on the averages; epistemic the sum
  of the two.

  Categorical entropies.  The fp32 softmax enters -p log p with the first-order sensitivity |1 + log p|: the error is measured in units
  of u sum_k p_k (1 + |log p_k|) per row (aleatoric: the weighted mean over the networks of their units; total: the unit at pbar, whose
  relative error is at most the networks').  No ULP statement for the device's expf is installed with the toolkit, so the bound is
  ENTROPY_ULP below, 4 x the largest figure observed against the fp64 reference on the first green MI355X run (DESIGN.md section 4.6,
  "Classification uncertainty"); 2^-126 x 128 of absolute slack per class below the fp32 normal range, (m + 16) U for the fp64 sums.
  Epistemic: the sum of the two.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import test_gpu_ensemble as ge
import uncertainty_ref as ur

pytestmark = pytest.mark.gpu

U, u = ge.U, ge.u
SOFTMAX_ULP = ge.XFORM_ULP["softmax"]
# 4 x the largest error of a categorical entropy observed against tests/uncertainty_ref.py on the first green MI355X run, 2026-10-20,
# library build 9b5ddac6bc71484e, in the units of the module docstring: 4.256 (30-80-80-10, one network alone; every other case of this
# module stayed below 3.2).  Below the softmax's own 18.4 ulp32: the entropy loses no more than the probabilities it is made of.
ENTROPY_MEASURED = 4.256
ENTROPY_ULP = 4 * ENTROPY_MEASURED
assert ENTROPY_MEASURED <= SOFTMAX_ULP

NONE, RELU, TANH, SIGMOID = 0, 1, 2, 3
LIK_GAUSSIAN, LIK_FIXED_GAUSSIAN, LIK_BERNOULLI, LIK_CATEGORICAL = 0, 1, 2, 3
FUSED = {"fast3": "mid,tall,wide", "mid": "fast3,fast,tall,wide", "tall": "fast3,fast,mid,wide", "wide": "fast3,fast,mid,tall"}

# dims, hidden activation, last activation, the reading, rows, how the handle is made, kernel-name prefix.  "aot": an ahead-of-time
# shape; "jit:<family>": a run-time shape other modules of the suite build too (tests/jit_shapes.json, tests/test_gpu_categorical.py);
# "layered" / "generic": those families.  The narrow family has no sigmoid output among its ahead-of-time shapes, so it runs the
# run-time Bernoulli shape the suite already builds (5-20-24-1), and the 5-50-50-50-1 sigmoid network runs where a handle without a
# run-time library puts it, on the layered family.
CASES = {
    "narrow": ([5, 20, 24, 1], TANH, SIGMOID, "bernoulli", 301, "jit:fast3", "jit-fast3"),
    "narrow_dims": ([5, 50, 50, 50, 1], RELU, SIGMOID, "bernoulli", 301, "layered", "layered<"),
    "tall": ([784, 20, 20, 1], RELU, SIGMOID, "bernoulli", 301, "aot", "tall<"),
    "mid": ([20, 100, 100, 2], RELU, SIGMOID, "bernoulli", 301, "aot", "mid<"),
    "mid10": ([30, 80, 80, 10], RELU, NONE, "categorical", 301, "jit:mid", "jit-mid"),
    "tall10": ([784, 20, 20, 10], RELU, NONE, "categorical", 301, "jit:tall", "jit-tall"),
    "wide10": ([10, 200, 200, 10], RELU, NONE, "categorical", 301, "jit:wide", "jit-wide"),
    "lay20": ([20, 64, 64, 20], TANH, NONE, "categorical", 301, "layered", "layered<"),
    "lay2": ([20, 64, 64, 2], RELU, NONE, "categorical", 301, "layered", "layered<"),
    "generic4": ([5, 16, 16, 4], TANH, NONE, "categorical", 517, "generic", "generic"),
}
KIND_LIK = {"bernoulli": LIK_BERNOULLI, "categorical": LIK_CATEGORICAL}
M = 8


def layers_for(name):
    dims, act, last = CASES[name][:3]
    return [(dims[i], dims[i + 1], act if i < len(dims) - 2 else last, 0) for i in range(len(dims) - 1)]


def jit_jobs():
    return [{"layers": [list(l) for l in layers_for(name)], "likelihood": KIND_LIK[c[3]], "skip": FUSED[c[5][4:]], "flags": ""}
            for name, c in CASES.items() if c[5].startswith("jit:")]


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """this module's run-time shapes, the jobs of tests/jit_shapes.json and tests/test_gpu_categorical.py: cache hits after those"""
    from tensorbnn_amd import jit
    jobs = jit_jobs()
    assert jit.prebuild(jobs) == len(jobs)


def make_chain(native, monkeypatch, name):
    how, prefix = CASES[name][5:7]
    lik = KIND_LIK[CASES[name][3]]
    if how.startswith("jit:"):
        monkeypatch.setenv("TBNN_JIT_SKIP", FUSED[how[4:]])
        ch = native.Chain(layers_for(name), likelihood=lik, jit=True)
    elif how == "layered":
        for k in ("TBNN_TALL", "TBNN_MID", "TBNN_REGISTERED"):
            monkeypatch.setenv(k, "0")
        monkeypatch.setenv("TBNN_JIT_SKIP", "fast3,fast,mid,tall,wide")
        ch = native.Chain(layers_for(name), likelihood=lik, jit=False)
    elif how == "generic":
        ch = native.Chain(layers_for(name), likelihood=lik, kernel=native.KERNEL_GENERIC)
    else:
        ch = native.Chain(layers_for(name), likelihood=lik)
    assert ch.kernel_name.startswith(prefix), (name, ch.kernel_name)
    return ch


def problem(name, m=M, seed=0, n=None):
    """the generator of tests/test_gpu_ensemble.problem: rows N(0, 1) scaled down for a long fan-in, thetas 0.35 N(0, 1)"""
    dims, rows = CASES[name][0], CASES[name][4]
    n = rows if n is None else n
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, dims[0])) / math.sqrt(max(dims[0] / 16.0, 1.0))).astype(np.float32)
    P = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
    thetas = (rng.standard_normal((m, P)) * 0.35).astype(np.float32)
    return X, thetas


KEYS = ("probs", "votes", "total", "aleatoric", "epistemic")
FIGURES = []                                        # the categorical entropies' errors in their units, as they are measured


def entropy_unit(p):
    """sum over axis -2 (the classes) of p (1 + |log p|), 0 at p = 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p == 0, 0.0, p * (1.0 + np.abs(np.log(np.where(p == 0, 1.0, p))))).sum(axis=-2)


def check(tag, got, f, w, kind, vacuity=False):
    """got: Chain.ensemble_uncertainty's dict; f: forward_many's fp32 [m, d_out, n].  Prints each figure, then asserts the bounds of the
    module docstring.  Returns the reference."""
    m, K, n = f.shape
    ref = ur.uncertainty(f, w, kind)
    wn = np.ones(m) / m if w is None else np.asarray(w, dtype=np.float64) / np.asarray(w, dtype=np.float64).sum()
    p = ref["p"]
    shape = (n,) if kind == "categorical" else (K, n)
    for k in KEYS:
        assert got[k].dtype == np.float64 and got[k].shape == ((K, n) if k in ("probs", "votes") else shape), (tag, k, got[k].shape)
        assert np.all(np.isfinite(got[k])), (tag, k)
    if vacuity:
        print(f"[uncertainty] {tag}: reference epistemic min {ref['epistemic'].min():.4f} max {ref['epistemic'].max():.4f}")
        assert ref["epistemic"].min() > 1e-3, (tag, float(ref["epistemic"].min()))
    keep = np.ones(n, dtype=bool)
    if kind == "categorical":
        dp = SOFTMAX_ULP * ge.ulp32(p) + 2.0 ** -126
        tol_p = 4 * m * U + np.tensordot(wn, dp, axes=(0, 0))
        top = np.sort(p, axis=1)[:, -2:, :]
        keep = ~((top[:, 1] - top[:, 0]) < SOFTMAX_ULP * ge.ulp32(top[:, 1])).any(axis=0)
        assert (~keep).mean() < 0.02, (tag, float((~keep).mean()))
        unit_al = u * np.tensordot(wn, entropy_unit(p), axes=(0, 0))
        unit_tot = u * entropy_unit(ref["probs"])
        slack = K * 2.0 ** -126 * 128 + (m + 16) * U
        tol_al, tol_tot = ENTROPY_ULP * unit_al + slack, ENTROPY_ULP * unit_tot + slack
    else:
        tol_p = np.full((K, n), 4 * m * U)
        tol_al = tol_tot = np.full((K, n), (m + 16) * U)
        assert np.all(got["total"] <= math.log(2) * (1 + 4 * U)), tag
    err = {k: np.abs(got[k] - ref[k]) for k in KEYS}
    tol = {"probs": tol_p, "votes": 4 * m * U, "total": tol_tot, "aleatoric": tol_al, "epistemic": tol_al + tol_tot}
    line = ", ".join(f"{k} {np.max(err[k][..., keep]):.2e} ({np.max((err[k] / tol[k])[..., keep]):.3f} of tol)" for k in KEYS)
    print(f"[uncertainty] {tag}: m={m} rows left out of the votes {int((~keep).sum())}; {line}")
    if kind == "categorical":
        fig = max(float(np.max(err["aleatoric"] / unit_al)), float(np.max(err["total"] / unit_tot)))
        FIGURES.append(fig)
        print(f"[uncertainty] {tag}: categorical entropy error {fig:.3f} units (largest so far {max(FIGURES):.3f}, bound {ENTROPY_ULP:.3f})")
    for k in KEYS:
        sel = keep if k == "votes" else slice(None)
        assert np.all(err[k][..., sel] <= (tol[k][..., sel] if np.ndim(tol[k]) else tol[k])), (tag, k, float(np.max((err[k] / tol[k])[..., sel])))
    assert np.all(got["epistemic"] >= 0) and np.all(got["probs"] >= 0) and np.all(got["votes"] >= 0) and np.all(got["votes"] <= 1)
    if w is None:
        counts = got["votes"][:, keep] * m
        if kind == "categorical":
            want = (ref["arg"][:, None, :] == np.arange(K)[None, :, None]).sum(axis=0)[:, keep]
        else:
            want = (p >= 0.5).sum(axis=0)
        assert np.array_equal(np.rint(counts), want) and np.all(np.abs(counts - want) <= 4 * m * m * U), tag
    return ref


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


# --------------------------------------------------------------------------------------------------------------------- every family
@pytest.mark.parametrize("name", list(CASES))
def test_every_family(native, monkeypatch, name):
    """equal weights and the gamma weights with one 0; explicit rows and staged validation rows; three calls, the same bits; the
    networks disagree on every row (the reference's epistemic term exceeds 1e-3), so a kernel that ignores the network axis fails"""
    kind = CASES[name][3]
    X, thetas = problem(name)
    ch = make_chain(native, monkeypatch, name)
    f = ch.forward_many(thetas, X=X)
    assert f.shape == (M, CASES[name][0][-1], X.shape[0]) and X.shape[0] % 64
    lik = KIND_LIK[kind]
    for tag, w in (("equal", None), ("weighted", ge.net_weights(M))):
        got = ch.ensemble_uncertainty(thetas, X=X, weights=w, likelihood=lik)
        ref = check(f"{name} [{ch.kernel_name}] {tag}", got, f, w, kind, vacuity=w is None)
        for _ in range(2):
            assert same_bits(got, ch.ensemble_uncertainty(thetas, X=X, weights=w, likelihood=lik)), (name, tag)
        if w is None and kind == "categorical":
            assert (ref["arg"] != np.argmax(ref["probs"], axis=0)[None]).any(axis=0).mean() >= 0.5      # (most rows: a network dissents)
    # likelihood None: the handle's own; staged validation rows
    nv = 77
    ch.set_validation(X[:nv], np.zeros((nv, f.shape[1]), dtype=np.float32))
    staged, explicit = ch.ensemble_uncertainty(thetas, which=1), ch.ensemble_uncertainty(thetas, X=X[:nv], likelihood=lik)
    for k in KEYS:
        assert np.array_equal(staged[k], explicit[k]), (name, k)
    assert np.array_equal(ch.forward_many(thetas, X=X), f)
    ch.close()


# ----------------------------------------------------------------------------------------------------------------- chunk carry-over
@pytest.mark.parametrize("name", ["mid", "lay20"])
def test_chunk_override_carries_over(native, monkeypatch, name):
    """TBNN_ENS_CHUNK_FLOATS cuts 8 networks into chunks of 3, 3 and 2: S, V and A are read back and continued in the same order, so
    every output equals the one-chunk call bit for bit"""
    kind = CASES[name][3]
    X, thetas = problem(name, seed=2)
    ch = make_chain(native, monkeypatch, name)
    w = ge.net_weights(M)
    d_out = CASES[name][0][-1]
    one = [ch.ensemble_uncertainty(thetas, X=X, weights=wt, likelihood=KIND_LIK[kind]) for wt in (None, w)]
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(3 * d_out * X.shape[0] + 5))
    cut = [ch.ensemble_uncertainty(thetas, X=X, weights=wt, likelihood=KIND_LIK[kind]) for wt in (None, w)]
    monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
    for a, b in zip(one, cut):
        assert same_bits(a, b)
    check(f"{name} chunks of 3", cut[1], ch.forward_many(thetas, X=X), w, kind)
    ch.close()


# ----------------------------------------------------------------------------------------------------------------------- one network
@pytest.mark.parametrize("name", ["tall", "mid", "mid10", "lay20", "generic4"])
def test_one_network(native, monkeypatch, name):
    """m = 1: nothing to disagree about -- epistemic <= 8 U, votes exactly 0 or 1, total = aleatoric"""
    kind = CASES[name][3]
    X, thetas = problem(name, m=3, seed=3)
    ch = make_chain(native, monkeypatch, name)
    for i in range(3):
        f = ch.forward_many(thetas[i:i + 1], X=X)
        for w in (None, np.array([0.37], dtype=np.float32)):
            got = ch.ensemble_uncertainty(thetas[i:i + 1], X=X, weights=w, likelihood=KIND_LIK[kind])
            check(f"{name} network {i} alone", got, f, w, kind)
            assert np.all((got["votes"] == 0) | (got["votes"] == 1))
            if w is not None:                      # (w p / w is p only up to a rounding)
                continue
            assert np.all(got["epistemic"] <= 8 * U), float(got["epistemic"].max())
            assert np.all(np.abs(got["total"] - got["aleatoric"]) <= 8 * U * (1 + got["total"]))
            if kind == "categorical":
                assert np.array_equal(got["votes"].sum(axis=0), np.ones(X.shape[0]))
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------ saturation
def scaled(thetas, s):
    return (thetas.astype(np.float64) * s).astype(np.float32)


@pytest.mark.parametrize("name,scale", [("lay20", 20.0), ("mid10", 6.0), ("mid", 8.0)])
def test_saturated(native, monkeypatch, name, scale):
    """thetas scaled up until fp32 probabilities come out exactly 0 and 1: every output finite (0 log 0 = 0), the comparison holds"""
    kind = CASES[name][3]
    X, thetas = problem(name, seed=4)
    th = scaled(thetas, scale)
    ch = make_chain(native, monkeypatch, name)
    f = ch.forward_many(th, X=X)
    assert np.all(np.isfinite(f))
    p32 = ur.softmax64(f).astype(np.float32) if kind == "categorical" else f
    print(f"[uncertainty] {name} x{scale}: {np.mean(p32 == 0):.3f} of the fp32 probabilities are 0, {np.mean(p32 == 1):.3f} are 1")
    assert np.mean(p32 == 0) > 0.05 and np.mean(p32 == 1) > 0.005
    for w in (None, ge.net_weights(M)):
        got = ch.ensemble_uncertainty(th, X=X, weights=w, likelihood=KIND_LIK[kind])
        check(f"{name} saturated x{scale} {'equal' if w is None else 'weighted'}", got, f, w, kind)
        assert np.all(got["total"] <= math.log(f.shape[1] if kind == "categorical" else 2) * (1 + 4 * U)), float(got["total"].max())
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------------- NaN
@pytest.mark.parametrize("name", ["tall", "generic4", "mid10"])
def test_nan_rule(native, monkeypatch, name):
    """one NaN in one theta (the last bias of network 3): every output of every row is NaN, whatever that network's weight, the call
    returns 0, and a clean call on the same handle afterwards gives the clean result bit for bit"""
    kind = CASES[name][3]
    X, thetas = problem(name, seed=5)
    ch = make_chain(native, monkeypatch, name)
    clean = ch.ensemble_uncertainty(thetas, X=X, likelihood=KIND_LIK[kind])
    bad = thetas.copy()
    bad[3, -1] = np.nan
    w0 = np.ones(M, dtype=np.float32)
    w0[3] = 0.0
    for w in (None, w0):
        got = ch.ensemble_uncertainty(bad, X=X, weights=w, likelihood=KIND_LIK[kind])
        for k in KEYS:
            assert np.all(np.isnan(got[k])), (name, k, int(np.isfinite(got[k]).sum()))
        assert same_bits(got, {k: v for k, v in ur.uncertainty(ch.forward_many(bad, X=X), w, kind).items() if k in KEYS})
    assert same_bits(clean, ch.ensemble_uncertainty(thetas, X=X, likelihood=KIND_LIK[kind]))
    ch.close()


# -------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(native, monkeypatch):
    dp = C.POINTER(C.c_double)
    lib, p = native.lib, native._p
    name = "generic4"
    X, thetas = problem(name, m=4)
    n, P, K = X.shape[0], thetas.shape[1], 4
    ch = make_chain(native, monkeypatch, name)
    one = make_chain(native, monkeypatch, "tall")                    # one output: no categorical reading
    outs = [np.full((K, n), -7.0) for _ in range(2)] + [np.full(n, -7.0) for _ in range(3)]
    ptrs = [a.ctypes.data_as(dp) for a in outs]

    def call(h=None, m=4, stride=P, lik=LIK_CATEGORICAL, w=None, which=1, X_=X, n_=n, o=ptrs):
        return lib.tbnn_ensemble_uncertainty(ch._h if h is None else h, p(thetas), m, stride, lik, p(w), which, p(X_), n_, *o)

    def refused(msg, **kw):
        assert call(**kw) < 0, msg
        assert msg in lib.tbnn_last_error().decode(), (msg, lib.tbnn_last_error())
        assert all(np.all(a == -7.0) for a in outs), msg

    f32 = lambda *v: np.array(v, dtype=np.float32)
    assert lib.tbnn_ensemble_uncertainty(None, p(thetas), 4, P, LIK_CATEGORICAL, None, 1, p(X), n, *ptrs) < 0
    assert "null handle" in lib.tbnn_last_error().decode() and all(np.all(a == -7.0) for a in outs)
    refused("every output is null", o=[None] * 5)
    for lik in (LIK_GAUSSIAN, LIK_FIXED_GAUSSIAN, 5, 8, 10, 12, 7):
        refused("tbnn_ensemble_predictive and tbnn_ensemble_moments", lik=lik)
    th1 = np.zeros((4, one.P), dtype=np.float32)
    X1 = np.zeros((n, 784), dtype=np.float32)
    assert lib.tbnn_ensemble_uncertainty(one._h, p(th1), 4, one.P, LIK_CATEGORICAL, None, 1, p(X1), n, *ptrs) < 0
    assert "at least 2 outputs" in lib.tbnn_last_error().decode() and all(np.all(a == -7.0) for a in outs)
    for w, msg in ((f32(1, -1, 1, 1), "negative"), (f32(1, np.nan, 1, 1), "not finite"), (f32(1, np.inf, 1, 1), "not finite"),
                   (f32(0, 0, 0, 0), "all weights are zero")):
        refused(msg, w=w)
    refused("m < 1", m=0)
    refused("theta_stride < P", stride=P - 1)
    refused("n < 1", n_=0)
    refused("which must be", X_=None, n_=0, which=2)
    refused("tbnn_set_validation has not been called", X_=None, n_=0, which=1)
    refused("tbnn_set_data has not been called", X_=None, n_=0, which=0)
    with pytest.raises(native.TbnnError, match="negative"):
        ch.ensemble_uncertainty(thetas, X=X, weights=[1, -1, 1, 1])
    with pytest.raises(ValueError, match="one per network"):
        ch.ensemble_uncertainty(thetas, X=X, weights=[1, 1])
    # some outputs NULL: the others are written, and equal the full call's
    full = ch.ensemble_uncertainty(thetas, X=X)
    assert call(o=[None, ptrs[1], None, None, ptrs[4]]) == 0
    assert np.array_equal(outs[1], full["votes"]) and np.array_equal(outs[4], full["epistemic"])
    assert np.all(outs[0] == -7.0) and np.all(outs[2] == -7.0) and np.all(outs[3] == -7.0)
    ch.close(); one.close()


def test_multi_chain_handle(native, monkeypatch):
    """a tbnn_create_multi handle takes explicit thetas like a one-chain handle"""
    name = "mid"
    X, thetas = problem(name, m=5)
    ch = make_chain(native, monkeypatch, name)
    grp = native.ChainGroup(layers_for(name), 3, likelihood=LIK_BERNOULLI)
    want = ch.ensemble_uncertainty(thetas, X=X, weights=ge.net_weights(5))
    w = ge.net_weights(5)
    n = X.shape[0]
    outs = [np.empty((2, n)) for _ in range(5)]
    dp = C.POINTER(C.c_double)
    rc = native.lib.tbnn_ensemble_uncertainty(grp._h, native._p(thetas), 5, thetas.shape[1], LIK_BERNOULLI, native._p(w), 1, native._p(X), n,
                                              *[a.ctypes.data_as(dp) for a in outs])
    assert rc == 0, native.lib.tbnn_last_error()
    for a, k in zip(outs, KEYS):
        assert np.array_equal(a, want[k]), k
    ch.close(); grp.close()


# ---------------------------------------------------------------------------------------------------------------- predictor, end to end
def write_networks(folder, dims, arch, thetas):
    """`folder` in the saved-sample format the predictor reads (summary.txt, <matrix>.0.txt, architecture.txt; no hypers): network i is
    thetas[i], per layer W[out, in] then b[out]"""
    os.makedirs(folder)
    S = thetas.shape[0]
    shapes = []
    for i in range(len(dims) - 1):
        shapes += [(dims[i + 1], dims[i]), (dims[i + 1],)]
    with open(os.path.join(folder, "summary.txt"), "w") as fh:
        for sh in shapes:
            fh.write(" ".join(str(v) for v in sh) + "\n")
        fh.write(f"{S} 1 {len(shapes)}\n0\n")
    off = 0
    for i, sh in enumerate(shapes):
        size = int(np.prod(sh))
        block = thetas[:, off:off + size].reshape(S * sh[0], sh[1] if len(sh) == 2 else 1)
        np.savetxt(os.path.join(folder, f"{i}.0.txt"), block, fmt="%.9e")
        off += size
    with open(os.path.join(folder, "architecture.txt"), "w") as fh:
        fh.write("\n".join(arch) + "\n")


def check_predictor(tag, p, X, Y, kind, weights, m):
    from tensorbnn_amd.predictor import predictor
    lik = KIND_LIK[kind]
    ch = p._ensure_chain()
    picked = np.stack(p.vectors)
    for n_, w in ((1, None), (1, weights), (2, None)):
        out = p.predictUncertainty(X, n=n_, weights=w)
        direct = ch.ensemble_uncertainty(picked[::n_], X=X, weights=w, likelihood=lik)
        assert same_bits(out, direct), (tag, n_)
        assert np.array_equal(out["variation_ratio"], ur.variation_ratio(out["votes"], kind))
        assert out["variation_ratio"].shape == out["total"].shape and np.all(out["variation_ratio"] >= 0)
        mk = len(range(0, m, n_))
        check(f"{tag} n={n_} {'weighted' if w is not None else 'equal'}", direct, np.array(p.predict(X, n_)), w, kind)
        cal = p.calibration(X, Y, bins=7, n=n_, weights=w)
        want = ur.calibration(out["probs"], Y, 7, kind)
        for k in ("accuracy", "nll", "brier", "ece", "mce"):
            assert cal[k] == pytest.approx(want[k], rel=1e-12, abs=1e-15), (tag, k)
        for k in ("count", "confidence", "accuracy", "edges"):
            assert np.allclose(cal["bins"][k], want["bins"][k], rtol=1e-12, atol=0, equal_nan=True), (tag, k)
        for k in ("predicted", "confidence", "correct"):
            assert np.array_equal(cal[k], want[k]), (tag, k)
        # ... and the helper applied to predictMoments' mean: the moments kernel shifts its sums, so within 4 m U, not bit for bit
        mean = p.predictMoments(X, n=n_, weights=w)[0]
        assert np.all(np.abs(mean - out["probs"]) <= 4 * mk * U + np.spacing(mean)), (tag, float(np.abs(mean - out["probs"]).max()))
        via = predictor._calibration_table(mean, Y, 7, kind)
        # where no arg-max and no bin edge lies within 1e-9 of a tie, the two tables differ by the 4 m U of their probabilities alone:
        # -log p moves by 4 m U / p, a square or a gap by a few times 4 m U
        sure = np.abs(np.sort(mean, axis=0)[-1] - np.sort(mean, axis=0)[-2]) > 1e-9 if kind == "categorical" else np.abs(mean - 0.5) > 1e-9
        near_edge = np.abs(cal["confidence"][..., None] - cal["bins"]["edges"][1:-1]).min() <= 1e-9      # (nothing lies beyond 0 and 1)
        assert np.all(sure) and not near_edge, tag
        label = ur.labels_of(Y, mean.shape[0], X.shape[0], kind)
        p_label = mean[label, np.arange(X.shape[0])] if kind == "categorical" else np.where(label, mean, 1.0 - mean)
        tol = {"nll": 2 * np.mean(4 * mk * U / p_label), "brier": 64 * mk * U, "ece": 64 * mk * U, "mce": 64 * mk * U}
        for k in tol:
            assert abs(via[k] - cal[k]) <= tol[k] + 4 * U * abs(cal[k]), (tag, k, via[k], cal[k])
        assert via["accuracy"] == cal["accuracy"] and np.array_equal(via["predicted"], cal["predicted"])
    return out


def test_predictor_categorical(tmp_path, monkeypatch, native):
    """a three-class network trained for a few epochs, the set-up of tests/test_gpu_ensemble.py's predictor test: predictUncertainty is the
    Chain call, variation_ratio follows from the votes, calibration is the helper on probs (integer labels = one-hot), reweight's
    weights pass through, a regression likelihood is refused"""
    from test_gpu_categorical import blobs, make_net
    from tensorbnn_amd.likelihood import CategoricalLikelihood, GaussianLikelihood
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    X, Y = blobs(600, 1)
    Xv, Yv = blobs(301, 2)
    net = make_net(X, Y, Xv, Yv)
    net.train(30, 2, CategoricalLikelihood(), folderName="blobs", networksPerFile=1, verbose=False)
    p = predictor(str(tmp_path / "blobs") + "/", likelihood=CategoricalLikelihood())
    assert p.numNetworks >= 4
    weights = np.asarray(p.reweight(str(tmp_path / "blobs" / "architecture.txt")), dtype=np.float32)
    out = check_predictor("predictor categorical", p, Xv, Yv, "categorical", weights, p.numNetworks)
    assert np.all(np.abs(out["probs"].sum(axis=0) - 1.0) <= 3 * 2.0 ** -23)
    a, b = p.calibration(Xv, Yv, bins=5), p.calibration(Xv, np.argmax(Yv, axis=1), bins=5)
    assert a["ece"] == b["ece"] and a["nll"] == b["nll"] and np.array_equal(a["bins"]["count"], b["bins"]["count"])
    assert a["accuracy"] > 0.8                                                   # (the blobs are separable: the fit is a classifier)
    with pytest.raises(ValueError, match="predictMoments"):
        p.predictUncertainty(Xv, likelihood=GaussianLikelihood(sd=0.1))
    with pytest.raises(ValueError, match="bins"):
        p.calibration(Xv, Yv, bins=0)


def test_predictor_bernoulli_and_from_chains(tmp_path, native):
    """saved networks written in the sample format: a two-output sigmoid network read under a BernoulliLikelihood, as one directory and
    as two chains through fromChains"""
    from tensorbnn_amd.likelihood import BernoulliLikelihood
    from tensorbnn_amd.predictor import predictor
    dims, arch = [4, 17, 9, 2], ["dense", "tanh", "dense", "tanh", "dense", "sigmoid"]
    rng = np.random.default_rng(21)
    P = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
    thetas = (rng.standard_normal((6, P)) * 0.8).astype(np.float32)
    X = rng.standard_normal((301, 4)).astype(np.float32)
    Y = (rng.random((301, 2)) < 0.5).astype(np.float32)
    write_networks(str(tmp_path / "solo"), dims, arch, thetas)
    p = predictor(str(tmp_path / "solo"), likelihood=BernoulliLikelihood())
    assert p.numNetworks == 6 and np.array_equal(np.stack(p.vectors), thetas)
    w = ge.net_weights(6)
    out = check_predictor("predictor bernoulli", p, X, Y, "bernoulli", w, 6)
    assert out["total"].shape == (2, 301)
    for c in range(2):
        write_networks(str(tmp_path / "multi" / f"chain{c}"), dims, arch, thetas[3 * c:3 * c + 3])
    q = predictor.fromChains(str(tmp_path / "multi"), likelihood=BernoulliLikelihood())
    assert q.numChains == 2 and q.numNetworks == 6
    assert same_bits(q.predictUncertainty(X, weights=w), p.predictUncertainty(X, weights=w))
    a, b = q.calibration(X, Y), p.calibration(X, Y)
    assert a["ece"] == b["ece"] and a["brier"] == b["brier"]
