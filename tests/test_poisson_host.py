"""PoissonLikelihood (TBNN_LIK_POISSON) without a GPU: the Python descriptor and its fp64 helper against math.lgamma, the predictor's data
term and count variance switch, the C ABI's admission rules (tbnn_fused_kernel_available runs the descriptor checks of tbnn_create on the
host), and the run-time kernel plumbing -- the Poisson code reaches every family the Gaussian code reaches (the weighted bit included),
never shares a table or a cache entry with another likelihood, and a narrow and a mid-width library cross-compile for gfx950 through the
checked compile."""
import ctypes as C
import math
import os

import numpy as np
import pytest

DIMS_GRID = ([1, 10, 10, 1], [5, 50, 50, 50, 1], [7, 17, 33, 2], [2, 12, 1], [1, 100, 1], [5, 20, 20, 3], [20, 64, 64, 1], [30, 80, 80, 10],
             [20, 100, 100, 2], [784, 20, 20, 1], [784, 20, 20, 10], [300, 33, 3], [10, 200, 200, 1], [10, 200, 200, 10], [8, 90, 130, 70, 3],
             [20, 64, 64, 20], [8, 300, 300, 1], [40, 24, 24, 3])


def layers_for(dims, hidden_act, last_act=0):
    return [(dims[i], dims[i + 1], hidden_act if i < len(dims) - 2 else last_act, 0) for i in range(len(dims) - 1)]


def test_descriptor_fields():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import PoissonLikelihood
    lik = PoissonLikelihood()
    assert nat.LIK_POISSON == 5 and lik.kind == nat.LIK_POISSON
    assert lik.hypers == [] and lik.mainProbsInHypers is False
    assert lik.display([]) is None
    assert lik.calcultateLogProb(hypers=[1, 2, 3]) == [0, 0, 0]
    assert nat.ABI_VERSION == 3


def test_response_likelihood_is_the_fp64_poisson_log_density():
    from tensorbnn_amd.likelihood import PoissonLikelihood
    rng = np.random.default_rng(3)
    n, k = 41, 3
    f = rng.uniform(-3, 6, (k, n)).astype(np.float32)                    # [d_out, rows] log-rates, as network.predict returns
    y = rng.poisson(np.exp(f.T.astype(np.float64))).astype(np.float32)   # [rows, d_out] counts
    y[0] = [0.0, 2.5, 170.25]                                            # zero, non-integers (lgamma generalises the factorial)
    f[:, 1], y[1] = np.log(2.5), [3, 0, 7]                               # a small rate with integer counts
    out = PoissonLikelihood().makeResponseLikelihood(None, predict=lambda train, _x: f, realVals=y)
    assert out.shape == (k, n) and out.dtype == np.float64 and np.all(np.isfinite(out))
    for o_ in range(k):
        for r in range(n):
            fv, yv = float(f[o_, r]), float(y[r, o_])
            assert math.isclose(out[o_, r], yv * fv - math.exp(fv) - math.lgamma(yv + 1.0), rel_tol=1e-13, abs_tol=1e-13)
    # integer counts: the log of the Poisson mass function
    for o_, cnt in enumerate((3, 0, 7)):
        rate = math.exp(float(f[o_, 1]))
        assert math.isclose(out[o_, 1], math.log(math.exp(-rate) * rate ** cnt / math.factorial(cnt)), rel_tol=1e-12)


def test_predictor_data_term_and_count_variance():
    from tensorbnn_amd.likelihood import PoissonLikelihood
    from tensorbnn_amd.predictor import predictor
    rng = np.random.default_rng(5)
    X = rng.standard_normal((20, 2)).astype(np.float32)
    preds = [rng.uniform(-2, 4, (2, 20)).astype(np.float32) for _ in range(2)]
    Y = rng.poisson(np.exp(preds[0].T.astype(np.float64))).astype(np.float32)
    p = predictor.__new__(predictor)                     # no saved networks, no device: only the host-side steps
    p.predict = lambda x, n=1: preds
    p.hypers = []
    got = p._data_logprob(PoissonLikelihood(), X, Y, 1)
    lg = np.vectorize(math.lgamma)
    for g, f in zip(got, preds):
        f64, y64 = f.T.astype(np.float64), Y.astype(np.float64)
        assert np.isclose(g, (y64 * f64 - np.exp(f64) - lg(y64 + 1.0)).sum(), rtol=1e-6)
    assert got[0] > got[1]                               # the counts were drawn from the first network's rates

    class FakeChain:
        def ensemble_moments(self, picked, X=None, weights=None, xform=None, scale=1.0, shift=0.0):
            self.xform = xform
            return np.full((2, 20), 3.0), np.full((2, 20), 0.5)
    p.likelihood, p.vectors, p.numNetworks = PoissonLikelihood(), [np.zeros(4, np.float32)] * 2, 2
    p._chain = FakeChain()
    from tensorbnn_amd import _native as nat
    m, v = p.predictMoments(X)
    assert p._chain.xform == nat.XFORM_EXP and np.all(m == 3.0) and np.all(v == 0.5)      # rate: exp by default
    m, v = p.predictMoments(X, countVariance=True)
    assert np.all(m == 3.0) and np.all(v == 3.5)                                          # E[rate] + Var[rate]
    with pytest.raises(ValueError, match="countVariance"):
        p.predictMoments(X, transform="none", countVariance=True)


def test_softmax_rejection_text_is_untouched():
    from tensorbnn_amd.activationFunctions import Softmax
    with pytest.raises(NotImplementedError, match="CategoricalLikelihood"):
        Softmax()


def _admission(dims, act_last, lik):
    from tensorbnn_amd import _native as nat
    layers = layers_for(dims, nat.ACT_RELU, act_last)
    arr = (nat.LayerDesc * len(layers))(*[nat.LayerDesc(*l) for l in layers])
    desc = nat.NetDesc(len(layers), arr, lik, 0.1, nat.KERNEL_AUTO, 0)
    rc = nat.lib.tbnn_fused_kernel_available(C.byref(desc))
    return rc, nat.lib.tbnn_last_error().decode()


def test_c_abi_admission():
    from tensorbnn_amd import _native as nat
    for dims in ([5, 8, 1], [5, 8, 3], [5, 8, 40]):                       # any d_out >= 1
        assert _admission(dims, nat.ACT_NONE, nat.LIK_POISSON)[0] >= 0
    for act in (nat.ACT_EXP, nat.ACT_SIGMOID, nat.ACT_RELU):
        rc, err = _admission([5, 8, 1], act, nat.LIK_POISSON)
        assert rc == -1 and "log-rate" in err and "no activation" in err, err
    for unknown in (4, 6, -1):                                           # (4 stays unassigned: tests/test_categorical_host.py)
        rc, err = _admission([5, 8, 3], nat.ACT_NONE, unknown)
        assert rc == -1 and "unknown likelihood" in err
    # an ahead-of-time Gaussian table is no table for the Poisson network of the same layers (tbnn_mid.hip: relu;7,33,18,50,2)
    dims = [7, 33, 18, 50, 2]
    assert _admission(dims, nat.ACT_NONE, nat.LIK_GAUSSIAN)[0] > 0
    assert _admission(dims, nat.ACT_NONE, nat.LIK_POISSON)[0] == 0
    assert _admission([5, 50, 50, 50, 1], nat.ACT_NONE, nat.LIK_GAUSSIAN)[0] > 0
    assert _admission([5, 50, 50, 50, 1], nat.ACT_NONE, nat.LIK_POISSON)[0] == 0


def test_lik_code_shape_and_cache_key():
    from tensorbnn_amd import _native as nat, jit
    assert jit.LIK_POIS == 3 and jit.lik_code(nat.LIK_POISSON) == 3 and jit.lik_code(nat.LIK_POISSON, True) == 3 | jit.LIK_WEIGHTED
    layers = layers_for([30, 80, 80, 10], nat.ACT_RELU)
    g, c, b, p, pw = (jit.shape_of(layers, lk, w) for lk, w in ((nat.LIK_GAUSSIAN, False), (nat.LIK_CATEGORICAL, False), (nat.LIK_BERNOULLI, False),
                                                               (nat.LIK_POISSON, False), (nat.LIK_POISSON, True)))
    assert g[:3] == p[:3] == pw[:3] and len({g[3], c[3], b[3], p[3], pw[3]}) == 5
    assert len({jit.cache_key(*s) for s in (g, c, b, p, pw)}) == 5
    src = jit.source(*p, "mid")
    assert "SHAPE_LIK_POIS" in src.split("Shape<")[1].split(">")[0] and src != jit.source(*g, "mid")
    assert ", 7, " in jit.source(*pw, "mid").split("Shape<")[1]           # weighted: the numeric code 3 | 4


@pytest.mark.parametrize("dims", DIMS_GRID, ids=lambda d: "-".join(map(str, d)))
def test_families_equal_the_gaussian_reach(dims):
    from tensorbnn_amd import jit
    want = jit.families(dims, jit.LIK_GAUSS)
    assert jit.families(dims, jit.LIK_POIS) == want == jit.families(dims)
    assert jit.families(dims, jit.LIK_POIS | jit.LIK_WEIGHTED) == jit.families(dims, jit.LIK_GAUSS | jit.LIK_WEIGHTED) == want


def test_families_reach_the_narrow_kernels_and_small_outputs():
    from tensorbnn_amd import jit
    P = jit.LIK_POIS
    assert jit.families([5, 50, 50, 50, 1], P)[0] == "fast3" and "fast" in jit.families([5, 50, 50, 50, 1], P)
    assert jit.families([1, 10, 10, 1], P)[0] == "fast3"
    assert jit.families([20, 100, 100, 2], P) == ["mid", "wide"] and jit.families([20, 100, 100, 2], jit.LIK_CAT) == []
    assert jit.families([784, 20, 20, 1], P) == ["tall"]
    assert jit.families([30, 80, 80, 10], P) == ["mid", "wide"]


@pytest.mark.parametrize("dims,skip,family,name", [
    ([3, 12, 12, 1], "", "fast3", b"<relu,none,poisson;3,12,12,1>"),
    ([20, 64, 64, 3], "wide", "mid", b"jit-mid<relu,none,poisson;20,64,64,3>"),
])
def test_poisson_library_cross_compiles_checked(tmp_path, monkeypatch, dims, skip, family, name):
    """jit.build of a narrow and a mid-width Poisson shape: hipcc for gfx950 through checked_compile, the MFMA hazard check clean"""
    from tensorbnn_amd import _native as nat, jit
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    monkeypatch.setenv("TBNN_JIT_DIR", str(tmp_path))
    monkeypatch.setenv("TBNN_JIT_SKIP", skip)
    so = jit.build(layers_for(dims, nat.ACT_RELU), nat.LIK_POISSON)
    assert so and os.path.exists(so)
    st = jit.lint_status(so)
    assert st.startswith(family + ":") and "listing checked" in st and "disassembly clean" in st, st
    lib = C.CDLL(so)
    buf = (C.c_char * 4096)()
    assert lib.tbnn_jit_ops(buf) == 0
    assert name in bytes(buf), bytes(buf)[:400]
