"""CategoricalLikelihood without a GPU: the Python descriptor and its NumPy helpers, the accuracy metric, the predictor's data term, the
C ABI's admission rules (tbnn_fused_kernel_available runs the descriptor checks of tbnn_create on the host), and the run-time kernel
plumbing -- a categorical network must never share a kernel table, a cache entry or a family list with the Gaussian network of the same
layers, and its mid-width library cross-compiles for gfx950 through the checked compile."""
import ctypes as C
import os

import numpy as np
import pytest


def fp64_log_softmax(f, axis):
    f = np.asarray(f, dtype=np.float64)
    m = f.max(axis=axis, keepdims=True)
    return f - m - np.log(np.exp(f - m).sum(axis=axis, keepdims=True))


def layers_for(dims, hidden_act, last_act=0):
    return [(dims[i], dims[i + 1], hidden_act if i < len(dims) - 2 else last_act, 0) for i in range(len(dims) - 1)]


def test_descriptor_fields():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import CategoricalLikelihood
    lik = CategoricalLikelihood()
    assert nat.LIK_CATEGORICAL == 3 and lik.kind == nat.LIK_CATEGORICAL
    assert lik.hypers == [] and lik.mainProbsInHypers is False
    assert lik.display([]) is None
    assert nat.ABI_VERSION == 3


def test_response_likelihood_is_the_fp64_log_softmax():
    from tensorbnn_amd.likelihood import CategoricalLikelihood
    rng = np.random.default_rng(3)
    n, k = 37, 5
    f = (rng.standard_normal((k, n)) * 4).astype(np.float32)             # [d_out, rows], as network.predict returns
    f[:, 0] = [80, -80, 0, 79.5, -3]                                     # saturated logits stay finite
    y = np.eye(k, dtype=np.float32)[rng.integers(0, k, n)]               # one-hot rows [rows, d_out]
    y[1] = [0.1, 0.2, 0.3, 0.4, 0.0]                                     # a soft row
    out = CategoricalLikelihood().makeResponseLikelihood(None, predict=lambda train, _x: f, realVals=y)
    want = y.T.astype(np.float64) * fp64_log_softmax(f, axis=0)
    assert out.shape == (k, n) and np.all(np.isfinite(out))
    np.testing.assert_allclose(out, want, rtol=1e-12, atol=1e-12)
    assert np.isclose(out.sum(), (y * fp64_log_softmax(f.T, axis=1)).sum(), rtol=1e-12)


def test_categorical_accuracy():
    from tensorbnn_amd.metrics import CategoricalAccuracy
    f_train = np.array([[2.0, 0.1, -1.0], [0.0, 3.0, 0.5], [1.0, 1.5, 4.0], [5.0, 0.0, 0.0]]).T      # [d_out, rows]: classes 0, 1, 2, 0
    y_train = np.eye(3)[[0, 1, 1, 0]]                                                               # 3 of 4 right
    f_val = np.array([[0.0, -1.0, 2.0], [9.0, 1.0, 1.0]]).T                                         # classes 2, 0
    y_val = np.array([[0.1, 0.2, 0.7], [0.6, 0.3, 0.1]])                                            # soft rows: argmax 2, 0
    m = CategoricalAccuracy(mean=5.0, sd=3.0, scaleExp=True)                                        # ignored for logits
    m.calculate(f_train, f_val, y_train, y_val)
    assert m.accuracyTrain == 0.75 and m.accuracyValidate == 1.0
    m.display()


def test_predictor_data_term():
    from tensorbnn_amd.likelihood import CategoricalLikelihood
    from tensorbnn_amd.predictor import predictor
    rng = np.random.default_rng(5)
    X = rng.standard_normal((20, 2)).astype(np.float32)
    Y = np.eye(4, dtype=np.float32)[rng.integers(0, 4, 20)]
    preds = [rng.standard_normal((4, 20)).astype(np.float32) * s for s in (1.0, 10.0)]
    p = predictor.__new__(predictor)                     # no saved networks, no device: only the data term
    p.predict = lambda x, n=1: preds
    p.hypers = []
    got = p._data_logprob(CategoricalLikelihood(), X, Y, 1)
    for g, f in zip(got, preds):
        assert np.isclose(g, (Y * fp64_log_softmax(f.T, axis=1)).sum(), rtol=1e-6)


def test_softmax_activation_still_refused_and_points_at_the_likelihood():
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
    rc, _ = _admission([5, 8, 3], nat.ACT_NONE, nat.LIK_CATEGORICAL)
    assert rc >= 0
    rc, err = _admission([5, 8, 1], nat.ACT_NONE, nat.LIK_CATEGORICAL)
    assert rc == -1 and "at least 2 outputs" in err
    rc, err = _admission([5, 8, 3], nat.ACT_SIGMOID, nat.LIK_CATEGORICAL)
    assert rc == -1 and "no activation" in err
    rc, err = _admission([5, 8, 3], nat.ACT_NONE, 4)
    assert rc == -1 and "unknown likelihood" in err
    # an ahead-of-time Gaussian table is no table for the categorical network of the same layers (tbnn_mid.hip: relu;7,33,18,50,2): only
    # the exact likelihood code matches -- "not Bernoulli" is not "Gaussian"
    dims = [7, 33, 18, 50, 2]
    assert _admission(dims, nat.ACT_NONE, nat.LIK_GAUSSIAN)[0] > 0
    assert _admission(dims, nat.ACT_NONE, nat.LIK_FIXED_GAUSSIAN)[0] > 0
    assert _admission(dims, nat.ACT_NONE, nat.LIK_CATEGORICAL)[0] == 0


def test_shape_and_cache_key_tell_categorical_from_gaussian():
    from tensorbnn_amd import _native as nat, jit
    layers = layers_for([30, 80, 80, 10], nat.ACT_RELU)
    g, c, b, fg = (jit.shape_of(layers, lk) for lk in (nat.LIK_GAUSSIAN, nat.LIK_CATEGORICAL, nat.LIK_BERNOULLI, nat.LIK_FIXED_GAUSSIAN))
    assert g[:3] == c[:3] and g[3] != c[3] and len({g[3], c[3], b[3]}) == 3
    assert fg == g                                                       # fixed-sd Gaussian shares the Gaussian kernels
    assert jit.cache_key(*g) != jit.cache_key(*c)
    assert jit.cache_key(*b) != jit.cache_key(*c)
    src_g, src_c = jit.source(*g, "mid"), jit.source(*c, "mid")
    assert "false" in src_g.split("Shape<")[1].split(">")[0]
    assert "SHAPE_LIK_CAT" in src_c and src_g != src_c


def test_families_for_categorical():
    from tensorbnn_amd import jit
    C_ = jit.LIK_CAT
    # narrow networks: fast3 / fast (and their trajectory kernel) compute the likelihood per element -- gone; mid takes 3 .. 16 outputs
    assert "fast" in jit.families([5, 20, 20, 3]) or "fast3" in jit.families([5, 20, 20, 3])
    fams = jit.families([5, 20, 20, 3], C_)
    assert "fast" not in fams and "fast3" not in fams
    assert fams == [f for f in jit.families([5, 20, 20, 3]) if f in ("mid", "tall", "wide")]
    assert jit.families([5, 20, 3], C_) == []                             # narrow only: the layered family
    assert jit.families([30, 80, 80, 10], C_) == ["mid", "wide"]
    assert jit.families([784, 20, 20, 10], C_) == ["tall"]
    assert jit.families([300, 33, 3], C_) == ["tall"]
    assert jit.families([10, 200, 200, 10], C_) == ["wide"]
    # two outputs: the mid / tall / wide kernels run their last layer on the VALU (per element): the layered family
    assert jit.families([20, 100, 100, 2], C_) == [] and jit.families([20, 100, 100, 2]) == ["mid", "wide"]
    assert jit.families([20, 64, 64, 20], C_) == []                       # more than one output tile: the layered family
    # nothing changes for the other likelihoods
    for dims in ([5, 50, 50, 50, 1], [20, 100, 100, 2], [784, 20, 20, 1]):
        assert jit.families(dims, jit.LIK_GAUSS) == jit.families(dims, jit.LIK_BERN) == jit.families(dims)


def test_categorical_mid_library_cross_compiles_checked(tmp_path, monkeypatch):
    """jit.build of a categorical mid-width shape: hipcc for gfx950 through checked_compile, the MFMA hazard check clean"""
    from tensorbnn_amd import _native as nat, jit
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    monkeypatch.setenv("TBNN_JIT_DIR", str(tmp_path))
    monkeypatch.setenv("TBNN_JIT_SKIP", "wide")
    so = jit.build(layers_for([20, 64, 64, 3], nat.ACT_RELU), nat.LIK_CATEGORICAL)
    assert so and os.path.exists(so)
    st = jit.lint_status(so)
    assert st.startswith("mid:") and "listing checked" in st and "disassembly clean" in st, st
    lib = C.CDLL(so)
    from tensorbnn_amd import _native  # noqa: F401  (FusedOps layout: read the name the table reports)
    buf = (C.c_char * 4096)()
    assert lib.tbnn_jit_ops(buf) == 0
    assert b"jit-mid<relu,none,categorical;20,64,64,3>" in bytes(buf)
