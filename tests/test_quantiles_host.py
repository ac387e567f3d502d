"""The ensemble quantiles (tbnn_ensemble_quantiles) without a GPU: the built library exports the entry point, the ctypes prototype agrees
with the header argument by argument, the C-ABI version is as before, a null handle is refused before any device is touched, and the
predictor picks the networks, the transform, the method and the probabilities its arguments ask for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_ensemble_host import CTYPE, header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "tbnn_ensemble_quantiles"


def test_library_exports_the_symbol(native):
    lib = C.CDLL(native.LIB_PATH)
    assert hasattr(lib, SYM), f"{SYM} not exported by {native.LIB_PATH}"
    assert native.lib.tbnn_abi_version() == native.ABI_VERSION == 3


def test_native_prototype_matches_the_header(native):
    protos = header_prototypes()
    bound = {name: (res, args) for name, res, args in native.SYMBOLS}
    assert SYM in protos, f"{SYM} not declared in include/tbnn.h"
    assert SYM in bound, f"{SYM} not in _native.SYMBOLS"
    res, args = bound[SYM]
    assert res is C.c_int
    want = [CTYPE[t] for t in protos[SYM]]
    assert len(protos[SYM]) == 15 and len(args) == 15
    for i, (a, w) in enumerate(zip(args, want)):
        assert a is w, (i, protos[SYM][i], a)
    assert (native.QUANT_LINEAR, native.QUANT_INVERTED_CDF) == (0, 1)
    txt = open(os.path.join(ROOT, "include", "tbnn.h")).read()
    assert re.search(r"TBNN_QUANT_LINEAR = 0, TBNN_QUANT_INVERTED_CDF = 1", txt)
    assert re.search(r"#define TBNN_ABI_VERSION 3\b", txt)


def test_null_handle_is_refused_with_a_message(native):
    z = np.zeros(4, dtype=np.float64)
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    assert native.lib.tbnn_ensemble_quantiles(None, None, 1, 1, None, 0, 0, 1.0, 0.0, 1, None, 0, dp, 1, dp) < 0
    assert "null handle" in native.lib.tbnn_last_error().decode()


class StubChain:
    """records what the predictor asks of Chain.ensemble_quantiles and answers with an array of the right shape"""

    def __init__(self, d_out=2):
        self.calls = []
        self.d_out = d_out

    def ensemble_quantiles(self, thetas, probs, **kw):
        probs = np.asarray(probs)
        self.calls.append((np.asarray(thetas), probs, kw))
        assert probs.ndim == 1
        rows = np.asarray(kw["X"]).shape[0]
        return np.arange(probs.size, dtype=np.float64)[:, None, None] + np.zeros((probs.size, self.d_out, rows))


def stub_predictor(likelihood, m=6, P=5):
    from tensorbnn_amd.predictor import predictor
    p = predictor.__new__(predictor)                     # no saved networks, no device
    p.numNetworks = m
    p.vectors = [np.full(P, i, dtype=np.float32) for i in range(m)]
    p.hypers = []
    p.likelihood = likelihood
    p._chain = StubChain()
    return p


X = np.zeros((3, 2), dtype=np.float32)


def test_predictor_picks_every_nth_network_and_passes_scale_and_shift():
    from tensorbnn_amd.likelihood import GaussianLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1))
    q = p.predictQuantiles(X, [0.25, 0.75], n=2, sd=3.0, mean=-1.0)
    th, probs, kw = p._chain.calls[-1]
    assert q.shape == (2, 2, 3)
    assert th.shape == (3, 5) and np.array_equal(th[:, 0], [0, 2, 4])
    assert probs.dtype == np.float64 and np.array_equal(probs, [0.25, 0.75])
    assert kw["scale"] == 3.0 and kw["shift"] == -1.0 and kw["weights"] is None
    p.predictQuantiles(X, [0.5])
    assert np.array_equal(p._chain.calls[-1][0][:, 0], np.arange(6))
    with pytest.raises(ValueError, match="one value per picked network"):
        p.predictQuantiles(X, [0.5], n=2, weights=[1.0, 1.0])


def test_predictor_default_transform_follows_the_likelihood():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import (BernoulliLikelihood, CategoricalLikelihood, FixedGaussianLikelihood, GaussianLikelihood,
                                          PoissonLikelihood)
    for lik, want in ((CategoricalLikelihood(), nat.XFORM_SOFTMAX), (PoissonLikelihood(), nat.XFORM_EXP), (GaussianLikelihood(sd=0.1), nat.XFORM_NONE),
                      (FixedGaussianLikelihood(sd=0.3), nat.XFORM_NONE), (BernoulliLikelihood(), nat.XFORM_NONE)):
        p = stub_predictor(lik)
        p.predictQuantiles(X, [0.5])
        assert p._chain.calls[-1][2]["xform"] == want, type(lik).__name__
    p = stub_predictor(CategoricalLikelihood())
    for name, want in (("exp", nat.XFORM_EXP), ("sigmoid", nat.XFORM_SIGMOID), ("softmax", nat.XFORM_SOFTMAX), ("none", nat.XFORM_NONE)):
        p.predictQuantiles(X, [0.5], transform=name)
        assert p._chain.calls[-1][2]["xform"] == want
    with pytest.raises(ValueError, match="transform"):
        p.predictQuantiles(X, [0.5], transform="tanh")


def test_predictor_default_method_follows_the_weights():
    from tensorbnn_amd.likelihood import GaussianLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1))
    p.predictQuantiles(X, [0.5])
    assert p._chain.calls[-1][2]["method"] == "linear"
    w = [0.5, 0.25, 0.25, 0, 0, 0]
    p.predictQuantiles(X, [0.5], weights=w)
    assert p._chain.calls[-1][2]["method"] == "inverted_cdf"
    assert np.array_equal(p._chain.calls[-1][2]["weights"], np.float32(w))
    p.predictQuantiles(X, [0.5], method="inverted_cdf")
    assert p._chain.calls[-1][2]["method"] == "inverted_cdf" and p._chain.calls[-1][2]["weights"] is None
    calls = len(p._chain.calls)
    with pytest.raises(ValueError, match="linear"):
        p.predictQuantiles(X, [0.5], weights=w, method="linear")
    with pytest.raises(ValueError, match="method"):
        p.predictQuantiles(X, [0.5], method="median_unbiased")
    assert len(p._chain.calls) == calls                  # refused before any native call


def test_scalar_probs_drop_the_axis():
    from tensorbnn_amd.likelihood import GaussianLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1))
    q = p.predictQuantiles(X, 0.5)
    assert q.shape == (2, 3)
    assert np.array_equal(p._chain.calls[-1][1], [0.5])
    assert p.predictQuantiles(X, [0.5]).shape == (1, 2, 3)


def test_interval_asks_for_three_probabilities_in_one_call():
    from tensorbnn_amd.likelihood import GaussianLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1))
    lower, median, upper = p.predictInterval(X, level=0.9)
    assert len(p._chain.calls) == 1
    assert p._chain.calls[-1][1].tolist() == [0.05, 0.5, 0.95]
    assert lower.shape == median.shape == upper.shape == (2, 3)
    assert not lower.any() and np.all(median == 1.0) and np.all(upper == 2.0)          # the stub's answers, in order
    p.predictInterval(X)                                                             # the default level is 0.9
    assert p._chain.calls[-1][1].tolist() == [0.05, 0.5, 0.95]
    p.predictInterval(X, level=0.5, n=3, weights=[1.0, 2.0], sd=2.0)
    th, probs, kw = p._chain.calls[-1]
    assert probs.tolist() == [0.25, 0.5, 0.75] and np.array_equal(th[:, 0], [0, 3])
    assert kw["method"] == "inverted_cdf" and kw["scale"] == 2.0
    for level in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="level"):
            p.predictInterval(X, level=level)
