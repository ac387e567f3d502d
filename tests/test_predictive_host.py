"""The predictive distribution with observation noise (tbnn_ensemble_predictive) without a GPU: the built library exports the entry point,
the ctypes prototype agrees with the header argument by argument, the C-ABI version is as before, a null handle is refused before any device
is touched, and the predictor picks the networks, the per-network sd's, the likelihood and the probabilities its arguments ask for, applies
sd and mean on the host and refuses what has no predictive quantile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_ensemble_host import CTYPE, header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "tbnn_ensemble_predictive"


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
    assert len(protos[SYM]) == 16 and len(args) == 16
    for i, (a, w) in enumerate(zip(args, want)):
        assert a is w, (i, protos[SYM][i], a)
    txt = open(os.path.join(ROOT, "include", "tbnn.h")).read()
    assert re.search(r"#define TBNN_ABI_VERSION 3\b", txt)
    # the kernels are part of the checked unit, like the other reductions'
    hpp = open(os.path.join(ROOT, "tensorbnn_amd", "csrc", "kernels_ensemble.hpp")).read()
    assert "k_ens_pred_cdf" in hpp and "k_ens_pred_quantiles" in hpp


def test_null_handle_is_refused_with_a_message(native):
    z = np.full(4, 0.5, dtype=np.float64)
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    assert native.lib.tbnn_ensemble_predictive(None, None, 1, 1, 0, None, None, 1, None, None, 0, dp, 1, dp, None, None) < 0
    assert "null handle" in native.lib.tbnn_last_error().decode()
    assert np.all(z == 0.5)


class StubChain:
    """records what the predictor asks of Chain.ensemble_predictive / ensemble_loglik and answers with arrays of the right shape"""

    def __init__(self, d_out=2):
        self.calls = []
        self.d_out = d_out

    def ensemble_predictive(self, thetas, probs=None, Y=None, **kw):
        self.calls.append((np.asarray(thetas), None if probs is None else np.asarray(probs), Y, kw))
        rows = np.asarray(kw["X"]).shape[0]
        q = None
        if probs is not None:
            assert np.asarray(probs).ndim == 1
            q = np.arange(len(probs), dtype=np.float64)[:, None, None] + np.zeros((len(probs), self.d_out, rows))
        F = None if Y is None else np.full((self.d_out, rows), 0.75)
        Fb = None if Y is None or kw["likelihood"] != 5 else np.full((self.d_out, rows), 0.25)
        return q, F, Fb

    def ensemble_loglik(self, thetas, **kw):
        self.calls.append((np.asarray(thetas), None, kw.get("Y"), kw))
        return "per_net", "rows"


def stub_predictor(likelihood, hypers=(), m=6, P=5):
    from tensorbnn_amd.predictor import predictor
    p = predictor.__new__(predictor)                     # no saved networks, no device
    p.numNetworks = m
    p.vectors = [np.full(P, i, dtype=np.float32) for i in range(m)]
    p.hypers = list(hypers)
    p.likelihood = likelihood
    p._chain = StubChain()
    return p


X = np.zeros((3, 2), dtype=np.float32)
Y = np.zeros((3, 2), dtype=np.float32)
HYPERS = [np.arange(9, dtype=np.float32) + 10 * i for i in range(6)]          # last hyper of network i: 8 + 10 i


def test_predictor_picks_networks_sd_and_likelihood():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import FixedGaussianLikelihood, GaussianLikelihood, PoissonLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1), HYPERS)
    q = p.predictiveQuantiles(X, [0.25, 0.75], n=2)
    th, probs, y, kw = p._chain.calls[-1]
    assert q.shape == (2, 2, 3) and y is None
    assert th.shape == (3, 5) and np.array_equal(th[:, 0], [0, 2, 4])
    assert probs.dtype == np.float64 and np.array_equal(probs, [0.25, 0.75])
    assert kw["likelihood"] == nat.LIK_GAUSSIAN and kw["weights"] is None
    assert kw["sd"].dtype == np.float32 and np.array_equal(kw["sd"], np.float32([8, 28, 48]))      # each picked network's saved last hyper
    # ... 0.1 where no hypers were saved, the fixed sd under the fixed Gaussian, none under Poisson
    p = stub_predictor(GaussianLikelihood(sd=0.1))
    p.predictiveQuantiles(X, [0.5])
    assert np.array_equal(p._chain.calls[-1][3]["sd"], np.full(6, np.float32(0.1)))
    assert np.array_equal(p._chain.calls[-1][0][:, 0], np.arange(6))
    p.predictiveQuantiles(X, [0.5], likelihood=FixedGaussianLikelihood(sd=0.3), weights=[1, 0, 2, 0, 1, 1])
    kw = p._chain.calls[-1][3]
    assert kw["likelihood"] == nat.LIK_FIXED_GAUSSIAN and np.array_equal(kw["sd"], np.full(6, np.float32(0.3)))
    assert np.array_equal(kw["weights"], np.float32([1, 0, 2, 0, 1, 1]))
    p = stub_predictor(PoissonLikelihood(), HYPERS)
    p.predictiveQuantiles(X, [0.5])
    kw = p._chain.calls[-1][3]
    assert kw["likelihood"] == nat.LIK_POISSON and kw["sd"] is None
    with pytest.raises(ValueError, match="one value per picked network"):
        p.predictiveQuantiles(X, [0.5], n=2, weights=[1.0, 1.0])


def test_log_predictive_density_reads_the_same_sd():
    """the helper both share: logPredictiveDensity passes what it passed before"""
    from tensorbnn_amd.likelihood import FixedGaussianLikelihood, GaussianLikelihood, PoissonLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1), HYPERS)
    assert p.logPredictiveDensity(X, Y, n=2) == ("per_net", "rows")
    sd = p._chain.calls[-1][3]["sd"]
    assert sd.dtype == np.float32 and np.array_equal(sd, np.float32([8, 28, 48]))
    p.predictiveCDF(X, Y, n=2)
    assert np.array_equal(p._chain.calls[-1][3]["sd"], sd)
    p.logPredictiveDensity(X, Y, likelihood=FixedGaussianLikelihood(sd=0.3))
    assert np.array_equal(p._chain.calls[-1][3]["sd"], np.full(6, np.float32(0.3)))
    p.logPredictiveDensity(X, Y, likelihood=PoissonLikelihood())
    assert p._chain.calls[-1][3]["sd"] is None


def test_sd_and_mean_are_applied_on_the_host():
    from tensorbnn_amd.likelihood import GaussianLikelihood, PoissonLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1))
    q = p.predictiveQuantiles(X, [0.1, 0.5, 0.9], sd=3.0, mean=-1.0)
    assert "scale" not in p._chain.calls[-1][3] and "shift" not in p._chain.calls[-1][3]
    assert q.dtype == np.float64 and np.array_equal(q[:, 0, 0], [-1.0, 2.0, 5.0])                 # the stub's 0, 1, 2 times 3 minus 1
    assert np.array_equal(p.predictiveQuantiles(X, [0.1, 0.5, 0.9])[:, 1, 2], [0.0, 1.0, 2.0])
    calls = len(p._chain.calls)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="sd must be > 0"):
            p.predictiveQuantiles(X, [0.5], sd=bad)
    p.likelihood = PoissonLikelihood()
    for kw in ({"sd": 2.0}, {"mean": 1.0}):
        with pytest.raises(ValueError, match="PoissonLikelihood"):
            p.predictiveQuantiles(X, [0.5], **kw)
    assert len(p._chain.calls) == calls                  # refused before any native call
    assert p.predictiveQuantiles(X, [0.5], sd=1.0, mean=0.0).shape == (1, 2, 3)


def test_scalar_probs_drop_the_axis():
    from tensorbnn_amd.likelihood import GaussianLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1))
    assert p.predictiveQuantiles(X, 0.5).shape == (2, 3)
    assert np.array_equal(p._chain.calls[-1][1], [0.5])
    assert p.predictiveQuantiles(X, [0.5]).shape == (1, 2, 3)


def test_interval_asks_for_three_decimal_probabilities_in_one_call():
    from tensorbnn_amd.likelihood import GaussianLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1))
    lower, median, upper = p.predictiveInterval(X, level=0.9)
    assert len(p._chain.calls) == 1
    assert p._chain.calls[-1][1].tolist() == [0.05, 0.5, 0.95]
    assert lower.shape == median.shape == upper.shape == (2, 3)
    assert not lower.any() and np.all(median == 1.0) and np.all(upper == 2.0)          # the stub's answers, in order
    p.predictiveInterval(X)                                                          # the default level is 0.9
    assert p._chain.calls[-1][1].tolist() == [0.05, 0.5, 0.95]
    p.predictiveInterval(X, level=0.5, n=3, weights=[1.0, 2.0], sd=2.0)
    th, probs, _y, kw = p._chain.calls[-1]
    assert probs.tolist() == [0.25, 0.5, 0.75] and np.array_equal(th[:, 0], [0, 3])
    assert np.array_equal(kw["weights"], np.float32([1.0, 2.0]))
    for level in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="level"):
            p.predictiveInterval(X, level=level)


def test_cdf_returns_the_pit_values_and_a_pair_for_counts():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import GaussianLikelihood, PoissonLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1), HYPERS)
    F = p.predictiveCDF(X, Y, n=3, weights=[1.0, 3.0])
    th, probs, y, kw = p._chain.calls[-1]
    assert isinstance(F, np.ndarray) and F.shape == (2, 3) and np.all(F == 0.75)
    assert probs is None and y.dtype == np.float32 and y.shape == (3, 2)
    assert np.array_equal(th[:, 0], [0, 3]) and np.array_equal(kw["sd"], np.float32([8, 38]))
    assert kw["likelihood"] == nat.LIK_GAUSSIAN and np.array_equal(kw["weights"], np.float32([1.0, 3.0]))
    below, at = p.predictiveCDF(X, Y, likelihood=PoissonLikelihood())
    assert np.all(below == 0.25) and np.all(at == 0.75)
    assert p._chain.calls[-1][3]["likelihood"] == nat.LIK_POISSON and p._chain.calls[-1][3]["sd"] is None


def test_labels_are_refused_naming_predict_moments():
    from tensorbnn_amd.likelihood import BernoulliLikelihood, CategoricalLikelihood, GaussianLikelihood
    for lik in (BernoulliLikelihood(), CategoricalLikelihood()):
        p = stub_predictor(lik)
        for call in (lambda: p.predictiveQuantiles(X, [0.5]), lambda: p.predictiveInterval(X), lambda: p.predictiveCDF(X, Y)):
            with pytest.raises(ValueError, match="predictMoments"):
                call()
        assert not p._chain.calls
        p = stub_predictor(GaussianLikelihood(sd=0.1))
        with pytest.raises(ValueError, match="predictMoments"):
            p.predictiveQuantiles(X, [0.5], likelihood=lik)


def test_predict_interval_docstring_points_at_the_predictive_one():
    from tensorbnn_amd.predictor import predictor
    assert "predictiveInterval" in predictor.predictInterval.__doc__
