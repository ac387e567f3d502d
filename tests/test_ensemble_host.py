"""The ensemble reductions (tbnn_ensemble_moments / tbnn_ensemble_loglik) without a GPU: the built library exports both entry points, the
ctypes prototypes agree with the header argument by argument, the C-ABI version and the build-time check are as before, the entry points
refuse what they can judge before touching a device, and the predictor picks the transform and the per-network sd its likelihood asks for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tbnn_ensemble_moments", "tbnn_ensemble_loglik")

# C parameter type (as the header spells it, qualifiers and names stripped) -> the ctypes type _native must declare
CTYPE = {"tbnn_handle": C.c_void_p, "float*": C.POINTER(C.c_float), "double*": C.POINTER(C.c_double), "int32_t": C.c_int32,
         "int64_t": C.c_int64, "int": C.c_int, "float": C.c_float}


def header_prototypes():
    """{name: [parameter types]} of the tbnn_* functions of include/tbnn.h, comments stripped as tests/test_cabi.py strips them"""
    txt = open(os.path.join(ROOT, "include", "tbnn.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {}
    for name, args in re.findall(r"\bint\s+(tbnn_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        types = []
        for a in args.split(","):
            a = a.replace("const", " ").strip()
            star = "*" if "*" in a else ""
            base = a.replace("*", " ").split()[0]
            types.append(base + star)
        protos[name] = types
    return protos


def test_library_exports_both_symbols(native):
    lib = C.CDLL(native.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), f"{s} not exported by {native.LIB_PATH}"
    assert native.lib.tbnn_abi_version() == native.ABI_VERSION == 3


def test_native_prototypes_match_the_header(native):
    protos = header_prototypes()
    bound = {name: (res, args) for name, res, args in native.SYMBOLS}
    for s in NEW:
        assert s in protos, f"{s} not declared in include/tbnn.h"
        assert s in bound, f"{s} not in _native.SYMBOLS"
        res, args = bound[s]
        assert res is C.c_int
        want = [CTYPE[t] for t in protos[s]]
        assert len(args) == len(want), (s, len(args), len(want))
        for i, (a, w) in enumerate(zip(args, want)):
            assert a is w, (s, i, protos[s][i], a)
    assert len(protos["tbnn_ensemble_moments"]) == 13 and len(protos["tbnn_ensemble_loglik"]) == 13
    assert (native.XFORM_NONE, native.XFORM_EXP, native.XFORM_SIGMOID, native.XFORM_SOFTMAX) == (0, 1, 2, 3)
    txt = open(os.path.join(ROOT, "include", "tbnn.h")).read()
    assert re.search(r"TBNN_XFORM_NONE = 0, TBNN_XFORM_EXP = 1, TBNN_XFORM_SIGMOID = 2, TBNN_XFORM_SOFTMAX = 3", txt)
    assert re.search(r"#define TBNN_ABI_VERSION 3\b", txt)


def test_lint_status_reports_every_unit_checked(native):
    st = native.lint_status()
    for unit in ("tbnn_api.hip", "tbnn_narrow.hip", "tbnn_wide.hip", "tbnn_mid.hip", "tbnn_tall.hip"):
        assert re.search(re.escape(unit) + r": listing checked[^;]*; disassembly clean", st), (unit, st)
    # the reductions' kernels are part of the checked unit: the header is included by tbnn_api.hip, not built on its own
    api = open(os.path.join(ROOT, "tensorbnn_amd", "csrc", "tbnn_api.hip")).read()
    assert '#include "kernels_ensemble.hpp"' in api


def test_null_handle_is_refused_with_a_message(native):
    z = np.zeros(4, dtype=np.float64)
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    assert native.lib.tbnn_ensemble_moments(None, None, 1, 1, None, 0, 1.0, 0.0, 1, None, 0, dp, None) < 0
    assert "null handle" in native.lib.tbnn_last_error().decode()
    assert native.lib.tbnn_ensemble_loglik(None, None, 1, 1, 0, None, None, 1, None, None, 0, dp, None) < 0
    assert "null handle" in native.lib.tbnn_last_error().decode()


class StubChain:
    """records what the predictor asks of Chain.ensemble_moments / ensemble_loglik"""

    def __init__(self):
        self.calls = []

    def ensemble_moments(self, thetas, **kw):
        self.calls.append(("moments", np.asarray(thetas), kw))
        return "mean", "var"

    def ensemble_loglik(self, thetas, **kw):
        self.calls.append(("loglik", np.asarray(thetas), kw))
        return "per_net", "rows"


def stub_predictor(likelihood, hypers, m=6, P=5):
    from tensorbnn_amd.predictor import predictor
    p = predictor.__new__(predictor)                     # no saved networks, no device
    p.numNetworks = m
    p.vectors = [np.full(P, i, dtype=np.float32) for i in range(m)]
    p.hypers = hypers
    p.likelihood = likelihood
    p._chain = StubChain()
    return p


def test_predictor_picks_the_transform():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import BernoulliLikelihood, CategoricalLikelihood, FixedGaussianLikelihood, GaussianLikelihood
    X = np.zeros((3, 2), dtype=np.float32)
    for lik, want in ((CategoricalLikelihood(), nat.XFORM_SOFTMAX), (GaussianLikelihood(sd=0.1), nat.XFORM_NONE),
                      (FixedGaussianLikelihood(sd=0.3), nat.XFORM_NONE), (BernoulliLikelihood(), nat.XFORM_NONE)):
        p = stub_predictor(lik, [])
        assert p.predictMoments(X) == ("mean", "var")
        kind, th, kw = p._chain.calls[-1]
        assert kind == "moments" and kw["xform"] == want and kw["weights"] is None and kw["scale"] == 1.0 and kw["shift"] == 0.0
        assert th.shape == (6, 5) and np.array_equal(th[:, 0], np.arange(6))
    p = stub_predictor(CategoricalLikelihood(), [])
    for name, want in (("exp", nat.XFORM_EXP), ("sigmoid", nat.XFORM_SIGMOID), ("softmax", nat.XFORM_SOFTMAX), ("none", nat.XFORM_NONE)):
        p.predictMoments(X, n=2, weights=[0.5, 0.25, 0.25], transform=name, sd=3.0, mean=-1.0)
        kind, th, kw = p._chain.calls[-1]
        assert kw["xform"] == want and kw["scale"] == 3.0 and kw["shift"] == -1.0
        assert np.array_equal(th[:, 0], [0, 2, 4]) and np.array_equal(kw["weights"], np.float32([0.5, 0.25, 0.25]))
    with pytest.raises(ValueError, match="transform"):
        p.predictMoments(X, transform="tanh")
    with pytest.raises(ValueError, match="one value per picked network"):
        p.predictMoments(X, n=2, weights=[1.0, 1.0])


def test_predictor_picks_sd_per_likelihood():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import BernoulliLikelihood, CategoricalLikelihood, FixedGaussianLikelihood, GaussianLikelihood
    X = np.zeros((3, 2), dtype=np.float32)
    Y = np.zeros((3, 1), dtype=np.float32)
    hypers = [np.arange(9, dtype=np.float32) + 10 * i for i in range(6)]          # last hyper of network i: 8 + 10 i
    # Gaussian: each picked network's saved last hyper, as _data_logprob reads it (not squared)
    p = stub_predictor(GaussianLikelihood(sd=0.1), hypers)
    assert p.logPredictiveDensity(X, Y, n=2) == ("per_net", "rows")
    kind, th, kw = p._chain.calls[-1]
    assert kind == "loglik" and kw["likelihood"] == nat.LIK_GAUSSIAN
    assert np.array_equal(kw["sd"], np.float32([8, 28, 48])) and np.array_equal(th[:, 0], [0, 2, 4])
    # ... and 0.1 where no hypers were saved
    p = stub_predictor(GaussianLikelihood(sd=0.1), [])
    p.logPredictiveDensity(X, Y)
    assert np.array_equal(p._chain.calls[-1][2]["sd"], np.full(6, np.float32(0.1)))
    # fixed Gaussian: its own sd for every network; an explicit likelihood overrides the predictor's
    p.logPredictiveDensity(X, Y, likelihood=FixedGaussianLikelihood(sd=0.3), weights=np.ones(6))
    kw = p._chain.calls[-1][2]
    assert kw["likelihood"] == nat.LIK_FIXED_GAUSSIAN and np.array_equal(kw["sd"], np.full(6, np.float32(0.3)))
    assert np.array_equal(kw["weights"], np.ones(6, dtype=np.float32))
    for lik in (BernoulliLikelihood(), CategoricalLikelihood()):
        p.logPredictiveDensity(X, Y, likelihood=lik)
        kw = p._chain.calls[-1][2]
        assert kw["likelihood"] == lik.kind and kw["sd"] is None
