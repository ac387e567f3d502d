"""PSIS-LOO and WAIC (tbnn_ensemble_loo) without a GPU.  tests/psis_ref.py, the NumPy restatement the GPU tests compare the device against,
is checked here against things it was not written from: tails that ARE generalised Pareto (scipy.stats.genpareto's quantiles) give their
shape back, the invariances the estimator has by construction hold, and the tail-length table of the definition.  Then the plumbing: the
library exports the entry point, the ctypes prototype agrees with the header, a null handle is refused before any device is touched, and the
predictor's loo / waic / compareLoo do their host arithmetic on what the chain returns."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from psis_ref import gpd_fit, psis_ref, tail_length
from test_ensemble_host import CTYPE, header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "tbnn_ensemble_loo"


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("k", [-0.3, 0.0, 0.4, 0.9])
def test_fit_recovers_the_shape_of_a_pareto_tail(k):
    """M = 2000 exact quantiles at p_j = (j - 1/2) / M: the fit's standard error is about (1 + k) / sqrt(M) <= 0.05 there, and the prior
    moves k by 10 (1/2 - k) / (M + 10) < 0.005; the bound is 0.15.  First the fit alone, then through psis_ref: m = 10,000 networks with
    r_eff = 0.02 give M = min(2000, 3 sqrt(500,000) = 2121) = 2000, the ratios of the tail 1 + y_j above a bulk below 1."""
    from scipy.stats import genpareto
    M = 2000
    y = genpareto.ppf((np.arange(1, M + 1) - 0.5) / M, k)
    got, sigma = gpd_fit(y[:, None])
    print(f"[psis] genpareto k={k}: fit alone k={got[0]:.4f} sigma={sigma[0]:.4f}")
    assert abs(got[0] - k) <= 0.15 and abs(sigma[0] - 1.0) <= 0.15
    m = 10_000
    assert tail_length(m, 0.02) == M
    rng = np.random.default_rng(3)
    ratios = np.concatenate([rng.uniform(0.2, 1.0, m - M - 1), [1.0], 1.0 + y])
    l = -np.log(rng.permutation(ratios))[:, None] + 7.5
    res = psis_ref(l, r_eff=0.02)
    print(f"[psis] genpareto k={k}: through psis_ref k={res['pareto_k'][0]:.4f}")
    assert abs(res["pareto_k"][0] - k) <= 0.15


def light_tails(m=200, n=9, seed=0):
    """log-likelihoods whose ratios have tails of several weights: Gaussian terms at growing residuals"""
    rng = np.random.default_rng(seed)
    f = 0.3 * rng.standard_normal((m, n))
    y = np.linspace(0.0, 2.5, n)
    return -0.5 * ((y - f) / 0.5) ** 2 - math.log(0.5) - 0.5 * math.log(2 * math.pi)


def test_shift_invariance():
    l = light_tails()
    a = psis_ref(l)
    shift = np.linspace(-300.0, 40.0, l.shape[1])
    b = psis_ref(l + shift)
    assert np.all(np.isfinite(a["pareto_k"])) and a["pareto_k"].max() - a["pareto_k"].min() > 0.2
    # the shifted l_i are rounded at |shift| 2^-53 each: k and p_waic see that through differences of the l_i, of size 1 .. 10 here
    assert np.allclose(b["pareto_k"], a["pareto_k"], rtol=0, atol=1e-9)
    assert np.allclose(b["p_waic"], a["p_waic"], rtol=1e-10, atol=0)
    assert np.allclose(b["elpd_loo"] - shift, a["elpd_loo"], rtol=0, atol=1e-10)
    assert np.allclose(b["lppd"] - shift, a["lppd"], rtol=0, atol=1e-10)


def test_permutation_invariance():
    l = light_tails(seed=1)
    a = psis_ref(l)
    b = psis_ref(l[np.random.default_rng(2).permutation(l.shape[0])])
    for key in a:
        assert np.allclose(a[key], b[key], rtol=1e-11, atol=1e-11), key


def test_constant_row_and_ties():
    l = light_tails(m=64, n=4, seed=4)
    l[:, 1] = -3.25                                         # every network alike: nothing to smooth
    l[1::2, 2] = l[0::2, 2]                                 # pairs of equal values: ties straddle the cutoff (M = 13 is odd)
    res = psis_ref(l)
    assert res["pareto_k"][1] == np.inf and res["elpd_loo"][1] == res["lppd"][1] == -3.25 and res["p_waic"][1] == 0.0
    assert np.all(np.isfinite(res["pareto_k"][[0, 2, 3]]))
    # the multiset decides: the same pairs in another order
    again = psis_ref(l[np.random.default_rng(5).permutation(64)])
    assert np.allclose(again["pareto_k"], res["pareto_k"], rtol=0, atol=1e-11) and np.allclose(again["elpd_loo"], res["elpd_loo"], rtol=1e-12)


def test_undefined_rows_stand_alone():
    l = light_tails(m=64, n=5, seed=6)
    want = psis_ref(l)
    l2 = l.copy()
    l2[7, 1], l2[9, 3] = np.nan, -np.inf
    got = psis_ref(l2)
    for key in want:
        assert np.all(np.isnan(got[key][[1, 3]])), key
        assert np.array_equal(got[key][[0, 2, 4]], want[key][[0, 2, 4]]), key


def test_tail_length_table():
    assert [tail_length(m) for m in (20, 25, 64, 256)] == [4, 5, 13, 48]
    assert tail_length(256, 0.5) == 52
    l = light_tails(m=20, n=3)
    res = psis_ref(l)                                       # M = 4 < 5: the raw ratios
    assert np.all(res["pareto_k"] == np.inf)
    x = -l - (-l).max(axis=0)
    raw = np.log(np.exp(x + l).sum(axis=0)) - np.log(np.exp(x).sum(axis=0))
    assert np.allclose(res["elpd_loo"], raw, rtol=1e-13)
    assert np.all(np.isfinite(psis_ref(light_tails(m=25, n=3))["pareto_k"]))


def test_waic_against_its_definition_and_loo_below_lppd():
    l = light_tails(m=256, n=9, seed=8)
    res = psis_ref(l)
    assert np.allclose(res["p_waic"], l.var(axis=0, ddof=1), rtol=1e-12)
    assert np.allclose(res["lppd"], np.log(np.exp(l).mean(axis=0)), rtol=1e-12)
    assert np.all(res["elpd_loo"] < res["lppd"])            # leaving a row out never helps predicting it


# ------------------------------------------------------------------------------------------------------------------------ the plumbing
def test_library_exports_the_symbol(native):
    lib = C.CDLL(native.LIB_PATH)
    assert hasattr(lib, SYM), f"{SYM} not exported by {native.LIB_PATH}"
    assert native.lib.tbnn_abi_version() == native.ABI_VERSION


def test_native_prototype_matches_the_header(native):
    protos = header_prototypes()
    bound = {name: (res, args) for name, res, args in native.SYMBOLS}
    assert SYM in protos, f"{SYM} not declared in include/tbnn.h"
    assert SYM in bound, f"{SYM} not in _native.SYMBOLS"
    res, args = bound[SYM]
    assert res is C.c_int
    want = [dict(CTYPE, double=C.c_double)[t] for t in protos[SYM]]
    assert len(protos[SYM]) == 16 and len(args) == 16
    for i, (a, w) in enumerate(zip(args, want)):
        assert a is w, (i, protos[SYM][i], a)
    assert re.search(r"#define TBNN_ABI_VERSION %d\b" % native.ABI_VERSION, open(os.path.join(ROOT, "include", "tbnn.h")).read())
    hpp = open(os.path.join(ROOT, "tensorbnn_amd", "csrc", "kernels_ensemble.hpp")).read()
    assert "k_ens_pointwise" in hpp and "k_ens_psis" in hpp


def test_null_handle_is_refused_with_a_message(native):
    z = np.full(4, 0.5, dtype=np.float64)
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    assert native.lib.tbnn_ensemble_loo(None, None, 2, 1, 0, None, 1, None, None, 0, 1.0, dp, dp, dp, dp, None) < 0
    assert "null handle" in native.lib.tbnn_last_error().decode()
    assert np.all(z == 0.5)


class StubChain:
    """records what the predictor asks of Chain.ensemble_loo and answers with rows it can be checked on"""

    def __init__(self):
        self.calls = []

    def ensemble_loo(self, thetas, **kw):
        self.calls.append((np.asarray(thetas), kw))
        rows = np.asarray(kw["X"]).shape[0]
        r = np.arange(rows, dtype=np.float64)
        out = {"elpd_loo": -1.0 - 0.25 * r, "pareto_k": np.where(r % 3 == 0, 0.9, 0.1), "lppd": -0.5 - 0.125 * r, "p_waic": 0.25 + 0.0625 * r}
        out["pareto_k"][-1] = np.inf
        if kw["pointwise"]:
            out["pointwise"] = np.zeros((np.asarray(thetas).shape[0], rows))
        if not kw["psis"]:
            del out["elpd_loo"], out["pareto_k"]
        return out


def stub_predictor(likelihood, hypers=(), m=6, P=5):
    from tensorbnn_amd.predictor import predictor
    p = predictor.__new__(predictor)                     # no saved networks, no device
    p.numNetworks = m
    p.vectors = [np.full(P, i, dtype=np.float32) for i in range(m)]
    p.hypers = list(hypers)
    p.likelihood = likelihood
    p._chain = StubChain()
    return p


X = np.zeros((8, 2), dtype=np.float32)
Y = np.zeros((8, 2), dtype=np.float32)
HYPERS = [np.arange(9, dtype=np.float32) + 10 * i for i in range(6)]          # last hyper of network i: 8 + 10 i


def test_predictor_loo_and_waic_arithmetic():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import BernoulliLikelihood, GaussianLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1), HYPERS)
    res = p.loo(X, Y, n=2, r_eff=0.5)
    th, kw = p._chain.calls[-1]
    assert th.shape == (3, 5) and np.array_equal(th[:, 0], [0, 2, 4])
    assert kw["likelihood"] == nat.LIK_GAUSSIAN and np.array_equal(kw["sd"], np.float32([8, 28, 48])) and kw["r_eff"] == 0.5
    assert kw["pointwise"] is False and kw["psis"] is True and "pointwise" not in res
    rows = -1.0 - 0.25 * np.arange(8)
    assert res["elpd_loo"] == rows.sum() and res["looic"] == -2.0 * rows.sum()
    assert res["se"] == math.sqrt(8 * np.var(rows, ddof=1))
    assert res["p_loo"] == np.sum((-0.5 - 0.125 * np.arange(8)) - rows)
    assert res["k_threshold"] == min(1.0 - 1.0 / math.log10(3), 0.7) and res["k_threshold"] < 0                    # three networks: no k passes
    assert res["n_bad_k"] == 8 and np.array_equal(res["elpd_loo_rows"], rows) and res["pareto_k"][-1] == np.inf
    p = stub_predictor(BernoulliLikelihood(), m=200)
    res = p.loo(X, Y, pointwise=True)
    th, kw = p._chain.calls[-1]
    assert kw["likelihood"] == nat.LIK_BERNOULLI and kw["sd"] is None and kw["r_eff"] == 1.0 and th.shape[0] == 200
    assert res["k_threshold"] == min(1.0 - 1.0 / math.log10(200), 0.7) and 0.5 < res["k_threshold"] < 0.7
    assert res["n_bad_k"] == 4 and res["pointwise"].shape == (200, 8)            # rows 0, 3, 6 at 0.9 and the last at +inf
    w = p.waic(X, Y)
    wrows = (-0.5 - 0.125 * np.arange(8)) - (0.25 + 0.0625 * np.arange(8))
    assert w["elpd_waic"] == wrows.sum() and w["waic"] == -2.0 * wrows.sum() and np.array_equal(w["elpd_waic_rows"], wrows)
    assert w["p_waic"] == np.sum(0.25 + 0.0625 * np.arange(8)) and w["se"] == math.sqrt(8 * np.var(wrows, ddof=1))
    assert "pareto_k" not in w and p._chain.calls[-1][1]["psis"] is False             # WAIC alone does not ask for the smoothing


def test_compare_loo_arithmetic_and_refusals():
    from tensorbnn_amd.predictor import predictor
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(50) - 1.0, rng.standard_normal(50) - 1.5
    res = predictor.compareLoo({"elpd_loo_rows": a}, {"elpd_loo_rows": b})
    assert res["elpd_diff"] == (a - b).sum() and res["se_diff"] == math.sqrt(50 * np.var(a - b, ddof=1))
    same = predictor.compareLoo({"elpd_loo_rows": a}, {"elpd_loo_rows": a.copy()})
    assert same == {"elpd_diff": 0.0, "se_diff": 0.0}
    mixed = predictor.compareLoo({"elpd_waic_rows": a}, {"elpd_loo_rows": b})
    assert mixed["elpd_diff"] == res["elpd_diff"]
    with pytest.raises(ValueError, match="same rows"):
        predictor.compareLoo({"elpd_loo_rows": a}, {"elpd_loo_rows": b[:49]})
    with pytest.raises(ValueError, match="loo or waic"):
        predictor.compareLoo({"elpd_loo": -3.0}, {"elpd_loo_rows": b})
