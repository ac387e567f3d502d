"""Classification uncertainty (tbnn_ensemble_uncertainty, predictor.predictUncertainty / calibration) without a GPU: the built library
exports the entry point, the ctypes prototype agrees with the header argument by argument, the C-ABI version is as before, a null handle
is refused with nothing written, the NumPy restatement (tests/uncertainty_ref.py) meets its closed forms, the calibration helper meets
hand-made tables and the restatement, and the predictor refuses a regression likelihood before any native call."""
import ctypes as C
import math

import numpy as np
import pytest

import uncertainty_ref as ur
from test_ensemble_host import CTYPE, header_prototypes

NAME = "tbnn_ensemble_uncertainty"


def test_symbol_prototype_and_abi(native):
    assert hasattr(C.CDLL(native.LIB_PATH), NAME)
    assert native.lib.tbnn_abi_version() == native.ABI_VERSION == 3
    protos = header_prototypes()
    bound = {name: (res, args) for name, res, args in native.SYMBOLS}
    assert NAME in protos and NAME in bound
    res, args = bound[NAME]
    want = [CTYPE[t] for t in protos[NAME]]
    assert res is C.c_int and len(args) == len(want) == 14
    for i, (a, w) in enumerate(zip(args, want)):
        assert a is w, (i, protos[NAME][i], a)


def test_null_handle_is_refused_and_nothing_is_written(native):
    outs = [np.full(4, -7.0) for _ in range(5)]
    dp = C.POINTER(C.c_double)
    assert native.lib.tbnn_ensemble_uncertainty(None, None, 1, 1, 3, None, 1, None, 0, *[a.ctypes.data_as(dp) for a in outs]) < 0
    assert "null handle" in native.lib.tbnn_last_error().decode()
    assert all(np.all(a == -7.0) for a in outs)


# ------------------------------------------------------------------------------------------------------- the reference's closed forms
def logits_of(p):
    with np.errstate(divide="ignore"):
        return np.maximum(np.log(np.asarray(p, dtype=np.float64)), -200.0).astype(np.float32)


def test_reference_two_certain_networks_that_disagree():
    """p = (1, 0) and (0, 1): all of the uncertainty is disagreement"""
    f = np.array([[[80.0], [-80.0]], [[-80.0], [80.0]]], dtype=np.float32)               # [m = 2, K = 2, n = 1]
    r = ur.uncertainty(f, None, "categorical")
    assert r["total"][0] == pytest.approx(math.log(2), abs=1e-15) and r["aleatoric"][0] == pytest.approx(0.0, abs=1e-30)
    assert r["epistemic"][0] == pytest.approx(math.log(2), abs=1e-15)
    assert np.array_equal(r["votes"][:, 0], [0.5, 0.5]) and np.allclose(r["probs"][:, 0], [0.5, 0.5], atol=1e-30)
    assert ur.variation_ratio(r["votes"], "categorical")[0] == 0.5
    # Bernoulli: p at the two ends of the clip
    b = ur.uncertainty(np.array([[[1.0]], [[0.0]]], dtype=np.float32), None, "bernoulli")
    assert b["total"][0, 0] == pytest.approx(math.log(2), abs=1e-7) and b["aleatoric"][0, 0] < 2e-6 and b["votes"][0, 0] == 0.5
    assert ur.variation_ratio(b["votes"], "bernoulli")[0, 0] == 0.5


def test_reference_identical_networks_have_no_epistemic_part():
    rng = np.random.default_rng(0)
    one = rng.standard_normal((1, 5, 40)).astype(np.float32) * 3
    f = np.repeat(one, 6, axis=0)
    for w in (None, rng.random(6).astype(np.float32)):
        r = ur.uncertainty(f, w, "categorical")
        assert np.all(r["epistemic"] <= 8 * 2.0 ** -53) and np.allclose(r["total"], r["aleatoric"], rtol=0, atol=1e-15)
        assert np.all((r["votes"] == 0) | (np.abs(r["votes"] - 1) <= 2.0 ** -52))
        assert np.allclose(r["total"], ur.uncertainty(one, None, "categorical")["total"], rtol=0, atol=1e-15)
    s = 1.0 / (1.0 + np.exp(-one[:, :2]))
    r = ur.uncertainty(np.repeat(s.astype(np.float32), 4, axis=0), None, "bernoulli")
    assert np.all(r["epistemic"] <= 8 * 2.0 ** -53) and r["total"].shape == (2, 40)


@pytest.mark.parametrize("K", [2, 3, 10, 19])
def test_reference_uniform_logits(K):
    f = np.full((4, K, 3), 1.25, dtype=np.float32)
    r = ur.uncertainty(f, None, "categorical")
    assert np.allclose(r["total"], math.log(K), rtol=0, atol=4e-16 * K) and np.allclose(r["aleatoric"], math.log(K), rtol=0, atol=4e-16 * K)
    assert np.all(r["epistemic"] <= 1e-15)
    assert np.array_equal(r["votes"][0], np.ones(3)) and not r["votes"][1:].any()          # ties: the lowest class


def test_reference_nan_rule_and_zero_probabilities():
    f = np.zeros((3, 4, 5), dtype=np.float32)
    f[0, :, 1] = [200.0, -200.0, 0.0, -200.0]                   # exact zeros among the fp64 probabilities: 0 log 0 = 0
    f[2, 1, 3] = np.nan
    w = np.array([1.0, 1.0, 0.0], dtype=np.float32)             # the NaN network has weight 0: the row is NaN all the same
    r = ur.uncertainty(f, w, "categorical")
    for k in ("probs", "votes"):
        assert np.all(np.isnan(r[k][:, 3])) and np.all(np.isfinite(np.delete(r[k], 3, axis=1)))
    for k in ("total", "aleatoric", "epistemic"):
        assert np.isnan(r[k][3]) and np.all(np.isfinite(np.delete(r[k], 3)))
    b = ur.uncertainty(f[:, :2], w, "bernoulli")
    assert np.isnan(b["total"][1, 3]) and np.isfinite(b["total"][0, 3]) and np.isnan(b["votes"][1, 3])


# ---------------------------------------------------------------------------------------------------------- the calibration helper
def table(probs, Y, bins, kind):
    from tensorbnn_amd.predictor import predictor
    return predictor._calibration_table(probs, Y, bins, kind)


def same_table(a, b):
    for k in ("accuracy", "nll", "brier", "ece", "mce"):
        assert a[k] == pytest.approx(b[k], rel=1e-13, abs=1e-15), k
    for k in ("edges", "count", "confidence", "accuracy"):
        assert np.allclose(a["bins"][k], b["bins"][k], rtol=1e-13, atol=0, equal_nan=True), k
    for k in ("predicted", "confidence", "correct"):
        assert np.array_equal(a[k], b[k]), k


def test_calibration_perfectly_calibrated_table():
    """4 rows at confidence 0.75 of which 3 are right, 5 at 0.6 of which 3: every bin's accuracy is its confidence"""
    conf = np.array([0.75] * 4 + [0.6] * 5)
    right = np.array([1, 1, 1, 0] + [1, 1, 1, 0, 0], dtype=bool)
    probs = np.stack([conf, 1.0 - conf])                              # class 0 is predicted everywhere
    labels = np.where(right, 0, 1)
    t = table(probs, labels, 10, "categorical")
    assert t["ece"] == pytest.approx(0.0, abs=1e-16) and t["mce"] == pytest.approx(0.0, abs=1e-16)
    assert t["accuracy"] == pytest.approx(6 / 9) and np.array_equal(t["predicted"], np.zeros(9, dtype=int))
    assert np.array_equal(t["bins"]["count"], [0, 0, 0, 0, 0, 5, 0, 4, 0, 0])              # (0.5, 0.6] and (0.7, 0.8]
    assert np.all(np.isnan(t["bins"]["confidence"][t["bins"]["count"] == 0])) and np.all(np.isnan(t["bins"]["accuracy"][t["bins"]["count"] == 0]))
    assert t["nll"] == pytest.approx(-np.mean(np.log(np.where(right, conf, 1 - conf))))
    assert t["brier"] == pytest.approx(np.mean(2 * np.where(right, 1 - conf, conf) ** 2))
    same_table(t, ur.calibration(probs, labels, 10, "categorical"))


def test_calibration_all_wrong_at_confidence_one():
    probs = np.array([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
    t = table(probs, np.array([1, 1, 1]), 10, "categorical")
    assert t["ece"] == 1.0 and t["mce"] == 1.0 and t["accuracy"] == 0.0 and t["nll"] == np.inf and t["brier"] == 2.0
    assert t["bins"]["count"][-1] == 3 and t["bins"]["count"].sum() == 3
    b = table(np.array([[1.0, 1.0, 0.0]]), np.array([0.0, 0.0, 1.0]), 4, "bernoulli")
    assert b["accuracy"] == 0.0 and b["ece"] == pytest.approx(1.0, abs=2e-7) and b["mce"] == pytest.approx(1.0, abs=2e-7)
    assert np.array_equal(b["predicted"], [[1, 1, 0]]) and np.isfinite(b["nll"]) and b["nll"] > 15.0      # (the clip keeps it finite)


def test_calibration_labels_bins_and_ties():
    rng = np.random.default_rng(3)
    z = rng.standard_normal((5, 200)) * 2
    probs = np.exp(z) / np.exp(z).sum(axis=0)
    probs[:, 7] = [0.3, 0.3, 0.2, 0.1, 0.1]                           # a tie: the lowest class
    labels = rng.integers(0, 5, 200)
    onehot = np.eye(5)[labels]
    soft = 0.6 * onehot + 0.08                                        # probability rows: the first arg-max is the label
    for bins in (1, 3, 10, 1000):
        a = table(probs, labels, bins, "categorical")
        same_table(a, table(probs, onehot, bins, "categorical"))
        same_table(a, table(probs, soft, bins, "categorical"))
        same_table(a, ur.calibration(probs, labels, bins, "categorical"))
        assert a["bins"]["count"].sum() == 200 and a["bins"]["edges"].shape == (bins + 1,)
        assert a["ece"] <= a["mce"] + 1e-15
    assert table(probs, labels, 10, "categorical")["predicted"][7] == 0
    # the edges: right-closed, 0 in the first bin
    c = np.array([[0.5, 0.75, 1.0, 0.5000001]])
    t = table(np.concatenate([c, 1 - c]), np.zeros(4, dtype=int), 4, "categorical")
    assert np.array_equal(t["bins"]["count"], [0, 1, 2, 1])
    z0 = table(np.array([[0.0, 0.25]]), np.array([1.0, 1.0]), 4, "bernoulli")              # confidence max(p, 1 - p) = 1, 0.75
    assert np.array_equal(z0["bins"]["count"], [0, 0, 1, 1])
    # Bernoulli: [rows, d_out], [rows] for one output, thresholds at 1/2
    pb = rng.random((2, 50))
    Yb = (rng.random((50, 2)) < 0.5).astype(np.float32)
    same_table(table(pb, Yb, 6, "bernoulli"), ur.calibration(pb, Yb, 6, "bernoulli"))
    same_table(table(pb, Yb, 6, "bernoulli"), table(pb, 0.2 + 0.6 * Yb, 6, "bernoulli"))
    same_table(table(pb[:1], Yb[:, 0], 6, "bernoulli"), table(pb[:1], Yb[:, :1], 6, "bernoulli"))
    for bad in (0, 1001, -3, 2.5, "10", None, True):
        with pytest.raises(ValueError, match="bins"):
            table(probs, labels, bad, "categorical")
    with pytest.raises(ValueError, match="0 .. 4"):
        table(probs, np.full(200, 5), 10, "categorical")
    with pytest.raises(ValueError):
        table(probs, labels[:-1], 10, "categorical")
    with pytest.raises(ValueError, match="kind"):
        table(probs, labels, 10, "gaussian")


# -------------------------------------------------------------------------------------------------------------------- the predictor
class StubChain:
    def __init__(self):
        self.calls = []

    def ensemble_uncertainty(self, thetas, **kw):
        self.calls.append((np.asarray(thetas), kw))
        K, n = 3, np.asarray(kw["X"]).shape[0]
        votes = np.tile(np.array([[0.5], [0.25], [0.25]]), (1, n))
        return {"probs": np.tile(np.array([[0.6], [0.3], [0.1]]), (1, n)), "votes": votes, "total": np.ones(n), "aleatoric": np.ones(n) / 2,
                "epistemic": np.ones(n) / 2}


def stub_predictor(likelihood, m=6, P=5):
    from tensorbnn_amd.predictor import predictor
    p = predictor.__new__(predictor)                     # no saved networks, no device
    p.numNetworks = m
    p.vectors = [np.full(P, i, dtype=np.float32) for i in range(m)]
    p.hypers = []
    p.likelihood = likelihood
    p._chain = StubChain()
    return p


def test_predictor_passes_through_and_refuses_regression():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import (BernoulliLikelihood, CategoricalLikelihood, FixedGaussianLikelihood, GaussianLikelihood,
                                          PoissonLikelihood)
    X = np.zeros((4, 2), dtype=np.float32)
    p = stub_predictor(CategoricalLikelihood())
    out = p.predictUncertainty(X, n=2, weights=[0.5, 0.25, 0.25])
    th, kw = p._chain.calls[-1]
    assert np.array_equal(th[:, 0], [0, 2, 4]) and kw["likelihood"] == nat.LIK_CATEGORICAL
    assert np.array_equal(kw["weights"], np.float32([0.5, 0.25, 0.25]))
    assert np.array_equal(out["variation_ratio"], np.full(4, 0.5)) and set(out) == {"probs", "votes", "total", "aleatoric", "epistemic", "variation_ratio"}
    p.predictUncertainty(X, likelihood=BernoulliLikelihood())
    assert p._chain.calls[-1][1]["likelihood"] == nat.LIK_BERNOULLI
    cal = p.calibration(X, np.array([0, 0, 1, 2]), bins=5)
    assert cal["accuracy"] == 0.5 and cal["ece"] == pytest.approx(0.1) and cal["bins"]["count"][2] == 4
    for lik in (GaussianLikelihood(sd=0.1), FixedGaussianLikelihood(sd=0.3), PoissonLikelihood()):
        q = stub_predictor(lik)
        for call in (lambda: q.predictUncertainty(X), lambda: q.calibration(X, np.zeros(4, dtype=int)),
                     lambda: p.predictUncertainty(X, likelihood=lik)):
            n_before = len(p._chain.calls)
            with pytest.raises(ValueError, match=r"predictMoments\(noiseVariance=True\).*predictiveInterval"):
                call()
            assert not q._chain.calls and len(p._chain.calls) == n_before                  # refused before any native call
    with pytest.raises(ValueError, match="bins"):
        p.calibration(X, np.zeros(4, dtype=int), bins=0)
    with pytest.raises(ValueError, match="one value per picked network"):
        p.predictUncertainty(X, n=2, weights=[1.0, 1.0])
