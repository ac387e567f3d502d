"""The chain diagnostics (tbnn_ensemble_diagnostics / tbnn_series_diagnostics) without a GPU: the fp64 restatement tests/diag_ref.py against
theory on AR(1) chains, the exported symbols and their ctypes prototypes against the header, and the predictor layer over a fake chain --
the chain-major order predictor.fromChains builds from a directory tree in the saved-sample format, thinning per chain, the refusals, the
NaN-ignoring summary and the three small accessors."""
import ctypes as C
import os

import numpy as np
import pytest

from diag_ref import diag_ref
from test_ensemble_host import CTYPE, header_prototypes

NEW = {"tbnn_ensemble_diagnostics": 13, "tbnn_series_diagnostics": 7}


# ------------------------------------------------------------------------------------------------------------- the restatement itself
def ar1(rng, phi, C, S, reps):
    """stationary AR(1) chains of unit marginal variance, [C S, reps] chain-major, rounded to fp32"""
    x = np.empty((C, S, reps))
    x[:, 0] = rng.standard_normal((C, reps))
    e = rng.standard_normal((C, S, reps)) * np.sqrt(1.0 - phi * phi)
    for s in range(1, S):
        x[:, s] = phi * x[:, s - 1] + e[:, s]
    return x.reshape(C * S, reps).astype(np.float32)


@pytest.fixture(scope="module")
def ar1_runs():
    rng = np.random.default_rng(5)
    C, S, reps = 4, 500, 200
    return {phi: (t, diag_ref(t, C)) for phi in (0.0, 0.5, 0.9) for t in [ar1(rng, phi, C, S, reps)]}


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_ess_against_theory(ar1_runs, phi):
    """C = 4, S = 500, 200 repetitions from default_rng(5): the median ESS within 10 % of m (1 - phi) / (1 + phi)"""
    _t, (rhat, ess, margin) = ar1_runs[phi]
    theory = 2000 * (1 - phi) / (1 + phi)
    print(f"[diagnostics] phi={phi}: median ESS {np.median(ess):.1f} (theory {theory:.1f}), max rhat {rhat.max():.4f}, min margin {margin.min():.3e}")
    assert abs(np.median(ess) - theory) <= 0.1 * theory
    assert np.all(np.isfinite(rhat)) and np.all(np.isfinite(ess)) and np.all(margin > 0)


def test_rhat_separates_a_shifted_chain(ar1_runs):
    t, (rhat, _ess, _m) = ar1_runs[0.0]
    assert rhat.max() < 1.05
    shifted = t.copy()
    shifted[:500] += np.float32(3.0)                         # chain 0 moved by 3 standard deviations
    assert diag_ref(shifted, 4)[0].min() > 1.5


def test_odd_draw_count_drops_the_middle_draw():
    rng = np.random.default_rng(1)
    t = rng.standard_normal((3 * 9, 5)).astype(np.float32)
    moved = t.copy()
    moved[[4, 13, 22]] = 1e6                                 # draw 4 of each chain of 9
    a, b = diag_ref(t, 3), diag_ref(moved, 3)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    even = np.delete(t, [4, 13, 22], axis=0)                 # the same chains of 8
    for x, y in zip(a, diag_ref(even, 3)):
        assert np.array_equal(x, y)
    moved[3] = -1e6                                          # draw 3 is used
    assert not np.array_equal(diag_ref(moved, 3)[0], a[0])


def test_constant_and_nan_series_are_undefined():
    rng = np.random.default_rng(2)
    t = rng.standard_normal((32, 4)).astype(np.float32)
    t[:, 1] = 2.5
    t[7, 2] = np.nan
    rhat, ess, margin = diag_ref(t, 2)
    assert np.array_equal(np.isnan(rhat), [False, True, True, False]) and np.array_equal(np.isnan(ess), [False, True, True, False])
    assert np.all(np.isinf(margin[1:3])) and np.all(np.isfinite(margin[[0, 3]]))
    t[:, 1] = np.repeat([1.0, 2.0, 3.0, 4.0], 8)             # every split chain constant, the chains apart: Wv = 0
    assert np.isnan(diag_ref(t, 2)[0][1])
    with pytest.raises(ValueError):
        diag_ref(t[:14], 2)
    with pytest.raises(ValueError):
        diag_ref(t, 3)


def test_hand_computed_element():
    """one chain of 8: the split chains are [1, 2, 4, 3] and [0, 5, 1, 2]"""
    t = np.array([1, 2, 4, 3, 0, 5, 1, 2], dtype=np.float32)[:, None]
    rhat, ess, margin = diag_ref(t, 1)
    d = np.array([[-1.5, -0.5, 1.5, 0.5], [-2.0, 3.0, -1.0, 0.0]])
    A = [np.mean([np.sum(dk[:4 - l] * dk[l:]) / 4 for dk in d]) for l in range(4)]
    Wv = A[0] * 4 / 3
    Vp = Wv * 3 / 4 + np.var([2.5, 2.0], ddof=1)
    assert rhat[0] == pytest.approx(np.sqrt(Vp / Wv), rel=1e-15)
    rho = [1 - (Wv - a) / Vp for a in A]
    P0, P1 = 1 + rho[1], rho[2] + rho[3]
    tau = max(-1 + 2 * (P0 + (min(P0, P1) if P1 > 0 else 0.0)), 1 / np.log10(8))
    assert ess[0] == pytest.approx(8 / tau, rel=1e-15)
    assert margin[0] == pytest.approx(min(abs(P0), abs(P1)), rel=1e-15)


# -------------------------------------------------------------------------------------------------------------------- library, header
def test_library_exports_the_symbols(native):
    lib = C.CDLL(native.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), f"{s} not exported by {native.LIB_PATH}"
    assert native.lib.tbnn_abi_version() == native.ABI_VERSION == 3


def test_native_prototypes_match_the_header(native):
    protos = header_prototypes()
    bound = {name: (res, args) for name, res, args in native.SYMBOLS}
    for s, count in NEW.items():
        assert s in protos, f"{s} not declared in include/tbnn.h"
        assert s in bound, f"{s} not in _native.SYMBOLS"
        res, args = bound[s]
        assert res is C.c_int
        want = [CTYPE[t] for t in protos[s]]
        assert len(protos[s]) == count and len(args) == count
        for i, (a, w) in enumerate(zip(args, want)):
            assert a is w, (s, i, protos[s][i], a)


def test_null_handle_is_refused_with_a_message(native):
    z = np.zeros(4, dtype=np.float64)
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    assert native.lib.tbnn_ensemble_diagnostics(None, None, 8, 1, 1, 0, 1.0, 0.0, 1, None, 0, dp, dp) < 0
    assert "null handle" in native.lib.tbnn_last_error().decode()
    assert native.lib.tbnn_series_diagnostics(None, None, 8, 1, 1, dp, dp) < 0
    assert "null handle" in native.lib.tbnn_last_error().decode()


# -------------------------------------------------------------------------------------------------------------------- predictor layer
class StubChain:
    """records what the predictor asks of Chain.ensemble_diagnostics / series_diagnostics; answers with planted NaNs"""

    def __init__(self, d_out=2):
        self.calls = []
        self.d_out = d_out

    def ensemble_diagnostics(self, thetas, **kw):
        self.calls.append(("ensemble", np.asarray(thetas), kw))
        rows = np.asarray(kw["X"]).shape[0]
        rhat = 1.0 + np.arange(self.d_out * rows, dtype=np.float64).reshape(self.d_out, rows) / 10
        ess = 100.0 - np.arange(self.d_out * rows, dtype=np.float64).reshape(self.d_out, rows)
        rhat[0, 1] = ess[0, 1] = np.nan
        rhat[-1, -1] = ess[-1, -1] = np.nan                  # the largest rhat and the smallest ess would be here
        return rhat, ess

    def series_diagnostics(self, series, **kw):
        self.calls.append(("series", np.asarray(series), kw))
        tot = np.asarray(series).shape[1]
        return np.full(tot, 1.01), np.full(tot, 50.0)


def stub_predictor(likelihood, m=32, P=5, chains=1, hypers=0):
    from tensorbnn_amd.predictor import predictor
    p = predictor.__new__(predictor)                         # no saved networks, no device
    p.numNetworks = m
    p.numChains = chains
    p.vectors = [np.full(P, i, dtype=np.float32) for i in range(m)]
    p.hypers = [np.full(hypers, 1000 + i, dtype=np.float32) for i in range(m)] if hypers else []
    p.likelihood = likelihood
    p._chain = StubChain()
    return p


X = np.zeros((3, 2), dtype=np.float32)


def test_predict_diagnostics_thins_within_each_chain_and_summarises():
    from tensorbnn_amd.likelihood import GaussianLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1), m=40, chains=2)
    out = p.predictDiagnostics(X, n=2, sd=3.0, mean=-1.0)
    kind, th, kw = p._chain.calls[-1]
    assert kind == "ensemble" and kw["chains"] == 2 and kw["scale"] == 3.0 and kw["shift"] == -1.0
    assert np.array_equal(th[:, 0], list(range(0, 20, 2)) + list(range(20, 40, 2)))
    assert set(out) == {"rhat", "ess", "max_rhat", "min_ess", "undefined"}
    assert out["rhat"].shape == out["ess"].shape == (2, 3)
    assert out["undefined"] == 2 and out["max_rhat"] == pytest.approx(1.4) and out["min_ess"] == 96.0
    # n = 3 over chains of 20: draws 0, 3, .., 18 of EACH chain (7 per chain: refused), not every third of the 40
    with pytest.raises(ValueError, match="at least 8"):
        p.predictDiagnostics(X, n=3)
    p = stub_predictor(GaussianLikelihood(sd=0.1), m=50, chains=2)
    p.predictDiagnostics(X, n=3)
    assert np.array_equal(p._chain.calls[-1][1][:, 0], list(range(0, 25, 3)) + list(range(25, 50, 3)))
    p = stub_predictor(GaussianLikelihood(sd=0.1), m=16)     # a plain predictor: one chain
    p.predictDiagnostics(X)
    assert p._chain.calls[-1][2]["chains"] == 1 and np.array_equal(p._chain.calls[-1][1][:, 0], np.arange(16))


def test_predict_diagnostics_transform_and_refusals():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import CategoricalLikelihood, GaussianLikelihood, PoissonLikelihood
    for lik, want in ((CategoricalLikelihood(), nat.XFORM_SOFTMAX), (PoissonLikelihood(), nat.XFORM_EXP), (GaussianLikelihood(sd=0.1), nat.XFORM_NONE)):
        p = stub_predictor(lik)
        p.predictDiagnostics(X)
        assert p._chain.calls[-1][2]["xform"] == want
    p.predictDiagnostics(X, transform="sigmoid")
    assert p._chain.calls[-1][2]["xform"] == nat.XFORM_SIGMOID
    calls = len(p._chain.calls)
    with pytest.raises(ValueError, match="transform"):
        p.predictDiagnostics(X, transform="tanh")
    p.numChains = 5                                          # 32 networks
    with pytest.raises(ValueError, match="divide"):
        p.predictDiagnostics(X)
    with pytest.raises(ValueError, match="divide"):
        p.parameterDiagnostics()
    p.numChains = 8                                          # 4 draws per chain
    with pytest.raises(ValueError, match="at least 8"):
        p.predictDiagnostics(X)
    with pytest.raises(ValueError, match="at least 8"):
        p.parameterDiagnostics()
    assert len(p._chain.calls) == calls                      # refused before any native call


def test_all_undefined_summary_is_nan():
    from tensorbnn_amd.predictor import predictor
    out = predictor._diagnostics(np.full((1, 3), np.nan), np.full((1, 3), np.nan))
    assert out["undefined"] == 3 and np.isnan(out["max_rhat"]) and np.isnan(out["min_ess"])


def test_parameter_diagnostics_covers_parameters_then_hypers():
    from tensorbnn_amd.likelihood import GaussianLikelihood
    p = stub_predictor(GaussianLikelihood(sd=0.1), m=32, P=5, chains=4, hypers=3)
    out = p.parameterDiagnostics()
    kind, series, kw = p._chain.calls[-1]
    assert kind == "series" and kw["chains"] == 4 and series.shape == (32, 8)
    assert np.array_equal(series[:, 0], np.arange(32)) and np.array_equal(series[:, 5], 1000 + np.arange(32))
    assert out["rhat"].shape == (8,) and out["undefined"] == 0 and out["max_rhat"] == 1.01 and out["min_ess"] == 50.0
    p = stub_predictor(GaussianLikelihood(sd=0.1), m=32, P=5)
    p.parameterDiagnostics()
    assert p._chain.calls[-1][1].shape == (32, 5) and p._chain.calls[-1][2]["chains"] == 1


# ------------------------------------------------------------------------------------------- fromChains over a written directory tree
def write_chain(root, c, S, dims=(2, 3, 1), arch=("dense", "relu", "dense"), hypers=2, files=1):
    """folder/chain<c> in the saved-sample format (summary.txt, <matrix>.<file>.txt, hypers<file>.txt, architecture.txt): every entry of
    draw s is 100 c + s (+ 0.5 in the hypers), so a loaded value names its chain and draw"""
    d = os.path.join(root, f"chain{c}")
    os.makedirs(d)
    shapes = []
    for i in range(len(dims) - 1):
        shapes += [(dims[i + 1], dims[i]), (dims[i + 1],)]
    per = S // files
    with open(os.path.join(d, "summary.txt"), "w") as f:
        for sh in shapes:
            f.write(" ".join(str(v) for v in sh) + "\n")
        f.write(f"{S} {files} {len(shapes)}\n{hypers}\n")
    for k in range(files):
        draws = range(k * per, (k + 1) * per)
        for i, sh in enumerate(shapes):
            rows = np.concatenate([np.full((sh[0], sh[1] if len(sh) == 2 else 1), 100.0 * c + s) for s in draws])
            np.savetxt(os.path.join(d, f"{i}.{k}.txt"), rows)
        np.savetxt(os.path.join(d, f"hypers{k}.txt"), np.concatenate([np.full(hypers, 100.0 * c + s + 0.5) for s in draws]))
    with open(os.path.join(d, "architecture.txt"), "w") as f:
        f.write("\n".join(arch) + "\n")
    return d


def test_from_chains_concatenates_chain_major(tmp_path):
    from tensorbnn_amd.predictor import predictor
    root = str(tmp_path / "run")
    for c in range(3):
        write_chain(root, c, 10, files=2)
    p = predictor.fromChains(root)
    assert p.numChains == 3 and p.numNetworks == 30 and len(p.vectors) == 30 and len(p.hypers) == 30
    want = [100.0 * c + s for c in range(3) for s in range(10)]
    assert np.array_equal([v[0] for v in p.vectors], want) and np.array_equal([h[0] for h in p.hypers], np.array(want) + 0.5)
    assert all(v.shape == (2 * 3 + 3 + 3 + 1,) for v in p.vectors)
    assert [m.shape for m in p.matrices] == [(30, 3, 2), (30, 3, 1), (30, 1, 3), (30, 1, 1)]
    assert np.array_equal(p.matrices[2][:, 0, 0], want)
    p._chain = StubChain(d_out=1)
    p.predictDiagnostics(X)
    assert p._chain.calls[-1][2]["chains"] == 3 and np.array_equal(p._chain.calls[-1][1][:, 0], want)
    one = predictor(os.path.join(root, "chain1"))
    assert one.numChains == 1 and one.numNetworks == 10
    # the accessors
    assert np.array_equal(p.extractHyperParameters(), np.array(p.hypers)) and p.extractHyperParameters().shape == (30, 2)
    means, sds = p.parameterStatistics()
    assert len(means) == len(sds) == 4
    for mat, mu, sd in zip(p.extractParameters(), means, sds):
        assert np.array_equal(mu, np.mean(mat, axis=0)) and np.array_equal(sd, np.std(mat, axis=0)) and mu.shape == mat.shape[1:]
    hm, hs = p.hyperStatistics()
    assert np.array_equal(hm, np.mean(np.array(p.hypers), axis=0)) and np.array_equal(hs, np.std(np.array(p.hypers), axis=0))
    assert hm.shape == (2,) and hs[0] > 0


def test_from_chains_refusals(tmp_path):
    from tensorbnn_amd.predictor import predictor
    with pytest.raises(ValueError, match="chain0"):
        predictor.fromChains(str(tmp_path))
    root = str(tmp_path / "a")
    write_chain(root, 0, 10)
    write_chain(root, 1, 9)
    with pytest.raises(ValueError, match="saved networks"):
        predictor.fromChains(root)
    root = str(tmp_path / "b")
    write_chain(root, 0, 10)
    write_chain(root, 1, 10, dims=(2, 4, 1))
    with pytest.raises(ValueError, match="architecture"):
        predictor.fromChains(root)
    root = str(tmp_path / "c")
    write_chain(root, 0, 10)
    write_chain(root, 1, 10, arch=("dense", "tanh", "dense"))
    with pytest.raises(ValueError, match="architecture"):
        predictor.fromChains(root)
    root = str(tmp_path / "d")
    write_chain(root, 0, 10)
    write_chain(root, 2, 10)                                 # chain1 missing: chain0 alone is loaded
    assert predictor.fromChains(root).numChains == 1
