"""NegativeBinomialLikelihood (TBNN_LIK_NEG_BINOMIAL) without a GPU: the oracle's fp64 negative-binomial likelihood against SciPy's
negative-binomial log mass at integer targets and against central differences, the Python class and the predictor's plumbing on a stub
chain, the kernels' likelihood code and the run-time kernel plumbing, the C ABI's admission rules (tbnn_fused_kernel_available runs the
descriptor checks of tbnn_create on the host), and `test_reference_in_fp32_stays_inside_the_bands`: the kernel's own formula in fp32
(the oracle's fp32 arm) against the fp64 definition at every case of tests/test_gpu_negbin.py, inside the project's bands -- value 4e-6
relative, gradient 1e-4 of each tensor's largest entry, log accept ratio 2e-2 + 1e-4 |lar| + 4e-7 |logp|.  Measured, fp32 arm vs fp64 over
the 13 cases: value gaps 1.0e-8 .. 1.2e-7, gradient gaps 1.0e-7 .. 1.0e-6: no case needs a band of its own."""
import ctypes as C
import math

import numpy as np
import pytest

import negbin_ref as nb
import tbnn_oracle as o
from tensor_checks import tensor_errs
from test_predictive_host import HYPERS, StubChain, X as SX, Y as SY, stub_predictor

DIMS_GRID = [c[0] for c in nb.CASES.values()] + [[2, 12, 1], [1, 100, 1], [5, 20, 20, 3], [20, 100, 100, 2], [8, 90, 130, 70, 3], [8, 300, 300, 1]]


def layers_for(dims, hidden_act, last_act=0):
    return [(dims[i], dims[i + 1], hidden_act if i < len(dims) - 2 else last_act, 0) for i in range(len(dims) - 1)]


# ---------------------------------------------------------------------------------------------------------------------- the reference
def test_reference_formula():
    from scipy.stats import nbinom
    rng = np.random.default_rng(1)
    f = 1.5 + 1.2 * rng.standard_normal((3, 50))
    f[0, :4] = [-30.0, 30.0, -700.0, 80.0]                          # far tails: the definition stays finite
    for r in (0.5, 2.5, 30.0, 1e4):
        y = rng.poisson(rng.gamma(r, np.exp(np.clip(f, -5, 8)) / r)).T.astype(np.float64)          # [rows, d_out], integers
        y[0] = 0.0
        got = o.negbin_terms(f, y, r)
        assert got.shape == (3, 50) and got.dtype == np.float64 and np.all(np.isfinite(got))
        # SciPy: nbinom(n = r, p = r / (r + mu)); its p is formed from f here as the stable sigmoid
        p = np.where(f > math.log(r), np.exp(math.log(r) - f) / (1.0 + np.exp(math.log(r) - f)), 1.0 / (1.0 + np.exp(f - math.log(r))))
        want = nbinom.logpmf(y.T, r, p)
        ok = np.isfinite(want) & (np.abs(f) < 25)                    # (SciPy's own log1p(-p) underflows at the far tails)
        assert ok.sum() >= 140
        # rtol 1e-13 and nothing else up to r = 30.  At r = 1e4 SciPy's OWN error is larger than that: its argument p = r / (r + mu) is a
        # double next to 1, so the p it is given differs from the true one by up to half a spacing of p, which moves its log mass by
        # |r / p - y / (1 - p)| times that; and both sides difference lgamma values of 8e4, a few of whose ulps is all either can promise.
        # Those two, computed per element, are allowed there on top
        with np.errstate(divide="ignore", invalid="ignore"):
            atol = 0.0 if r <= 30.0 else (np.abs(r / p - y.T / (1.0 - p)) * np.spacing(p) + 4 * np.spacing(math.lgamma(r + float(y.max()))))[ok]
        err = np.abs(got[ok] - want[ok])
        print(f"[negbin] r {r:g}: fp64 arm against scipy.stats.nbinom.logpmf, worst relative gap {np.max(err / np.abs(want[ok])):.3e}")
        assert np.all(err <= 1e-13 * np.abs(want[ok]) + atol)
    # r -> inf is the Poisson model
    y = rng.poisson(np.exp(f[1:, :])).T.astype(np.float64)
    pois = y.T * f[1:] - np.exp(f[1:]) - np.vectorize(math.lgamma)(y.T + 1.0)
    # (the two log masses differ by ((y - mu)^2 - y) / (2 r) to first order in 1 / r; the lgamma differences at r = 1e7 add ~1e-7)
    mu = np.exp(f[1:])
    assert np.all(np.abs(o.negbin_terms(f[1:], y, 1e7) - pois) <= ((y.T - mu) ** 2 + y.T + 1.0) / 1e7 + 1e-6)
    # the delta is r (y - mu) / (r + mu), bounded by r from below
    _t, d = o.negbin_elementwise(f, np.zeros((50, 3)), 2.5, np.float64)
    assert np.all(d >= -2.5) and d[0, 1] == pytest.approx(-2.5, rel=1e-9)


def test_reference_gradient_against_central_differences():
    spec, X, Y, theta, eta = nb.problem_of([3, 6, 5, 2], 40, o.ACT_TANH, o.PRIOR_CAUCHY, 2.5)
    th = theta.astype(np.float64)
    w = np.random.default_rng(2).integers(0, 3, 40).astype(np.float64)
    for weights in (None, w):
        lp, g = o.target_log_prob_and_grad(spec, th, eta, X, Y, np.float64, weights)
        h = 1e-6
        for j in range(0, spec.n_params, 3):
            e = np.zeros_like(th)
            e[j] = h
            num = (o.target_log_prob_and_grad(spec, th + e, eta, X, Y, np.float64, weights)[0]
                   - o.target_log_prob_and_grad(spec, th - e, eta, X, Y, np.float64, weights)[0]) / (2 * h)
            assert abs(num - g[j]) <= 1e-6 * max(1.0, abs(g[j])), (j, num, g[j])
    # integer weights are duplicated rows, the constant included
    idx = np.repeat(np.arange(40), w.astype(int))
    a = o.target_log_prob_and_grad(spec, th, eta, X, Y, np.float64, w)
    b = o.target_log_prob_and_grad(spec, th, eta, X[idx], Y[idx], np.float64)
    assert math.isclose(a[0], b[0], rel_tol=1e-12) and np.allclose(a[1], b[1], rtol=1e-10, atol=1e-12)


def test_fp32_arm_is_finite_for_every_finite_log_rate():
    """Poisson's overflow past the fp32 range of exp does not occur: the kernel's formula at log-rates far past the
    range of exp (the term is ~ -y |t| or -r t there: finite while that product is)"""
    f = np.array([[-1e30, -1e4, -104.0, -88.0, -20.0, 0.0, 20.0, 88.0, 89.0, 104.0, 1e4, 1e30]], dtype=np.float32)
    y = np.full((f.shape[1], 1), 7.0, dtype=np.float32)
    for r in (0.5, 1e4):
        t, d = o.negbin_elementwise(f, y, r, np.float32)
        assert np.all(np.isfinite(t)) and np.all(np.isfinite(d)) and np.all(t <= 0)
        assert np.all(d <= 7.0) and np.all(d >= -np.float32(r))
    t, d = o.negbin_elementwise(np.array([[np.nan]], dtype=np.float32), y[:1], 2.5, np.float32)
    assert np.isnan(t).all() and np.isnan(d).all()


@pytest.mark.parametrize("name", list(nb.CASES))
def test_reference_in_fp32_stays_inside_the_bands(name):
    """CPU arithmetic only: the kernel's formula in fp32 against the fp64 definition -- value, gradient per tensor, and the log accept ratio
    of the GPU module's injected transition"""
    spec, X, Y, theta, eta = nb.problem(name)
    r = spec.lik_df
    lp64, g64 = nb.ref64(name)
    lp32, g32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)
    gv, gg = abs(lp32 - lp64) / max(abs(lp64), 1.0), tensor_errs(spec, g32, g64, 1e-3)
    f = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    t = f - math.log(r)
    print(f"[negbin] {name}: r {r:g}, counts 0 .. {Y.max():.0f} ({(Y == 0).mean():.2f} zeros), f - log r in [{t.min():.2f}, {t.max():.2f}]; "
          f"fp32 arm: value gap {gv:.3e}, gradient gap {max(gg):.3e}")
    assert Y.min() == 0 and Y.max() > 20 and np.all(Y == np.floor(Y))
    assert gv <= 4e-6 and max(gg) <= 1e-4, (gv, gg)
    p0 = np.random.default_rng(4).standard_normal(spec.n_params).astype(np.float32)
    r64 = o.weight_step(spec, theta, eta, X, Y, nb.step_size(name), 4, p0, -1e30, np.float64)
    r32 = o.weight_step(spec, theta, eta, X, Y, nb.step_size(name), 4, p0, -1e30, np.float32, np.float64)
    tol = 2e-2 + 1e-4 * abs(r64.log_accept_ratio) + 4e-7 * abs(lp64)
    print(f"[negbin] {name}: lar fp32 {r32.log_accept_ratio:.6g} fp64 {r64.log_accept_ratio:.6g} (band {tol:.3g})")
    assert abs(r32.log_accept_ratio - r64.log_accept_ratio) <= tol


def test_cases_are_the_student_cases_with_spread_dispersions():
    import student_ref as sr
    assert list(nb.CASES) == list(sr.CASES)
    for name in nb.CASES:
        assert nb.CASES[name][:6] == sr.CASES[name][:6]
    assert {c[6] for c in nb.CASES.values()} == {0.5, 2.5, 30.0, 1e4}


# ---------------------------------------------------------------------------------------------------------------------- the Python class
def test_python_class_terms_and_shapes():
    import tensorbnn_amd
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import NegativeBinomialLikelihood
    assert tensorbnn_amd.NegativeBinomialLikelihood is NegativeBinomialLikelihood
    lik = NegativeBinomialLikelihood(dispersion=4.0)
    assert nat.LIK_NEG_BINOMIAL == 10 and lik.kind == nat.LIK_NEG_BINOMIAL and lik.dispersion == 4.0
    assert lik.hypers == [] and lik.mainProbsInHypers is False
    assert lik.calcultateLogProb(hypers=[1, 2, 3]) == [0, 0, 0]
    rng = np.random.default_rng(3)
    f = (1.0 + rng.standard_normal((2, 31))).astype(np.float32)            # [d_out, rows], as network.predict returns
    y = rng.poisson(np.exp(f.T)).astype(np.float32)                       # [rows, d_out]
    y[5] += 120.0
    out = lik.makeResponseLikelihood(None, predict=lambda train, _x: f, realVals=y)
    assert out.shape == (2, 31) and out.dtype == np.float64 and np.all(np.isfinite(out))
    np.testing.assert_allclose(out, o.negbin_terms(f.astype(np.float64), y.astype(np.float64), 4.0), rtol=1e-12)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            NegativeBinomialLikelihood(dispersion=bad)
    with pytest.raises(KeyError):
        NegativeBinomialLikelihood()


class NbStubChain(StubChain):
    """tests/test_predictive_host.py's stub with the two calls the negative binomial adds: the dispersion set on the forward chain, and the
    moments of the rate"""

    def __init__(self, d_out=2):
        super().__init__(d_out)
        self.df = []

    def set_lik_df(self, df):
        self.df.append(float(df))

    def ensemble_predictive(self, thetas, probs=None, Y=None, **kw):
        q, F, _Fb = super().ensemble_predictive(thetas, probs=probs, Y=Y, **kw)
        rows = np.asarray(kw["X"]).shape[0]
        return q, F, None if Y is None or kw["likelihood"] not in (5, 10) else np.full((self.d_out, rows), 0.25)

    def ensemble_moments(self, thetas, **kw):
        self.calls.append((np.asarray(thetas), None, None, kw))
        rows = np.asarray(kw["X"]).shape[0]
        return np.full((self.d_out, rows), 6.0), np.full((self.d_out, rows), 2.0)


def test_predictor_host_paths():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import NegativeBinomialLikelihood
    from tensorbnn_amd.predictor import predictor
    rng = np.random.default_rng(5)
    X = rng.standard_normal((20, 2)).astype(np.float32)
    preds = [(1.0 + rng.standard_normal((2, 20))).astype(np.float32) for _ in range(2)]
    Y = rng.poisson(np.exp(preds[0].T)).astype(np.float32)
    p = predictor.__new__(predictor)                     # no saved networks, no device: only the host-side steps
    p.predict = lambda x, n=1: preds
    p.hypers = []
    lik = NegativeBinomialLikelihood(dispersion=3.0)
    got = p._data_logprob(lik, X, Y, 1)
    for g, f in zip(got, preds):
        assert np.isclose(g, o.negbin_terms(f.astype(np.float64), Y.astype(np.float64), 3.0).sum(), rtol=1e-6)
    assert got[0] > got[1]
    # the stub chain: the likelihood code, no sd, the dispersion set on the forward chain before the call, the pair for counts
    p = stub_predictor(lik, HYPERS)
    p._chain = NbStubChain()
    assert p._transform(None) == "exp"
    q = p.predictiveQuantiles(SX, [0.25, 0.75], n=2)
    th, probs, y, kw = p._chain.calls[-1]
    assert q.shape == (2, 2, 3) and y is None and np.array_equal(th[:, 0], [0, 2, 4])
    assert kw["likelihood"] == nat.LIK_NEG_BINOMIAL == 10 and kw["sd"] is None and p._chain.df == [3.0]
    lo, med, hi = p.predictiveInterval(SX)
    assert p._chain.calls[-1][1].tolist() == [0.05, 0.5, 0.95] and np.all(hi == 2.0)
    below, at = p.predictiveCDF(SX, SY)
    assert np.all(below == 0.25) and np.all(at == 0.75) and p._chain.calls[-1][3]["likelihood"] == 10
    assert p.logPredictiveDensity(SX, SY) == ("per_net", "rows")
    assert p._chain.calls[-1][3]["likelihood"] == 10 and p._chain.calls[-1][3]["sd"] is None and p._chain.df[-1] == 3.0
    n_calls = len(p._chain.calls)
    for kw in ({"sd": 2.0}, {"mean": 1.0}):
        with pytest.raises(ValueError, match="NegativeBinomialLikelihood"):
            p.predictiveQuantiles(SX, [0.5], **kw)
    assert len(p._chain.calls) == n_calls
    # countVariance: E[rate] + Var[rate] + E[rate^2] / r on the host, from the device's mean 6 and variance 2
    m, v = p.predictMoments(SX, countVariance=True)
    assert p._chain.calls[-1][3]["xform"] == nat.XFORM_EXP
    assert np.all(m == 6.0) and np.allclose(v, 6.0 + 2.0 + (2.0 + 36.0) / 3.0, rtol=1e-15)
    m, v = p.predictMoments(SX)
    assert np.all(m == 6.0) and np.all(v == 2.0)


# ---------------------------------------------------------------------------------------------------------------------- codes and plumbing
def test_codes_shape_and_cache_key():
    from tensorbnn_amd import _native as nat, jit
    assert jit.LIK_NEGBIN == 8
    assert jit.lik_code(nat.LIK_NEG_BINOMIAL) == 11 and jit.lik_code(nat.LIK_NEG_BINOMIAL, True) == 15
    # every existing code keeps its value
    assert (jit.LIK_GAUSS, jit.LIK_BERN, jit.LIK_CAT, jit.LIK_POIS, jit.LIK_WEIGHTED, jit.LIK_STUDENT) == (0, 1, 2, 3, 4, 8)
    assert [jit.lik_code(k) for k in (nat.LIK_GAUSSIAN, nat.LIK_FIXED_GAUSSIAN, nat.LIK_BERNOULLI, nat.LIK_CATEGORICAL, nat.LIK_POISSON,
                                      nat.LIK_STUDENT_T)] == [0, 0, 1, 2, 3, 8]
    layers = layers_for([30, 80, 80, 10], nat.ACT_RELU)
    g, gw, t, tw = (jit.shape_of(layers, lk, w) for lk, w in ((nat.LIK_POISSON, False), (nat.LIK_POISSON, True),
                                                              (nat.LIK_NEG_BINOMIAL, False), (nat.LIK_NEG_BINOMIAL, True)))
    assert g[:3] == t[:3] == tw[:3] and (g[3], gw[3], t[3], tw[3]) == (3, 7, 11, 15)
    assert len({jit.cache_key(*s) for s in (g, gw, t, tw)}) == 4
    src = jit.source(*t, "mid")
    inner = src.split("Shape<")[1].split(">")[0]
    assert "SHAPE_LIK_POIS | SHAPE_LIK_NEGBIN" in inner and "WEIGHTED" not in inner and src != jit.source(*g, "mid")
    inner = jit.source(*tw, "mid").split("Shape<")[1].split(">")[0]
    assert "SHAPE_LIK_NEGBIN" in inner and "SHAPE_LIK_WEIGHTED" in inner
    assert jit.source(*g, "mid").split("Shape<")[1].split(">")[0].split(", ")[2] == "SHAPE_LIK_POIS"       # the Poisson spelling is untouched


@pytest.mark.parametrize("dims", DIMS_GRID, ids=lambda d: "-".join(map(str, d)))
def test_families_equal_the_poisson_reach(dims):
    from tensorbnn_amd import jit
    want = jit.families(dims, jit.LIK_POIS)
    assert want == jit.families(dims, jit.LIK_GAUSS)
    assert jit.families(dims, jit.LIK_POIS | jit.LIK_NEGBIN) == want
    assert jit.families(dims, jit.LIK_POIS | jit.LIK_NEGBIN | jit.LIK_WEIGHTED) == jit.families(dims, jit.LIK_POIS | jit.LIK_WEIGHTED) == want


def _admission(dims, act_last, lik, fixed_sd=0.1, lik_df=0.0):
    from tensorbnn_amd import _native as nat
    layers = layers_for(dims, nat.ACT_RELU, act_last)
    arr = (nat.LayerDesc * len(layers))(*[nat.LayerDesc(*l) for l in layers])
    desc = nat.NetDesc(len(layers), arr, lik, fixed_sd, nat.KERNEL_AUTO, lik_df)
    rc = nat.lib.tbnn_fused_kernel_available(C.byref(desc))
    return rc, nat.lib.tbnn_last_error().decode()


def test_c_abi_admission(monkeypatch):
    from tensorbnn_amd import _native as nat
    # (the ahead-of-time tables are what is judged: a run-time library that an earlier test of the same process registered does not count)
    monkeypatch.setenv("TBNN_REGISTERED", "0")
    assert C.sizeof(nat.NetDesc) == 32 and nat.NetDesc.lik_df.offset == 28 and nat.lib.tbnn_abi_version() == 3
    for dims in ([5, 8, 1], [5, 8, 3], [5, 8, 40]):                       # any d_out >= 1
        assert _admission(dims, nat.ACT_NONE, nat.LIK_NEG_BINOMIAL, lik_df=4.0)[0] >= 0
        for act in (nat.ACT_TANH, nat.ACT_SIGMOID, nat.ACT_EXP):         # the output is the log of the mean: no last activation
            rc, err = _admission(dims, act, nat.LIK_NEG_BINOMIAL, lik_df=4.0)
            assert rc == -1 and "negative-binomial" in err and "no activation" in err, err
    for df in (0.0, -1.0, float("nan"), float("inf")):
        rc, err = _admission([5, 8, 1], nat.ACT_NONE, nat.LIK_NEG_BINOMIAL, lik_df=df)
        assert rc == -1 and "lik_df" in err, (df, err)
    for sd in (0.0, -0.5, float("nan")):                                  # fixed_sd is not read
        assert _admission([5, 8, 1], nat.ACT_NONE, nat.LIK_NEG_BINOMIAL, fixed_sd=sd, lik_df=4.0)[0] >= 0
    for unknown in (4, 6, 7, -1, 9, 11):
        rc, err = _admission([5, 8, 3], nat.ACT_NONE, unknown, lik_df=4.0)
        assert rc == -1 and "unknown likelihood" in err
    # lik_df stays ignored under the Gaussian kinds and Poisson
    for lik in (nat.LIK_GAUSSIAN, nat.LIK_FIXED_GAUSSIAN, nat.LIK_POISSON):
        assert _admission([5, 8, 1], nat.ACT_NONE, lik, lik_df=float("nan"))[0] >= 0
    # an ahead-of-time Gaussian table is no table for the negative-binomial network of the same layers (the library holds no ahead-of-time
    # Poisson table: test_negbin_library_cross_compiles_checked registers a Poisson library and asks again)
    for dims in ([7, 33, 18, 50, 2], [5, 50, 50, 50, 1]):
        assert _admission(dims, nat.ACT_NONE, nat.LIK_FIXED_GAUSSIAN)[0] > 0
        assert _admission(dims, nat.ACT_NONE, nat.LIK_POISSON)[0] == 0
        assert _admission(dims, nat.ACT_NONE, nat.LIK_NEG_BINOMIAL, lik_df=4.0)[0] == 0


def test_header_and_setter():
    import os
    from tensorbnn_amd import _native as nat
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tbnn.h")).read()
    assert "TBNN_LIK_NEG_BINOMIAL = 10" in hdr and "TBNN_LIK_STUDENT_T = 8" in hdr and "#define TBNN_ABI_VERSION 3" in hdr
    assert nat.ABI_VERSION == 3
    hpp = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tensorbnn_amd", "csrc", "kernels_ensemble.hpp")).read()
    assert "ens_betainc" in hpp and "itmax" in hpp.split("ens_beta_cf")[1][:600]          # the fraction's loop has its bound


@pytest.mark.parametrize("dims,skip,family,name,weighted", [
    ([3, 12, 12, 1], "", "fast3", b"<relu,none,neg-binomial;3,12,12,1>", False),
    ([20, 64, 64, 3], "wide", "mid", b"jit-mid<relu,none,neg-binomial,weighted;20,64,64,3>", True),
])
def test_negbin_library_cross_compiles_checked(tmp_path, monkeypatch, dims, skip, family, name, weighted):
    """jit.build of a narrow and a weighted mid-width negative-binomial shape: hipcc for gfx950 through checked_compile, the MFMA hazard
    check clean, the kernel name carrying neg-binomial"""
    import os
    from tensorbnn_amd import _native as nat, jit
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    monkeypatch.setenv("TBNN_JIT_DIR", str(tmp_path))
    monkeypatch.setenv("TBNN_JIT_SKIP", skip)
    so = jit.build(layers_for(dims, nat.ACT_RELU), nat.LIK_NEG_BINOMIAL, weighted=weighted)
    assert so and os.path.exists(so)
    st = jit.lint_status(so)
    assert st.startswith(family + ":") and "listing checked" in st and "disassembly clean" in st, st
    lib = C.CDLL(so)
    buf = (C.c_char * 4096)()
    assert lib.tbnn_jit_ops(buf) == 0
    assert name in bytes(buf), bytes(buf)[:400]
    if weighted:
        return
    # a Poisson table is no table for the negative-binomial network of the same layers, and the other way round: the Poisson library of
    # the shape registered, then this one
    monkeypatch.delenv("TBNN_REGISTERED", raising=False)
    pso = jit.build(layers_for(dims, nat.ACT_RELU), nat.LIK_POISSON)
    assert pso and pso != so
    before = (_admission(dims, nat.ACT_NONE, nat.LIK_POISSON)[0], _admission(dims, nat.ACT_NONE, nat.LIK_NEG_BINOMIAL, lik_df=2.0)[0])
    assert nat.lib.tbnn_register_kernel_lib(pso.encode()) >= 0, nat.lib.tbnn_last_error().decode()
    assert _admission(dims, nat.ACT_NONE, nat.LIK_POISSON)[0] > 0
    assert _admission(dims, nat.ACT_NONE, nat.LIK_NEG_BINOMIAL, lik_df=2.0)[0] == before[1]
    if before == (0, 0):
        assert nat.lib.tbnn_register_kernel_lib(so.encode()) >= 0, nat.lib.tbnn_last_error().decode()
        assert _admission(dims, nat.ACT_NONE, nat.LIK_NEG_BINOMIAL, lik_df=2.0)[0] > 0
