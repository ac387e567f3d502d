"""GammaLikelihood (TBNN_LIK_GAMMA) without a GPU: the fp64 arm of tests/gamma_ref.py against SciPy's Gamma log density and against
central differences, the Python class and the predictor's plumbing on a stub chain, the kernels' likelihood code and the run-time kernel
plumbing, the C ABI's admission rules (tbnn_fused_kernel_available runs the descriptor checks of tbnn_create on the host), a NumPy port of
the device's incomplete gamma function (csrc/kernels_ensemble.hpp ens_gamma_q / ens_gamma_p) against SciPy at non-integer shapes, and
`test_reference_in_fp32_stays_inside_the_bands`: the kernel's own formula in fp32 against the fp64 definition at every case of
tests/test_gpu_gamma.py, inside the project's bands -- value 4e-6 relative, gradient 1e-4 of each tensor's largest entry, log accept
ratio 2e-2 + 1e-4 |lar| + 4e-7 |logp|.  Measured, fp32 arm vs fp64 over the 13 cases: value gaps 1.6e-9 .. 1.9e-6 (mid10, a = 0.5),
gradient gaps 1.2e-7 .. 2.9e-6: no case needs a band of its own."""
import ctypes as C
import math

import numpy as np
import pytest

import gamma_ref as gr
import tbnn_oracle as o
from tensor_checks import tensor_errs
from test_predictive_host import HYPERS, StubChain, X as SX, Y as SY, stub_predictor

DIMS_GRID = [c[0] for c in gr.CASES.values()] + [[2, 12, 1], [1, 100, 1], [5, 20, 20, 3], [20, 100, 100, 2], [8, 90, 130, 70, 3], [8, 300, 300, 1]]


def layers_for(dims, hidden_act, last_act=0):
    return [(dims[i], dims[i + 1], hidden_act if i < len(dims) - 2 else last_act, 0) for i in range(len(dims) - 1)]


# ---------------------------------------------------------------------------------------------------------------------- the reference
def test_reference_formula():
    from scipy.stats import gamma
    rng = np.random.default_rng(1)
    f = 0.5 + 0.8 * rng.standard_normal((3, 50))
    f[0, :4] = [-30.0, 30.0, -200.0, 80.0]                          # far tails: the definition stays finite
    for a in (0.5, 1.0, 2.0, 10.0, 200.0):
        y = np.maximum(rng.gamma(a, np.exp(np.clip(f, -5, 8)) / a), 1e-300).T          # [rows, d_out]
        got = gr.terms(f, y, a)
        assert got.shape == (3, 50) and got.dtype == np.float64 and np.all(np.isfinite(got))
        want = gamma(a, scale=np.exp(f) / a).logpdf(y.T)
        ok = np.isfinite(want)
        assert ok.sum() >= 146
        # both sides sum the same five terms in fp64: a few ulps of the largest of them (a log a and lgamma(a) cancel at a = 200)
        mag = abs(a * math.log(a)) + abs(math.lgamma(a)) + np.abs((a - 1.0) * np.log(y.T)) + np.abs(a * f) + a * y.T * np.exp(-f)
        err = np.abs(got[ok] - want[ok])
        print(f"[gamma] a {a:g}: fp64 arm against scipy.stats.gamma.logpdf, worst gap {np.max(err / mag[ok]):.3e} of the terms' magnitudes")
        assert np.all(err <= 1e-14 * mag[ok])
    # a = 1 is the exponential distribution of mean mu
    y = rng.exponential(np.exp(f[1:])).T
    assert np.allclose(gr.terms(f[1:], y, 1.0), -f[1:] - y.T * np.exp(-f[1:]), rtol=1e-14, atol=1e-14)
    # the delta is a (y / mu - 1), bounded by -a from below
    _t, d = gr.elementwise(f, np.zeros((50, 3)), 2.5, np.float64)
    assert np.all(d == -2.5)
    _t, d = gr.elementwise(f, np.exp(f).T, 2.5, np.float64)
    assert np.all(np.abs(d) <= 1e-14)


def test_reference_gradient_against_central_differences():
    spec, X, Y, theta, eta = gr.problem_of([3, 6, 5, 2], 40, o.ACT_TANH, o.PRIOR_CAUCHY, 2.0)
    th = theta.astype(np.float64)
    w = np.random.default_rng(2).integers(0, 3, 40).astype(np.float64)
    for weights in (None, w):
        lp, g = gr.target_log_prob_and_grad(spec, 2.0, th, eta, X, Y, np.float64, weights)
        h = 1e-6
        for j in range(0, spec.n_params, 3):
            e = np.zeros_like(th)
            e[j] = h
            num = (gr.target_log_prob_and_grad(spec, 2.0, th + e, eta, X, Y, np.float64, weights)[0]
                   - gr.target_log_prob_and_grad(spec, 2.0, th - e, eta, X, Y, np.float64, weights)[0]) / (2 * h)
            assert abs(num - g[j]) <= 1e-6 * max(1.0, abs(g[j])), (j, num, g[j])
    # integer weights are duplicated rows, the constant included
    idx = np.repeat(np.arange(40), w.astype(int))
    a_ = gr.target_log_prob_and_grad(spec, 2.0, th, eta, X, Y, np.float64, w)
    b_ = gr.target_log_prob_and_grad(spec, 2.0, th, eta, X[idx], Y[idx], np.float64)
    assert math.isclose(a_[0], b_[0], rel_tol=1e-12) and np.allclose(a_[1], b_[1], rtol=1e-10, atol=1e-12)
    # the likelihood-only objective is the data term
    lv, lg = gr.likelihood_value_and_grad(spec, 2.0, th, eta, X, Y, np.float64)
    f = o.forward(spec, th, X.astype(np.float64), np.float64)
    assert math.isclose(lv, gr.terms(f, Y, 2.0).sum(), rel_tol=1e-10)


def test_fp32_arm_overflows_only_below_the_range_of_exp():
    """Poisson's rule on the other side: a log-mean below the fp32 range of exp(-f) gives a non-finite term (the proposal is rejected);
    every other finite log-mean gives a finite one"""
    f = np.array([[-1e4, -104.0, -89.0, -80.0, -20.0, 0.0, 20.0, 88.0, 104.0, 1e4]], dtype=np.float32)
    y = np.full((f.shape[1], 1), 7.0, dtype=np.float32)
    t, d = gr.elementwise(f, y, 2.0, np.float32)
    assert not np.isfinite(t[0, :3]).any() and np.all(np.isfinite(t[0, 3:])) and np.all(np.isfinite(d[0, 3:]))
    assert np.all(d[0, 7:] == -2.0)
    t, d = gr.elementwise(np.array([[np.nan]], dtype=np.float32), y[:1], 2.0, np.float32)
    assert np.isnan(t).all() and np.isnan(d).all()


@pytest.mark.parametrize("name", list(gr.CASES))
def test_reference_in_fp32_stays_inside_the_bands(name):
    """CPU arithmetic only: the kernel's formula in fp32 against the fp64 definition -- value, gradient per tensor, and the log accept ratio
    of the GPU module's injected transition"""
    spec, X, Y, theta, eta, a = gr.problem(name)
    lp64, g64 = gr.ref64(name)
    lp32, g32 = gr.target_log_prob_and_grad(spec, a, theta, eta, X, Y, np.float32)
    gv, gg = abs(lp32 - lp64) / max(abs(lp64), 1.0), tensor_errs(spec, g32, g64, 1e-3)
    f = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    print(f"[gamma] {name}: a {a:g}, targets {Y.min():.3g} .. {Y.max():.3g}, f in [{f.min():.2f}, {f.max():.2f}]; "
          f"fp32 arm: value gap {gv:.3e}, gradient gap {max(gg):.3e}")
    assert Y.min() > 0 and np.all(np.isfinite(Y))
    assert gv <= 4e-6 and max(gg) <= 1e-4, (gv, gg)
    p0 = np.random.default_rng(4).standard_normal(spec.n_params).astype(np.float32)
    r64 = gr.weight_step(spec, a, theta, eta, X, Y, gr.step_size(name), 4, p0, -1e30, np.float64)
    r32 = gr.weight_step(spec, a, theta, eta, X, Y, gr.step_size(name), 4, p0, -1e30, np.float32)
    tol = 2e-2 + 1e-4 * abs(r64.log_accept_ratio) + 4e-7 * abs(lp64)
    print(f"[gamma] {name}: lar fp32 {r32.log_accept_ratio:.6g} fp64 {r64.log_accept_ratio:.6g} (band {tol:.3g})")
    assert abs(r32.log_accept_ratio - r64.log_accept_ratio) <= tol


def test_cases_are_the_student_cases_with_spread_shapes():
    import student_ref as sr
    assert list(gr.CASES) == list(sr.CASES)
    for name in gr.CASES:
        assert gr.CASES[name][:6] == sr.CASES[name][:6]
    assert {c[6] for c in gr.CASES.values()} == {0.5, 2.0, 10.0, 200.0}


# ---------------------------------------------------------------------------------------------------------------------- the Python class
def test_python_class_terms_and_shapes():
    import tensorbnn_amd
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import GammaLikelihood
    assert tensorbnn_amd.GammaLikelihood is GammaLikelihood
    lik = GammaLikelihood(shape=4.0)
    assert nat.LIK_GAMMA == 14 and lik.kind == nat.LIK_GAMMA and lik.shape == 4.0
    assert lik.hypers == [] and lik.mainProbsInHypers is False
    assert lik.calcultateLogProb(hypers=[1, 2, 3]) == [0, 0, 0]
    rng = np.random.default_rng(3)
    f = (1.0 + rng.standard_normal((2, 31))).astype(np.float32)            # [d_out, rows], as network.predict returns
    y = rng.gamma(4.0, np.exp(f.T) / 4.0).astype(np.float32)               # [rows, d_out]
    out = lik.makeResponseLikelihood(None, predict=lambda train, _x: f, realVals=y)
    assert out.shape == (2, 31) and out.dtype == np.float64 and np.all(np.isfinite(out))
    np.testing.assert_allclose(out, gr.terms(f.astype(np.float64), y.astype(np.float64), 4.0), rtol=1e-12)
    np.testing.assert_allclose(lik.logDensity(f, y.T), out, rtol=0, atol=0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            GammaLikelihood(shape=bad)
    with pytest.raises(KeyError):
        GammaLikelihood()


class GammaStubChain(StubChain):
    """tests/test_predictive_host.py's stub with the two calls the Gamma likelihood adds: the shape set on the forward chain, and the
    moments of the mean"""

    def __init__(self, d_out=2):
        super().__init__(d_out)
        self.df = []

    def set_lik_df(self, df):
        self.df.append(float(df))

    def ensemble_moments(self, thetas, **kw):
        self.calls.append((np.asarray(thetas), None, None, kw))
        rows = np.asarray(kw["X"]).shape[0]
        return np.full((self.d_out, rows), 6.0), np.full((self.d_out, rows), 2.0)

    def ensemble_crps(self, *a, **kw):
        raise AssertionError("the CRPS must be refused on the host")

    def ensemble_uncertainty(self, *a, **kw):
        raise AssertionError("the entropy split must be refused on the host")


def test_predictor_host_paths():
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import GammaLikelihood, PoissonLikelihood, StudentTLikelihood
    from tensorbnn_amd.predictor import predictor
    rng = np.random.default_rng(5)
    X = rng.standard_normal((20, 2)).astype(np.float32)
    preds = [(1.0 + rng.standard_normal((2, 20))).astype(np.float32) for _ in range(2)]
    Y = rng.gamma(3.0, np.exp(preds[0].T) / 3.0).astype(np.float32)
    p = predictor.__new__(predictor)                     # no saved networks, no device: only the host-side steps
    p.predict = lambda x, n=1: preds
    p.hypers = []
    lik = GammaLikelihood(shape=3.0)
    got = p._data_logprob(lik, X, Y, 1)
    for g, f in zip(got, preds):
        assert np.isclose(g, gr.terms(f.astype(np.float64), Y.astype(np.float64), 3.0).sum(), rtol=1e-6)
    assert got[0] > got[1]
    # the stub chain: the likelihood code, no sd, the shape set on the forward chain before the call, F alone (a continuous CDF)
    p = stub_predictor(lik, HYPERS)
    p._chain = GammaStubChain()
    assert p._transform(None) == "exp"
    q = p.predictiveQuantiles(SX, [0.25, 0.75], n=2)
    th, probs, y, kw = p._chain.calls[-1]
    assert q.shape == (2, 2, 3) and y is None and np.array_equal(th[:, 0], [0, 2, 4])
    assert kw["likelihood"] == nat.LIK_GAMMA == 14 and kw["sd"] is None and p._chain.df == [3.0]
    lo, med, hi = p.predictiveInterval(SX)
    assert p._chain.calls[-1][1].tolist() == [0.05, 0.5, 0.95] and np.all(hi == 2.0)
    F = p.predictiveCDF(SX, SY)
    assert isinstance(F, np.ndarray) and np.all(F == 0.75) and p._chain.calls[-1][3]["likelihood"] == 14
    assert p.logPredictiveDensity(SX, SY) == ("per_net", "rows")
    assert p._chain.calls[-1][3]["likelihood"] == 14 and p._chain.calls[-1][3]["sd"] is None and p._chain.df[-1] == 3.0
    n_calls = len(p._chain.calls)
    for kw in ({"sd": 2.0}, {"mean": 1.0}):
        with pytest.raises(ValueError, match="GammaLikelihood"):
            p.predictiveQuantiles(SX, [0.5], **kw)
    with pytest.raises(ValueError, match="not built for a GammaLikelihood"):
        p.crps(SX, SY)
    with pytest.raises(ValueError, match="GammaLikelihood's positive target"):
        p.predictUncertainty(SX)
    assert len(p._chain.calls) == n_calls
    # noiseVariance: Var[mu] + E[mu^2] / a on the host, from the device's mean 6 and variance 2
    m, v = p.predictMoments(SX, noiseVariance=True)
    assert p._chain.calls[-1][3]["xform"] == nat.XFORM_EXP
    assert np.all(m == 6.0) and np.allclose(v, 2.0 + (2.0 + 36.0) / 3.0, rtol=1e-15)
    m, v = p.predictMoments(SX)
    assert np.all(m == 6.0) and np.all(v == 2.0) and p._chain.calls[-1][3]["xform"] == nat.XFORM_EXP
    for kw in ({"sd": 2.0}, {"mean": 1.0}, {"transform": "none"}, {"countVariance": True}):
        with pytest.raises(ValueError, match="GammaLikelihood"):
            p.predictMoments(SX, noiseVariance=True, **kw)
    # every other existing likelihood without a predicted noise keeps raising there
    for other in (PoissonLikelihood(), StudentTLikelihood(sd=0.5, df=4.0)):
        q_ = stub_predictor(other, HYPERS)
        q_._chain = GammaStubChain()
        with pytest.raises(ValueError, match="HeteroscedasticGaussianLikelihood"):
            q_.predictMoments(SX, noiseVariance=True)


# ---------------------------------------------------------------------------------------------------------------------- codes and plumbing
def test_codes_shape_and_cache_key():
    from tensorbnn_amd import _native as nat, jit
    assert jit.LIK_GAMMA == 16
    assert jit.lik_code(nat.LIK_GAMMA) == 19 and jit.lik_code(nat.LIK_GAMMA, True) == 23
    # every existing code keeps its value
    assert (jit.LIK_GAUSS, jit.LIK_BERN, jit.LIK_CAT, jit.LIK_POIS, jit.LIK_WEIGHTED, jit.LIK_STUDENT, jit.LIK_NEGBIN, jit.LIK_HETERO) == (0, 1, 2, 3, 4, 8, 8, 16)
    assert [jit.lik_code(k) for k in (nat.LIK_GAUSSIAN, nat.LIK_FIXED_GAUSSIAN, nat.LIK_BERNOULLI, nat.LIK_CATEGORICAL, nat.LIK_POISSON,
                                      nat.LIK_STUDENT_T, nat.LIK_NEG_BINOMIAL, nat.LIK_HETERO_GAUSSIAN)] == [0, 0, 1, 2, 3, 8, 11, 16]
    assert (nat.LIK_GAUSSIAN, nat.LIK_FIXED_GAUSSIAN, nat.LIK_BERNOULLI, nat.LIK_CATEGORICAL, nat.LIK_POISSON, nat.LIK_STUDENT_T,
            nat.LIK_NEG_BINOMIAL, nat.LIK_HETERO_GAUSSIAN, nat.LIK_GAMMA) == (0, 1, 2, 3, 5, 8, 10, 12, 14)
    layers = layers_for([30, 80, 80, 10], nat.ACT_RELU)
    g, gw, t, tw = (jit.shape_of(layers, lk, w) for lk, w in ((nat.LIK_POISSON, False), (nat.LIK_POISSON, True),
                                                              (nat.LIK_GAMMA, False), (nat.LIK_GAMMA, True)))
    assert g[:3] == t[:3] == tw[:3] and (g[3], gw[3], t[3], tw[3]) == (3, 7, 19, 23)
    assert len({jit.cache_key(*s) for s in (g, gw, t, tw)}) == 4
    src = jit.source(*t, "mid")
    inner = src.split("Shape<")[1].split(">")[0]
    assert "SHAPE_LIK_POIS | SHAPE_LIK_GAMMA" in inner and "WEIGHTED" not in inner and src != jit.source(*g, "mid")
    inner = jit.source(*tw, "mid").split("Shape<")[1].split(">")[0]
    assert "SHAPE_LIK_GAMMA" in inner and "SHAPE_LIK_WEIGHTED" in inner
    assert jit.source(*g, "mid").split("Shape<")[1].split(">")[0].split(", ")[2] == "SHAPE_LIK_POIS"       # the Poisson spelling is untouched
    # a heteroscedastic code still needs its two outputs; the Gamma code, the same bit on the Poisson code, does not
    assert jit.families([5, 20, 20, 3], jit.LIK_HETERO) == [] and jit.families([5, 20, 20, 3], jit.LIK_POIS | jit.LIK_GAMMA) != []


@pytest.mark.parametrize("dims", DIMS_GRID, ids=lambda d: "-".join(map(str, d)))
def test_families_equal_the_poisson_reach(dims):
    from tensorbnn_amd import jit
    want = jit.families(dims, jit.LIK_POIS)
    assert want == jit.families(dims, jit.LIK_GAUSS)
    assert jit.families(dims, jit.LIK_POIS | jit.LIK_GAMMA) == want
    assert jit.families(dims, jit.LIK_POIS | jit.LIK_GAMMA | jit.LIK_WEIGHTED) == jit.families(dims, jit.LIK_POIS | jit.LIK_WEIGHTED) == want


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
        assert _admission(dims, nat.ACT_NONE, nat.LIK_GAMMA, lik_df=4.0)[0] >= 0
        for act in (nat.ACT_TANH, nat.ACT_SIGMOID, nat.ACT_EXP):         # the output is the log of the mean: no last activation
            rc, err = _admission(dims, act, nat.LIK_GAMMA, lik_df=4.0)
            assert rc == -1 and "Gamma" in err and "no activation" in err, err
    for df in (0.0, -1.0, float("nan"), float("inf")):
        rc, err = _admission([5, 8, 1], nat.ACT_NONE, nat.LIK_GAMMA, lik_df=df)
        assert rc == -1 and "lik_df" in err, (df, err)
    for sd in (0.0, -0.5, float("nan")):                                  # fixed_sd is not read
        assert _admission([5, 8, 1], nat.ACT_NONE, nat.LIK_GAMMA, fixed_sd=sd, lik_df=4.0)[0] >= 0
    for unknown in (4, 6, 7, 9, 11, 13, 15, -1):
        rc, err = _admission([5, 8, 3], nat.ACT_NONE, unknown, lik_df=4.0)
        assert rc == -1 and "unknown likelihood" in err
    # lik_df stays ignored under the Gaussian kinds and Poisson
    for lik in (nat.LIK_GAUSSIAN, nat.LIK_FIXED_GAUSSIAN, nat.LIK_POISSON):
        assert _admission([5, 8, 1], nat.ACT_NONE, lik, lik_df=float("nan"))[0] >= 0
    # an ahead-of-time Gaussian table is no table for the Gamma network of the same layers (the library holds no ahead-of-time Poisson
    # table: test_gamma_library_cross_compiles_checked registers a Poisson library and asks again)
    for dims in ([7, 33, 18, 50, 2], [5, 50, 50, 50, 1]):
        assert _admission(dims, nat.ACT_NONE, nat.LIK_FIXED_GAUSSIAN)[0] > 0
        assert _admission(dims, nat.ACT_NONE, nat.LIK_POISSON)[0] == 0
        assert _admission(dims, nat.ACT_NONE, nat.LIK_GAMMA, lik_df=4.0)[0] == 0


def test_header_text():
    import os
    from tensorbnn_amd import _native as nat
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    hdr = open(os.path.join(root, "include", "tbnn.h")).read()
    assert "TBNN_LIK_GAMMA = 14" in hdr and "TBNN_LIK_HETERO_GAUSSIAN = 12" in hdr and "TBNN_LIK_NEG_BINOMIAL = 10" in hdr
    assert "#define TBNN_ABI_VERSION 3" in hdr and nat.ABI_VERSION == 3
    assert "a log a - lgamma(a) + (a - 1) log y - a f - a y exp(-f)" in hdr and "dL/df = a (y exp(-f) - 1)" in hdr
    common = open(os.path.join(root, "tensorbnn_amd", "csrc", "common.hpp")).read()
    assert "enum { SHAPE_LIK_GAMMA = 16 };" in common and "gamma_term" in common and "gamma_elem" in common
    hpp = open(os.path.join(root, "tensorbnn_amd", "csrc", "kernels_ensemble.hpp")).read()
    assert "ens_gamma_p" in hpp and "itmax" in hpp.split("double ens_gamma_p")[1][:900]          # the series' loop has its bound


@pytest.mark.parametrize("dims,skip,family,name,weighted", [
    ([3, 12, 12, 1], "", "fast3", b"<relu,none,gamma;3,12,12,1>", False),
    ([20, 64, 64, 3], "wide", "mid", b"jit-mid<relu,none,gamma,weighted;20,64,64,3>", True),
])
def test_gamma_library_cross_compiles_checked(tmp_path, monkeypatch, dims, skip, family, name, weighted):
    """jit.build of a narrow and a weighted mid-width Gamma shape: hipcc for gfx950 through checked_compile, the MFMA hazard check clean,
    the kernel name carrying gamma"""
    import os
    from tensorbnn_amd import _native as nat, jit
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    monkeypatch.setenv("TBNN_JIT_DIR", str(tmp_path))
    monkeypatch.setenv("TBNN_JIT_SKIP", skip)
    so = jit.build(layers_for(dims, nat.ACT_RELU), nat.LIK_GAMMA, weighted=weighted)
    assert so and os.path.exists(so)
    st = jit.lint_status(so)
    assert st.startswith(family + ":") and "listing checked" in st and "disassembly clean" in st, st
    lib = C.CDLL(so)
    buf = (C.c_char * 4096)()
    assert lib.tbnn_jit_ops(buf) == 0
    assert name in bytes(buf), bytes(buf)[:400]
    if weighted:
        return
    # a Poisson table is no table for the Gamma network of the same layers, and the other way round: the Poisson library of the shape
    # registered, then this one
    monkeypatch.delenv("TBNN_REGISTERED", raising=False)
    pso = jit.build(layers_for(dims, nat.ACT_RELU), nat.LIK_POISSON)
    assert pso and pso != so
    before = (_admission(dims, nat.ACT_NONE, nat.LIK_POISSON)[0], _admission(dims, nat.ACT_NONE, nat.LIK_GAMMA, lik_df=2.0)[0])
    assert nat.lib.tbnn_register_kernel_lib(pso.encode()) >= 0, nat.lib.tbnn_last_error().decode()
    assert _admission(dims, nat.ACT_NONE, nat.LIK_POISSON)[0] > 0
    assert _admission(dims, nat.ACT_NONE, nat.LIK_GAMMA, lik_df=2.0)[0] == before[1]
    if before == (0, 0):
        assert nat.lib.tbnn_register_kernel_lib(so.encode()) >= 0, nat.lib.tbnn_last_error().decode()
        assert _admission(dims, nat.ACT_NONE, nat.LIK_GAMMA, lik_df=2.0)[0] > 0


# ---------------------------------------------------------------------------------------------------------------------- incomplete gamma
def _log1pmx(mu):
    if abs(mu) >= 0.03125:
        return math.log1p(mu) - mu
    t = 0.0
    for k in range(15, 1, -1):
        t = (1.0 if k & 1 else -1.0) / k + mu * t
    return mu * mu * t


def _logpref(a, x):
    if a < 32.0:
        return a * math.log(x) - x - math.lgamma(a + 1.0)
    r = 1.0 / a
    r2 = r * r
    return a * _log1pmx((x - a) / a) - 0.5 * math.log(2.0 * math.pi * a) - r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0)))


def _series(a, x, itmax):
    ap, d, s = a, 1.0, 1.0
    for _ in range(itmax):
        ap += 1.0
        d *= x / ap
        s += d
        if d < s * 1e-17:
            break
    return s


def port_gamma_q(a, x):
    """csrc/kernels_ensemble.hpp ens_gamma_q below its Temme threshold, statement by statement"""
    if x <= 0.0:
        return 1.0
    lp = _logpref(a, x)
    series = x < a + 1.0
    if lp < -80.0:
        return 1.0 if series else 0.0
    pref = math.exp(lp)
    itmax = int(10.0 * math.sqrt(max(a, x))) + 100
    if series:
        return max(1.0 - pref * _series(a, x, itmax), 0.0)
    tiny = 1e-300
    b, c = x + 1.0 - a, 1.0 / tiny
    d = 1.0 / b
    h = d
    for it in range(1, itmax + 1):
        an = -it * (it - a)
        b += 2.0
        d = an * d + b
        if abs(d) < tiny:
            d = tiny
        c = b + an / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        de = d * c
        h *= de
        if abs(de - 1.0) < 2.3e-16:
            break
    return min(pref * a * h, 1.0)


def port_gamma_p(a, x):
    """csrc/kernels_ensemble.hpp ens_gamma_p: the series' side returned directly, 1 - Q elsewhere"""
    if not x > 0.0:
        return 0.0
    if x == math.inf:
        return 1.0
    if not x < a + 1.0:
        return 1.0 - port_gamma_q(a, x)
    lp = _logpref(a, x)
    if lp < -80.0:
        return 0.0
    return min(math.exp(lp) * _series(a, x, int(10.0 * math.sqrt(max(a, x))) + 100), 1.0)


GAMMA_GRID_SHAPES = (0.05, 0.5, 1.0, 2.0, 10.0, 37.5, 200.0, 5000.3)


def gamma_grid(a):
    """x / a swept over e^-6 .. e^3, and x within a +- 8 sqrt a (the positive part)"""
    return np.unique(np.concatenate([a * np.exp(np.linspace(-6.0, 3.0, 91)),
                                     np.maximum(a + math.sqrt(a) * np.linspace(-8.0, 8.0, 65), a * 1e-3)]))


PORT_FIGURE = 5e-15          # measured: the worst |port - scipy.special.gammainc| over the grid (printed on every run)


def test_incomplete_gamma_port_against_scipy():
    """the device's series and fraction are valid for every a > 0: the NumPy port against scipy.special.gammainc / gammaincc at
    non-integer shapes, shapes below 1 included.  Absolute error within 4 x the figure measured for the port; the side formed directly
    (P on the series' side, Q on the fraction's) also relatively, within 4 x 2.4e-13 where it is above 1e-30 (where the prefactor is
    below e^-80 = 1.8e-35 the function answers 0 or 1 by design and nothing is summed)."""
    from scipy.special import gammainc, gammaincc
    worst_abs, worst_rel = 0.0, 0.0
    for a in GAMMA_GRID_SHAPES:
        xs = gamma_grid(a)
        p = np.array([port_gamma_p(a, x) for x in xs])
        q = np.array([port_gamma_q(a, x) for x in xs])
        P, Q = gammainc(a, xs), gammaincc(a, xs)
        ea = max(np.abs(p - P).max(), np.abs(q - Q).max())
        left = xs < a + 1.0
        direct, ref = np.where(left, p, q), np.where(left, P, Q)
        ok = ref > 1e-30
        er = float(np.max(np.abs(direct[ok] - ref[ok]) / ref[ok]))
        print(f"[gamma] incomplete gamma port, a {a:g}: {xs.size} points, abs err {ea:.3e}, the direct side's relative err {er:.3e}")
        worst_abs, worst_rel = max(worst_abs, ea), max(worst_rel, er)
        assert np.all((p >= 0) & (p <= 1) & (q >= 0) & (q <= 1))
    print(f"[gamma] incomplete gamma port: worst abs err {worst_abs:.3e} (recorded {PORT_FIGURE:.1e}), worst relative err of the direct side {worst_rel:.3e}")
    assert worst_abs <= 4 * PORT_FIGURE
    assert worst_rel <= 4 * 2.4e-13
    # a small lower tail is not formed as 1 - (1 - P): relative accuracy where 1 - Q would have none
    for a, x in ((0.5, 1e-12), (0.05, 1e-200), (2.0, 1e-9), (37.5, 8.0)):
        want = float(gammainc(a, x))
        assert want < 1e-5 and abs(port_gamma_p(a, x) - want) <= 1e-12 * want, (a, x)
