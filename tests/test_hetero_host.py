"""CPU: the heteroscedastic Gaussian likelihood (TBNN_LIK_HETERO_GAUSSIAN) without a GPU -- the oracle's heteroscedastic likelihood against
central differences and SciPy, its fp32 arm (the kernel's own operations) inside HALF the GPU module's bands on every case of
tests/test_gpu_hetero.py, the Python class, the kernels' likelihood code and the run-time kernel plumbing, the C ABI's admission rules
(tbnn_fused_kernel_available runs the same descriptor check as tbnn_create), the target padding, and a cross-compile of two shapes through
the checked compile."""
import ctypes as C
import math

import numpy as np
import pytest

import hetero_ref as hr
import tbnn_oracle as o
from tensor_checks import tensor_errs
from test_negbin_host import layers_for


def test_reference_formula_against_scipy():
    from scipy.stats import norm
    from tensorbnn_amd.likelihood import HeteroscedasticGaussianLikelihood
    rng = np.random.default_rng(0)
    f, g, y = rng.normal(size=200), rng.uniform(-5.0, 5.0, 200), rng.normal(size=200) * 3.0
    lik = HeteroscedasticGaussianLikelihood()
    assert lik.kind == 12 and lik.hypers == [] and not lik.mainProbsInHypers
    want = norm.logpdf(y, loc=f, scale=np.exp(g))
    got = lik.logDensity(f, g, y)
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert np.allclose(o.hetero_terms(np.stack([f, g]), y), want, rtol=1e-12, atol=1e-12)
    # the clip: g beyond +-log(1e8) is read as the bound
    for gg in (25.0, -25.0):
        assert lik.logDensity(0.0, gg, 1e-9) == lik.logDensity(0.0, math.copysign(o.LOG_CLIP, gg), 1e-9)
    # makeResponseLikelihood: [1, rows], one target per row in any of the three layouts
    pred = lambda *_a: np.stack([f, g]).astype(np.float32)
    base = lik.makeResponseLikelihood(None, predict=pred, realVals=y.astype(np.float32))
    assert base.shape == (1, 200) and base.dtype == np.float64
    for yy in (y.reshape(-1, 1), np.stack([y, 7.0 * y], axis=1)):
        assert np.array_equal(lik.makeResponseLikelihood(None, predict=pred, realVals=yy.astype(np.float32)), base)
    import tensorbnn_amd
    assert tensorbnn_amd.HeteroscedasticGaussianLikelihood is HeteroscedasticGaussianLikelihood


def test_reference_gradient_against_central_differences():
    spec, X, Y, theta, eta = hr.problem_of([5, 8, 2], 40, o.ACT_TANH, o.PRIOR_CAUCHY)
    th = theta.astype(np.float64)
    w = np.random.default_rng(2).integers(0, 3, 40).astype(np.float64)
    for weights in (None, w):
        lp, g = o.target_log_prob_and_grad(spec, th, eta, X, Y, np.float64, weights)
        h = 1e-6
        for j in range(spec.n_params):
            e = np.zeros_like(th)
            e[j] = h
            num = (o.target_log_prob_and_grad(spec, th + e, eta, X, Y, np.float64, weights)[0]
                   - o.target_log_prob_and_grad(spec, th - e, eta, X, Y, np.float64, weights)[0]) / (2 * h)
            assert abs(num - g[j]) <= 2e-6 * max(1.0, abs(g[j])), (j, num, g[j])
    # integer weights are duplicated rows, the constant included
    idx = np.repeat(np.arange(40), w.astype(int))
    a = o.target_log_prob_and_grad(spec, th, eta, X, Y, np.float64, w)
    b = o.target_log_prob_and_grad(spec, th, eta, X[idx], Y[idx], np.float64)
    assert math.isclose(a[0], b[0], rel_tol=1e-12) and np.allclose(a[1], b[1], rtol=1e-10, atol=1e-12)
    # outside the clip the derivative with respect to g is 0, and a NaN g stays NaN in both arms
    for dt in (np.float64, np.float32):
        t, d = o.hetero_pair(np.array([[0.0, 0.0, 0.0], [25.0, -25.0, np.nan]]), np.array([1.0, 1e-9, 1.0]), dt)
        assert d[1][0] == 0 and d[1][1] == 0 and np.isfinite(t[:2]).all() and np.isnan(t[2]) and np.isnan(d[0][2])


@pytest.mark.parametrize("name", list(hr.CASES))
def test_reference_in_fp32_stays_inside_half_the_bands(name):
    """CPU arithmetic only: the kernel's formula in fp32 against the fp64 definition -- value, gradient per tensor, and the log accept ratio
    of the GPU module's injected transition -- within HALF the GPU bands; and the problem has what the module promises of it"""
    spec, X, Y, theta, eta = hr.problem(name)
    lp64, g64 = hr.ref64(name)
    lp32, g32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)
    gv, gg = abs(lp32 - lp64) / max(abs(lp64), 1.0), tensor_errs(spec, g32, g64, 1e-3)
    f = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    q = (Y.astype(np.float64) - f[0]) ** 2 * np.exp(-2.0 * f[1])
    print(f"[hetero] {name}: g in [{f[1].min():.2f}, {f[1].max():.2f}], r^2 u in [{q.min():.2e}, {q.max():.2e}]; "
          f"fp32 arm: value gap {gv:.3e}, gradient gap {max(gg):.3e}")
    assert Y.shape == (X.shape[0],) and np.abs(f[1]).max() < 6.0
    n16 = (X.shape[0] // 16) * 16
    tiles = q[:n16].reshape(-1, 16)
    assert np.all(tiles.min(axis=1) < 1e-2) and np.all(tiles.max(axis=1) > 50.0)        # both regimes in every full tile
    assert gv <= 2e-6 and max(gg) <= 5e-5, (gv, gg)
    p0 = np.random.default_rng(4).standard_normal(spec.n_params).astype(np.float32)
    r64 = o.weight_step(spec, theta, eta, X, Y, hr.step_size(name), 4, p0, -1e30, np.float64)
    r32 = o.weight_step(spec, theta, eta, X, Y, hr.step_size(name), 4, p0, -1e30, np.float32, np.float64)
    tol = 2e-2 + 1e-4 * abs(r64.log_accept_ratio) + 4e-7 * abs(lp64)
    print(f"[hetero] {name}: lar fp32 {r32.log_accept_ratio:.6g} fp64 {r64.log_accept_ratio:.6g} (band {tol:.3g})")
    assert abs(r32.log_accept_ratio - r64.log_accept_ratio) <= 0.5 * tol


@pytest.mark.parametrize("name", hr.CLIP_CASES)
def test_clip_cases_in_fp32(name):
    spec, X, Y, theta, eta = hr.problem(name)
    j = hr.last_bias_index(spec, 1)
    for bias in (25.0, -25.0):
        th = theta.copy()
        th[j] = bias
        lp64, g64 = o.target_log_prob_and_grad(spec, th, eta, X, Y, np.float64)
        lp32, g32 = o.target_log_prob_and_grad(spec, th, eta, X, Y, np.float32)
        assert np.isfinite(lp32) and abs(lp32 - lp64) <= 2e-6 * abs(lp64) and max(tensor_errs(spec, g32, g64, 1e-3)) <= 5e-5
        assert g64[j] == o.prior_grad(spec.layers[-1], eta[-4:].astype(np.float64), *o.unflatten(spec, th.astype(np.float64))[-1], np.float64)[1][1, 0]


def test_cases_are_the_student_cases_ending_in_two():
    import student_ref as sr
    pairs = {"fast3": "fast3", "fast3_two_outputs": "fast3_two_outputs", "fast": "fast", "mid": "mid1", "tall": "tall", "wide": "wide1",
             "lay_last": "lay_last", "lay_separate": "lay_separate", "lay_tail": "lay_tail", "generic": "generic", "traj": "traj"}
    assert list(hr.CASES) == list(pairs)
    for name, src in pairs.items():
        c, s = hr.CASES[name], sr.CASES[src]
        assert c[0] == s[0][:-1] + [2] and c[2:] == s[2:6]
        assert c[1] == (380 if name == "traj" else s[1])          # (the trajectory kernel of a 2-output network takes 384 rows: hetero_ref)


# ---------------------------------------------------------------------------------------------------------------------- codes and plumbing
def test_codes_shape_and_cache_key():
    from tensorbnn_amd import _native as nat, jit
    assert nat.LIK_HETERO_GAUSSIAN == 12 and jit.LIK_HETERO == 16
    assert jit.lik_code(nat.LIK_HETERO_GAUSSIAN) == 16 and jit.lik_code(nat.LIK_HETERO_GAUSSIAN, True) == 20
    # every existing code keeps its value
    assert (jit.LIK_GAUSS, jit.LIK_BERN, jit.LIK_CAT, jit.LIK_POIS, jit.LIK_WEIGHTED, jit.LIK_STUDENT, jit.LIK_NEGBIN) == (0, 1, 2, 3, 4, 8, 8)
    assert [jit.lik_code(k) for k in (nat.LIK_GAUSSIAN, nat.LIK_FIXED_GAUSSIAN, nat.LIK_BERNOULLI, nat.LIK_CATEGORICAL, nat.LIK_POISSON,
                                      nat.LIK_STUDENT_T, nat.LIK_NEG_BINOMIAL)] == [0, 0, 1, 2, 3, 8, 11]
    assert [jit.lik_code(k, True) for k in (nat.LIK_GAUSSIAN, nat.LIK_BERNOULLI, nat.LIK_POISSON, nat.LIK_STUDENT_T, nat.LIK_NEG_BINOMIAL)] == [4, 5, 7, 12, 15]
    layers = layers_for([20, 64, 64, 2], nat.ACT_RELU)
    g, gw, t, tw = (jit.shape_of(layers, lk, w) for lk, w in ((nat.LIK_FIXED_GAUSSIAN, False), (nat.LIK_FIXED_GAUSSIAN, True),
                                                              (nat.LIK_HETERO_GAUSSIAN, False), (nat.LIK_HETERO_GAUSSIAN, True)))
    assert g[:3] == t[:3] == tw[:3] and (g[3], gw[3], t[3], tw[3]) == (0, 4, 16, 20)
    assert len({jit.cache_key(*s) for s in (g, gw, t, tw)}) == 4
    src = jit.source(*t, "mid")
    inner = src.split("Shape<")[1].split(">")[0]
    assert "SHAPE_LIK_HETERO" in inner and "WEIGHTED" not in inner and src != jit.source(*g, "mid")
    inner = jit.source(*tw, "mid").split("Shape<")[1].split(">")[0]
    assert "SHAPE_LIK_HETERO" in inner and "SHAPE_LIK_WEIGHTED" in inner
    assert jit.source(*g, "mid").split("Shape<")[1].split(">")[0].split(", ")[2] == "false"       # the Gaussian spelling is untouched


DIMS_GRID = [c[0] for c in hr.CASES.values()] + [[2, 12, 2], [1, 100, 2], [20, 100, 100, 2], [8, 300, 300, 2], [5, 20, 20, 3], [5, 50, 50, 50, 1],
                                                 [30, 80, 80, 10]]


@pytest.mark.parametrize("dims", DIMS_GRID, ids=lambda d: "-".join(map(str, d)))
def test_families_equal_the_gaussian_reach_at_two_outputs(dims):
    from tensorbnn_amd import jit
    want = jit.families(dims, jit.LIK_GAUSS) if dims[-1] == 2 else []
    assert jit.families(dims, jit.LIK_HETERO) == want
    assert jit.families(dims, jit.LIK_HETERO | jit.LIK_WEIGHTED) == want
    if dims[-1] == 2:
        assert want == jit.families(dims, jit.LIK_GAUSS | jit.LIK_WEIGHTED)


def _admission(dims, act_last, lik, fixed_sd=0.1, lik_df=0.0):
    from tensorbnn_amd import _native as nat
    layers = layers_for(dims, nat.ACT_RELU, act_last)
    arr = (nat.LayerDesc * len(layers))(*[nat.LayerDesc(*l) for l in layers])
    desc = nat.NetDesc(len(layers), arr, lik, fixed_sd, nat.KERNEL_AUTO, lik_df)
    rc = nat.lib.tbnn_fused_kernel_available(C.byref(desc))
    return rc, nat.lib.tbnn_last_error().decode()


def test_c_abi_admission(monkeypatch):
    from tensorbnn_amd import _native as nat
    monkeypatch.setenv("TBNN_REGISTERED", "0")
    LIK = nat.LIK_HETERO_GAUSSIAN
    assert C.sizeof(nat.NetDesc) == 32 and nat.lib.tbnn_abi_version() == 3
    assert _admission([5, 8, 2], nat.ACT_NONE, LIK)[0] >= 0
    for d_out in (1, 3, 4, 16):
        rc, err = _admission([5, 8, d_out], nat.ACT_NONE, LIK)
        assert rc == -1 and "needs exactly 2 outputs: mean and log-sd" in err, err
    for act in (nat.ACT_TANH, nat.ACT_SIGMOID, nat.ACT_EXP, nat.ACT_RELU):
        rc, err = _admission([5, 8, 2], act, LIK)
        assert rc == -1 and "no activation" in err, err
    for sd in (0.0, -0.5, float("nan")):                                  # fixed_sd and lik_df are not read
        assert _admission([5, 8, 2], nat.ACT_NONE, LIK, fixed_sd=sd, lik_df=float("nan"))[0] >= 0
    for unknown in (4, 6, 7, 9, 11, 13, -1):
        rc, err = _admission([5, 8, 2], nat.ACT_NONE, unknown)
        assert rc == -1 and "unknown likelihood" in err
    # an ahead-of-time Gaussian table is no table for the heteroscedastic network of the same layers
    assert _admission([7, 33, 18, 50, 2], nat.ACT_NONE, nat.LIK_FIXED_GAUSSIAN)[0] > 0
    assert _admission([7, 33, 18, 50, 2], nat.ACT_NONE, LIK)[0] == 0


def test_header():
    import os
    from tensorbnn_amd import _native as nat
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tbnn.h")).read()
    assert "TBNN_LIK_HETERO_GAUSSIAN = 12" in hdr and "TBNN_LIK_NEG_BINOMIAL = 10" in hdr and "#define TBNN_ABI_VERSION 3" in hdr
    assert nat.ABI_VERSION == 3


def test_target_padding():
    from tensorbnn_amd import _native as nat
    y = np.arange(5, dtype=np.float64) + 0.5
    for yy in (y, y.reshape(5, 1), y.reshape(1, 5)):
        out = nat.pad_targets(yy, 5, 2, nat.LIK_HETERO_GAUSSIAN)
        assert out.dtype == np.float32 and out.shape == (5, 2) and out.flags["C_CONTIGUOUS"]
        assert np.array_equal(out[:, 0], y.astype(np.float32)) and np.all(out[:, 1] == 0)
    two = np.stack([y, -y], axis=1)
    assert np.array_equal(nat.pad_targets(two, 5, 2, nat.LIK_HETERO_GAUSSIAN), two.astype(np.float32))
    # every other likelihood: the plain reshape, as before
    assert np.array_equal(nat.pad_targets(np.arange(10.0), 5, 2, nat.LIK_FIXED_GAUSSIAN), np.arange(10, dtype=np.float32).reshape(5, 2))
    with pytest.raises(ValueError):
        nat.pad_targets(y, 5, 2, nat.LIK_FIXED_GAUSSIAN)
    with pytest.raises(ValueError):
        nat.pad_targets(np.arange(7.0), 5, 2, nat.LIK_HETERO_GAUSSIAN)


@pytest.mark.parametrize("dims,skip,family,name,weighted", [
    ([3, 12, 12, 2], "", "fast3", b"<relu,none,hetero-gaussian;3,12,12,2>", False),
    ([20, 64, 64, 2], "wide", "mid", b"jit-mid<relu,none,hetero-gaussian,weighted;20,64,64,2>", True),
])
def test_hetero_library_cross_compiles_checked(tmp_path, monkeypatch, dims, skip, family, name, weighted):
    """jit.build of a narrow and a weighted mid-width heteroscedastic shape: hipcc for gfx950 through checked_compile, the MFMA hazard
    check clean, the kernel name carrying hetero-gaussian"""
    import os
    from tensorbnn_amd import _native as nat, jit
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    monkeypatch.setenv("TBNN_JIT_DIR", str(tmp_path))
    monkeypatch.setenv("TBNN_JIT_SKIP", skip)
    so = jit.build(layers_for(dims, nat.ACT_RELU), nat.LIK_HETERO_GAUSSIAN, weighted=weighted)
    assert so and os.path.exists(so)
    st = jit.lint_status(so)
    assert st.startswith(family + ":") and "listing checked" in st and "disassembly clean" in st, st
    lib = C.CDLL(so)
    buf = (C.c_char * 4096)()
    assert lib.tbnn_jit_ops(buf) == 0
    assert name in bytes(buf), bytes(buf)[:400]
