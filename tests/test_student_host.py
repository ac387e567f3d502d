"""StudentTLikelihood (TBNN_LIK_STUDENT_T) without a GPU: the oracle's fp64 Student-t likelihood against SciPy's t density (or, without
SciPy, the Cauchy density at nu = 1) and against central differences, the Python class, the kernels' likelihood code and the run-time
kernel plumbing, the C ABI's admission rules (tbnn_fused_kernel_available runs the descriptor checks of tbnn_create on the host), and
`test_reference_in_fp32_stays_inside_the_bands`: the kernel's own formula in fp32 (the oracle's fp32 arm) against the fp64 definition at
every case of tests/test_gpu_student.py, inside the project's bands -- value 4e-6 relative, gradient 1e-4 of each tensor's largest entry, log
accept ratio 2e-2 + 1e-4 |lar| + 4e-7 |logp|.  That test decided the form of log1p the kernels use (csrc/common.hpp log1p_fast: a series
below 1/4, the hardware log2 above).  Measured, fp32 arm vs fp64 over the 13 cases: value gaps 1.5e-9 .. 9.4e-8, gradient gaps 9.9e-8 .. 1.8e-6:
no case needs a band of its own."""
import ctypes as C
import math

import numpy as np
import pytest

import student_ref as sr
import tbnn_oracle as o
from tensor_checks import tensor_errs

DIMS_GRID = [c[0] for c in sr.CASES.values()] + [[2, 12, 1], [1, 100, 1], [5, 20, 20, 3], [20, 100, 100, 2], [8, 90, 130, 70, 3], [8, 300, 300, 1]]


def layers_for(dims, hidden_act, last_act=0):
    return [(dims[i], dims[i + 1], hidden_act if i < len(dims) - 2 else last_act, 0) for i in range(len(dims) - 1)]


# ---------------------------------------------------------------------------------------------------------------------- the reference
def test_reference_formula():
    rng = np.random.default_rng(1)
    f = rng.standard_normal((3, 50))
    y = f.T + rng.standard_normal((50, 3)) * np.array([0.1, 1.0, 30.0])
    try:
        from scipy.stats import t as student
    except ImportError:
        student = None
    for nu, s in ((1.0, 0.1), (2.5, 1.0), (30.0, 0.1), (1e4, 1.0)):
        got = o.student_terms(f, y, nu, s)
        assert got.shape == (3, 50) and got.dtype == np.float64
        if student is not None:
            # (the constant differences two lgamma values, 3.8e4 each at nu = 1e4: a few of THEIR ulps is all either side can promise)
            atol = 1e-13 + 4 * np.spacing(math.lgamma(0.5 * (nu + 1.0)))
            np.testing.assert_allclose(got, student.logpdf(y.T, nu, loc=f, scale=s), rtol=1e-13, atol=atol)
        if nu == 1.0:       # the Cauchy density 1 / (pi s (1 + (r / s)^2))
            np.testing.assert_allclose(got, -np.log(np.pi * s * (1.0 + ((y.T - f) / s) ** 2)), rtol=1e-13, atol=1e-13)


def test_reference_gradient_against_central_differences():
    spec, X, Y, theta, eta = sr.problem_of([3, 6, 5, 2], 40, o.ACT_TANH, o.PRIOR_CAUCHY, 2.5, 0.3)
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
    # the data term's constant counts W = sum w rows; integer weights are duplicated rows
    idx = np.repeat(np.arange(40), w.astype(int))
    a = o.target_log_prob_and_grad(spec, th, eta, X, Y, np.float64, w)
    b = o.target_log_prob_and_grad(spec, th, eta, X[idx], Y[idx], np.float64)
    assert math.isclose(a[0], b[0], rel_tol=1e-12) and np.allclose(a[1], b[1], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("name", list(sr.CASES))
def test_reference_in_fp32_stays_inside_the_bands(name):
    """CPU arithmetic only: the kernel's formula in fp32 against the fp64 definition -- value, gradient per tensor, and the log accept ratio
    of the GPU module's injected transition"""
    spec, X, Y, theta, eta = sr.problem(name)
    nu = spec.lik_df
    lp64, g64 = sr.ref64(name)
    lp32, g32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)
    gv, gg = abs(lp32 - lp64) / max(abs(lp64), 1.0), tensor_errs(spec, g32, g64, 1e-3)
    f = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
    u = (Y.reshape(f.shape[1], -1).T - f) ** 2 / (nu * spec.fixed_sd ** 2)
    print(f"[student] {name}: nu {nu:g} s {spec.fixed_sd:g}, r^2/(nu s^2) in [{u.min():.1e}, {u.max():.1e}]; fp32 arm: value gap {gv:.3e}, gradient gap {max(gg):.3e}")
    assert u.min() < 0.01 and u.max() > 0.25                    # both branches of the kernel's log1p, in one problem
    assert gv <= 4e-6 and max(gg) <= 1e-4, (gv, gg)
    p0 = np.random.default_rng(4).standard_normal(spec.n_params).astype(np.float32)
    r64 = o.weight_step(spec, theta, eta, X, Y, sr.step_size(name), 4, p0, -1e30, np.float64)
    r32 = o.weight_step(spec, theta, eta, X, Y, sr.step_size(name), 4, p0, -1e30, np.float32, np.float64)
    tol = 2e-2 + 1e-4 * abs(r64.log_accept_ratio) + 4e-7 * abs(lp64)
    print(f"[student] {name}: lar fp32 {r32.log_accept_ratio:.6g} fp64 {r64.log_accept_ratio:.6g} (band {tol:.3g})")
    assert abs(r32.log_accept_ratio - r64.log_accept_ratio) <= tol


# ---------------------------------------------------------------------------------------------------------------------- the Python class
def test_python_class_terms_and_shapes():
    import tensorbnn_amd
    from tensorbnn_amd import _native as nat
    from tensorbnn_amd.likelihood import StudentTLikelihood
    assert tensorbnn_amd.StudentTLikelihood is StudentTLikelihood
    lik = StudentTLikelihood(df=4.0, sd=0.3)
    assert nat.LIK_STUDENT_T == 8 and lik.kind == nat.LIK_STUDENT_T and lik.df == 4.0 and lik.fixed_sd == pytest.approx(0.3)
    assert lik.hypers == [] and lik.mainProbsInHypers is False
    assert lik.calcultateLogProb(hypers=[1, 2, 3]) == [0, 0, 0]
    rng = np.random.default_rng(3)
    f = rng.standard_normal((2, 31)).astype(np.float32)                   # [d_out, rows], as network.predict returns
    y = (f.T + 0.3 * rng.standard_normal((31, 2))).astype(np.float32)      # [rows, d_out]
    y[5] += 12.0
    out = lik.makeResponseLikelihood(None, predict=lambda train, _x: f, realVals=y)
    assert out.shape == (2, 31) and out.dtype == np.float64 and np.all(np.isfinite(out))
    np.testing.assert_allclose(out, o.student_terms(f.astype(np.float64), y.astype(np.float64), 4.0, float(np.float64(0.3))), rtol=1e-12)
    for bad in ({"df": 0.0, "sd": 1.0}, {"df": -1.0, "sd": 1.0}, {"df": float("nan"), "sd": 1.0}, {"df": float("inf"), "sd": 1.0}, {"df": 3.0, "sd": 0.0}):
        with pytest.raises(ValueError):
            StudentTLikelihood(**bad)


def test_predictor_host_paths():
    from tensorbnn_amd.likelihood import StudentTLikelihood
    from tensorbnn_amd.predictor import predictor
    rng = np.random.default_rng(5)
    X = rng.standard_normal((20, 2)).astype(np.float32)
    preds = [rng.standard_normal((2, 20)).astype(np.float32) for _ in range(2)]
    Y = (preds[0].T + 0.1 * rng.standard_normal((20, 2))).astype(np.float32)
    p = predictor.__new__(predictor)                     # no saved networks, no device: only the host-side steps
    p.predict = lambda x, n=1: preds
    p.hypers = []
    lik = StudentTLikelihood(df=3.0, sd=0.1)
    got = p._data_logprob(lik, X, Y, 1)
    for g, f in zip(got, preds):
        assert np.isclose(g, o.student_terms(f.astype(np.float64), Y.astype(np.float64), 3.0, 0.1).sum(), rtol=1e-6)
    assert got[0] > got[1]
    p.likelihood = lik
    for call in (lambda: p.predictiveQuantiles(X, 0.5), lambda: p.predictiveInterval(X), lambda: p.predictiveCDF(X, Y)):
        with pytest.raises(ValueError, match="StudentTLikelihood"):
            call()


# ---------------------------------------------------------------------------------------------------------------------- codes and plumbing
def test_codes_shape_and_cache_key():
    from tensorbnn_amd import _native as nat, jit
    assert jit.LIK_STUDENT == 8
    assert jit.lik_code(nat.LIK_STUDENT_T) == 8 and jit.lik_code(nat.LIK_STUDENT_T, True) == 12
    # every existing code keeps its value
    assert (jit.LIK_GAUSS, jit.LIK_BERN, jit.LIK_CAT, jit.LIK_POIS, jit.LIK_WEIGHTED) == (0, 1, 2, 3, 4)
    assert [jit.lik_code(k) for k in (nat.LIK_GAUSSIAN, nat.LIK_FIXED_GAUSSIAN, nat.LIK_BERNOULLI, nat.LIK_CATEGORICAL, nat.LIK_POISSON)] == [0, 0, 1, 2, 3]
    layers = layers_for([30, 80, 80, 10], nat.ACT_RELU)
    g, gw, t, tw = (jit.shape_of(layers, lk, w) for lk, w in ((nat.LIK_FIXED_GAUSSIAN, False), (nat.LIK_FIXED_GAUSSIAN, True),
                                                              (nat.LIK_STUDENT_T, False), (nat.LIK_STUDENT_T, True)))
    assert g[:3] == t[:3] == tw[:3] and (g[3], gw[3], t[3], tw[3]) == (0, 4, 8, 12)
    assert len({jit.cache_key(*s) for s in (g, gw, t, tw)}) == 4
    src = jit.source(*t, "mid")
    assert "SHAPE_LIK_STUDENT" in src.split("Shape<")[1].split(">")[0] and src != jit.source(*g, "mid")
    inner = jit.source(*tw, "mid").split("Shape<")[1].split(">")[0]
    assert "SHAPE_LIK_STUDENT" in inner and "SHAPE_LIK_WEIGHTED" in inner
    assert jit.source(*g, "mid").split("Shape<")[1].split(">")[0].split(", ")[2] == "false"       # the Gaussian spelling is untouched


@pytest.mark.parametrize("dims", DIMS_GRID, ids=lambda d: "-".join(map(str, d)))
def test_families_equal_the_gaussian_reach(dims):
    from tensorbnn_amd import jit
    want = jit.families(dims, jit.LIK_GAUSS)
    assert jit.families(dims, jit.LIK_STUDENT) == want
    assert jit.families(dims, jit.LIK_STUDENT | jit.LIK_WEIGHTED) == jit.families(dims, jit.LIK_GAUSS | jit.LIK_WEIGHTED) == want


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
    assert C.sizeof(nat.NetDesc) == 32 and nat.NetDesc.lik_df.offset == 28 and nat.NetDesc.lik_df.size == 4      # where `reserved` was
    for dims in ([5, 8, 1], [5, 8, 3], [5, 8, 40]):                       # any d_out >= 1
        for act in (nat.ACT_NONE, nat.ACT_TANH, nat.ACT_SIGMOID):         # any last activation the Gaussian kinds accept
            assert _admission(dims, act, nat.LIK_STUDENT_T, lik_df=4.0)[0] >= 0
    for df in (0.0, -1.0, float("nan"), float("inf")):
        rc, err = _admission([5, 8, 1], nat.ACT_NONE, nat.LIK_STUDENT_T, lik_df=df)
        assert rc == -1 and "lik_df" in err, (df, err)
    for sd in (0.0, -0.5, float("nan")):
        rc, err = _admission([5, 8, 1], nat.ACT_NONE, nat.LIK_STUDENT_T, fixed_sd=sd, lik_df=4.0)
        assert rc == -1 and "fixed_sd" in err, (sd, err)
    for unknown in (4, 6, 7, -1, 9):
        rc, err = _admission([5, 8, 3], nat.ACT_NONE, unknown, lik_df=4.0)
        assert rc == -1 and "unknown likelihood" in err
    # lik_df is ignored under every other likelihood
    for lik in (nat.LIK_GAUSSIAN, nat.LIK_FIXED_GAUSSIAN, nat.LIK_POISSON):
        assert _admission([5, 8, 1], nat.ACT_NONE, lik, lik_df=float("nan"))[0] >= 0
    # an ahead-of-time Gaussian table is no table for the Student-t network of the same layers (tbnn_mid.hip: relu;7,33,18,50,2)
    for dims in ([7, 33, 18, 50, 2], [5, 50, 50, 50, 1]):
        assert _admission(dims, nat.ACT_NONE, nat.LIK_GAUSSIAN)[0] > 0
        assert _admission(dims, nat.ACT_NONE, nat.LIK_FIXED_GAUSSIAN)[0] > 0
        assert _admission(dims, nat.ACT_NONE, nat.LIK_STUDENT_T, lik_df=4.0)[0] == 0


def test_the_setter_is_bound_and_declared():
    import os
    from tensorbnn_amd import _native as nat
    bound = {name: (res, args) for name, res, args in nat.SYMBOLS}
    assert bound["tbnn_set_lik_df"] == (C.c_int, [C.c_void_p, C.c_float])
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tbnn.h")).read()
    assert "int tbnn_set_lik_df(tbnn_handle h, float df);" in hdr and "TBNN_LIK_STUDENT_T = 8" in hdr and "float lik_df;" in hdr
    assert nat.lib.tbnn_set_lik_df(None, 3.0) == -1 and "null handle" in nat.lib.tbnn_last_error().decode()
    assert nat.ABI_VERSION == 3


@pytest.mark.parametrize("dims,skip,family,name,weighted", [
    ([3, 12, 12, 1], "", "fast3", b"<relu,none,student-t;3,12,12,1>", False),
    ([20, 64, 64, 3], "wide", "mid", b"jit-mid<relu,none,student-t,weighted;20,64,64,3>", True),
])
def test_student_library_cross_compiles_checked(tmp_path, monkeypatch, dims, skip, family, name, weighted):
    """jit.build of a narrow and a weighted mid-width Student-t shape: hipcc for gfx950 through checked_compile, the MFMA hazard check clean"""
    import os
    from tensorbnn_amd import _native as nat, jit
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    monkeypatch.setenv("TBNN_JIT_DIR", str(tmp_path))
    monkeypatch.setenv("TBNN_JIT_SKIP", skip)
    so = jit.build(layers_for(dims, nat.ACT_RELU), nat.LIK_STUDENT_T, weighted=weighted)
    assert so and os.path.exists(so)
    st = jit.lint_status(so)
    assert st.startswith(family + ":") and "listing checked" in st and "disassembly clean" in st, st
    lib = C.CDLL(so)
    buf = (C.c_char * 4096)()
    assert lib.tbnn_jit_ops(buf) == 0
    assert name in bytes(buf), bytes(buf)[:400]
