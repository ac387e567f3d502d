"""No GPU: the yardsticks of tests/test_gpu_optimize.py and the host side of the optimiser's surface.  The NumPy restatement of
tbnn_optimize's step (tests/optim_ref.py) against torch.optim.Adam on the CPU in fp64; the header, the binding and the reference's
signatures; the refusal of a leaky-ReLU alpha; and the fp32 arm of the restatement on the free-run cases, whose gap to fp64 is what the
GPU test's band is 8 x of."""
import inspect
import os
import re

import numpy as np
import pytest

import optim_ref as R
import tbnn_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("amsgrad", [True, False])
def test_restatement_equals_torch_adam(amsgrad):
    """30 steps of torch.optim.Adam(amsgrad=..., maximize=True) in fp64 on the oracle's gradients: <= 1e-12 (a CPU check found 1.1e-16)"""
    import torch
    spec, X, Y, theta0, eta = R.problem([6, 24, 24, 1], 300, o.PRIOR_GAUSSIAN)
    p = torch.tensor(theta0.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([p], lr=R.LR, betas=(R.B1, R.B2), eps=R.EPS, amsgrad=amsgrad, maximize=True)
    theta = theta0.astype(np.float64)
    m = v = vhat = np.zeros_like(theta)
    worst = 0.0
    for t in range(1, 31):
        g = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[1]
        theta, m, v, vhat = R.adam_step(theta, g, m, v, vhat, t, R.LR, amsgrad=amsgrad, dtype=np.float64)
        p.grad = torch.tensor(o.target_log_prob_and_grad(spec, p.detach().numpy(), eta, X, Y, np.float64)[1])
        opt.step()
        worst = max(worst, float(np.abs(p.detach().numpy() - theta).max()))
    print(f"[optimize] restatement vs torch.optim.Adam(amsgrad={amsgrad}): {worst:.2e}")
    assert worst <= 1e-12
    assert np.abs(theta - theta0).max() > 20 * R.LR            # (the run went somewhere)
    # run() is the same loop
    assert np.array_equal(R.run(spec, theta0, eta, X, Y, 30, amsgrad=amsgrad, dtype=np.float64)[1], theta)


def test_header_and_binding_declare_the_optimiser(native):
    txt = open(os.path.join(ROOT, "include", "tbnn.h")).read()
    assert "#define TBNN_ABI_VERSION 3 " in txt and native.ABI_VERSION == 3 and native.lib.tbnn_abi_version() == 3
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int tbnn_optimize\(tbnn_handle h, const tbnn_optim_cfg\* cfg, int32_t n_steps, int32_t reset, tbnn_optim_out\* out\s*,\s*double\* trace\s*\);", code)
    assert re.search(r"int tbnn_optim_state\(tbnn_handle h, float\* m, float\* v, float\* vhat, float\* g, int32_t\* t\);", code)
    assert "enum { TBNN_OPT_POSTERIOR = 0, TBNN_OPT_LIKELIHOOD = 1 };" in code
    assert "float lr, beta1, beta2, epsilon; int32_t amsgrad, objective, check_every, keep_best;" in code
    assert "int32_t steps_done, diverged, best_step, n_checks; double obj_first, obj_last, obj_best; float device_us;" in code
    bound = {name for name, _, _ in native.SYMBOLS}
    assert {"tbnn_optimize", "tbnn_optim_state"} <= bound
    assert [f for f, _ in native.OptimCfg._fields_] == ["lr", "beta1", "beta2", "epsilon", "amsgrad", "objective", "check_every", "keep_best"]
    assert [f for f, _ in native.OptimOut._fields_] == ["steps_done", "diverged", "best_step", "n_checks", "obj_first", "obj_last", "obj_best", "device_us"]
    import ctypes
    assert ctypes.sizeof(native.OptimCfg) == 32 and ctypes.sizeof(native.OptimOut) == 48
    assert (native.OPT_POSTERIOR, native.OPT_LIKELIHOOD) == (0, 1)
    for cls in (native.Chain, native.ChainGroup):
        sig = inspect.signature(cls.optimize)
        assert list(sig.parameters)[1:] == ["steps", "lr", "beta1", "beta2", "epsilon", "amsgrad", "objective", "check_every", "keep", "reset"]
        d = {k: p.default for k, p in sig.parameters.items()}
        assert (d["lr"], d["beta1"], d["beta2"], d["epsilon"], d["amsgrad"], d["objective"], d["check_every"], d["keep"], d["reset"]) == \
            (1e-2, 0.9, 0.999, 1e-8, True, "posterior", 10, "best", True)
        assert hasattr(cls, "optim_state")
    # a null handle is refused like everywhere else (no GPU needed)
    assert native.lib.tbnn_optimize(None, None, 1, 1, None, None) < 0 and native.lib.tbnn_optim_state(None, None, None, None, None, None) < 0


REFERENCE_ARGS = ["hidden", "inputDims", "outputDims", "width", "cycles", "epochs", "alpha", "trainIn", "trainOut", "valIn", "valOut", "name",
                  "callbacks", "callbackMetric", "patience"]          # tensorBNN/BNN_functions.py:60-75, :183-198


def test_bnn_functions_signatures_match_the_reference():
    import tensorbnn_amd
    from tensorbnn_amd import BNN_functions as B
    from tensorbnn_amd.network import network
    for fn in (B.trainBasicRegression, B.trainBasicClassification):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == REFERENCE_ARGS
        assert [sig.parameters[k].default for k in REFERENCE_ARGS[12:]] == [True, "val_loss", 10]
        assert all(sig.parameters[k].default is inspect.Parameter.empty for k in REFERENCE_ARGS[:12])
        assert "full-batch" in B.__doc__.lower() and "alpha" in fn.__doc__
    assert tensorbnn_amd.trainBasicRegression is B.trainBasicRegression and tensorbnn_amd.trainBasicClassification is B.trainBasicClassification
    sig = inspect.signature(network.pretrain)
    assert list(sig.parameters)[1:] == ["likelihood", "cycles", "epochs", "learningRate", "decay", "objective", "patience", "checkEvery", "verbose"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [3, 1000, 0.01, 10.0, "posterior", 10, 10, True]
    assert "mini-batches of 32" in network.pretrain.__doc__


@pytest.mark.parametrize("fn", ["trainBasicRegression", "trainBasicClassification"])
def test_leaky_alpha_is_refused_without_a_gpu(fn):
    import tensorbnn_amd
    X, Y = np.zeros((8, 2), np.float32), np.zeros((8, 1), np.float32)
    with pytest.raises(NotImplementedError, match="leaky"):
        getattr(tensorbnn_amd, fn)(1, 2, 1, 4, 1, 1, 0.3, X, Y, X, Y, "unused")


@pytest.mark.parametrize("name", list(R.FREE_RUN))
def test_fp32_arm_of_the_free_run_stays_close(name):
    """the yardstick of the GPU free-run test: the restatement in fp32 against fp64 over the same 30 steps -- below 1e-5 (trace, relative) and
    1e-2 lr (theta) on every chosen case, so 8 x its gap is a band an fp32 kernel can be held to and a wrong update cannot meet"""
    pb, (tr64, th64), (tr32, th32) = R.free_run(name)
    gt, gth = R.free_gaps(tr32, th32, tr64, th64)
    moved = float(np.abs(th64 - pb[3]).max() / R.LR)
    print(f"[optimize] {name}: fp32 arm vs fp64: trace {gt:.3e}, theta {gth:.3e} lr; the run moved theta by {moved:.1f} lr; objective {tr64[0]:.6g} -> {tr64[-1]:.6g}")
    assert len(tr64) == R.FREE_STEPS + 1 and np.all(np.isfinite(tr64)) and tr64[-1] > tr64[0]
    assert 0 < gt < 1e-5 and 0 < gth < 1e-2
    assert 0.01 * moved > 10 * 8 * gth                          # a step wrong by one per cent leaves the band by more than an order of magnitude
