"""GPU: tbnn_ensemble_input_grad (csrc/kernels_input_grad.hpp) against the fp64 reverse pass of tests/input_grad_ref.py.  Every network's
Jacobian (jac_out) is held to the reference within its band on every unflagged row; the three planes are held to fp64 moments of jac_out
itself within 4 m 2^-53 of the span, which isolates the reduction.  What the cases reach is in input_grad_ref.CASES; here also the
carry-over between chunks, the transform and the scale on a generic handle, duplicates, a NaN weight, the refusals and the predictor.

Measured worst err / tol of jac_out on an MI355X: headline 1.4e-5, one-input 1.4e-4, no-hidden 0.205, odd-widths 1.0e-3, 16-outputs
2.3e-4, 16-row-tile 1.2e-5, 16-layers 1.3e-8; the headline on a generic handle under exp and scale 2.5: 3.7e-5."""
import numpy as np
import pytest

import input_grad_ref as ig

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def make_chain(native, spec, kernel=None):
    return native.Chain(ig.layers_of(spec), likelihood=1, fixed_sd=0.7, jit=False,
                        kernel=native.KERNEL_GENERIC if kernel is None else kernel)


def check_planes(tag, res, w=None):
    """mean, var and abs_mean against fp64 moments of the device's own per-network Jacobians"""
    jac = res["per_network"].astype(np.float64)
    m = jac.shape[0]
    w = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
    ws = w.reshape(-1, 1, 1, 1) / w.sum()
    mean = (ws * jac).sum(axis=0)
    span = np.abs(jac - jac[0]).max(axis=0)
    mag = np.abs(jac).max(axis=0)
    assert np.all(np.abs(res["mean"] - mean) <= 4 * m * U * (span + mag)), tag
    assert np.all(np.abs(res["var"] - (ws * (jac - mean) ** 2).sum(axis=0)) <= 8 * m * U * span * span), tag
    assert np.all(np.abs(res["abs_mean"] - (ws * np.abs(jac)).sum(axis=0)) <= 4 * m * U * mag), tag


@pytest.mark.parametrize("tag", list(ig.CASES))
def test_jacobian_and_planes(native, tag):
    spec, X, thetas = ig.problem(tag)
    J, A, flagged = ig.jacobian(spec, thetas, X)
    keep = ig.check_rows(tag, flagged)
    ch = make_chain(native, spec, native.KERNEL_AUTO if tag == "headline" else None)
    res = ch.ensemble_input_grad(thetas, X=X, per_network=True)
    ch.close()
    assert res["per_network"].shape == J.shape and res["per_network"].dtype == np.float32
    w, at = ig.worst(res["per_network"], J, ig.tolerance(spec, J, A), keep)
    print(f"[input_grad] {tag}: worst err/tol {w:.2e} at (network, output, input, row) = {at}; {int(flagged.sum())} rows flagged")
    assert w <= 1.0, (tag, w, at)
    check_planes(tag, res)


def test_chunks_weights_transform_and_duplicates(native, monkeypatch):
    spec, X, thetas = ig.problem("headline")
    thetas[5] = thetas[1]                                                          # slots of two different chunks
    w = np.array([1, 0, 2, 3, 0.5, 1, 4, 1], dtype=np.float32)
    J, A, flagged = ig.jacobian(spec, thetas, X, xform=ig.XFORM_EXP, scale=2.5)
    ch = make_chain(native, spec)
    assert ch.kernel_name.startswith("generic")
    whole = ch.ensemble_input_grad(thetas, X=X, weights=w, xform=native.XFORM_EXP, scale=2.5, per_network=True)
    budget = 3 * spec.n_params + 5
    assert min(8, budget // spec.n_params) == 3                                    # the driver's rule: 3 + 3 + 2
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    cut = ch.ensemble_input_grad(thetas, X=X, weights=w, xform=native.XFORM_EXP, scale=2.5, per_network=True)
    ch.close()
    for k in ("mean", "var", "abs_mean", "per_network"):
        assert np.array_equal(whole[k].view(np.uint8), cut[k].view(np.uint8)), k
    assert np.array_equal(whole["per_network"][1].view(np.uint32), whole["per_network"][5].view(np.uint32))
    worst, at = ig.worst(whole["per_network"], J, ig.tolerance(spec, J, A), ~flagged)
    print(f"[input_grad] headline, generic handle, exp, scale 2.5: worst err/tol {worst:.2e} at {at}")
    assert worst <= 1.0, (worst, at)
    check_planes("weighted", whole, w)


def test_nan_weight_stays_in_its_network(native):
    spec, X, thetas = ig.problem("headline")
    thetas[2, spec.offsets()[-1][0] + 3] = np.nan                                   # a weight of the last layer: every unit below it
    ch = make_chain(native, spec)
    res = ch.ensemble_input_grad(thetas, X=X, per_network=True)
    ch.close()
    assert np.isnan(res["per_network"][2]).all() and np.isfinite(np.delete(res["per_network"], 2, axis=0)).all()
    assert all(np.isnan(res[k]).all() for k in ("mean", "var", "abs_mean"))


def test_refusals(native):
    spec, X, thetas = ig.problem("odd-widths")
    ch = make_chain(native, spec)
    with pytest.raises(RuntimeError, match="SOFTMAX"):
        ch.ensemble_input_grad(thetas, X=X, xform=native.XFORM_SOFTMAX)
    with pytest.raises(RuntimeError, match="m < 1"):
        ch.ensemble_input_grad(thetas[:0], X=X)
    ch.close()
    # the stated limit (include/tbnn.h): (d_in + sum out) 17 + 2 max out 17 + 2176 floats above 40944
    d_in = (40944 - 2176 - 2 * 17) // 17                                           # the first d_in whose 16-row tile does not fit with one output
    assert (d_in + 1) * 17 + 2 * 17 + 2176 > 40944 >= (d_in - 1 + 1) * 17 + 2 * 17 + 2176
    big = ig.fr.spec_of([d_in, 1], [], 0)
    ch = make_chain(native, big)
    with pytest.raises(RuntimeError, match="16-row tile.*40944"):
        ch.ensemble_input_grad(np.zeros((1, big.n_params), dtype=np.float32), X=np.zeros((1, d_in), dtype=np.float32))
    ch.close()


def test_predictor_round_trip(native, tmp_path, monkeypatch):
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.likelihood import CategoricalLikelihood, GaussianLikelihood
    from tensorbnn_amd.network import network
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(71)
    X = rng.uniform(-2, 2, (120, 2)).astype(np.float32)
    Y = (np.sin(2 * X[:, :1]) + 0.3 * rng.standard_normal((120, 1))).astype(np.float32)
    net = network(np.float32, 2, X, Y, X[:50], Y[:50])
    net.add(DenseLayer(2, 8, seed=1000)); net.add(Tanh())
    net.add(DenseLayer(8, 1, seed=3000))
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    net.train(30, 2, GaussianLikelihood(sd=0.5), folderName="reg", networksPerFile=1, verbose=False)
    p = predictor(str(tmp_path / "reg") + "/", likelihood=GaussianLikelihood(sd=0.5))
    res = p.inputGradient(X, perNetwork=True)
    assert res["mean"].shape == res["sd"].shape == res["abs_mean"].shape == (1, 2, 120)
    assert res["per_network"].shape == (p.numNetworks, 1, 2, 120) and res["importance"].shape == (1, 2)
    assert np.array_equal(res["importance"], res["abs_mean"].mean(axis=2)) and np.array_equal(res["importance_sd"], res["abs_mean"].std(axis=2))
    assert np.all(res["importance"] > 0) and np.all(np.isfinite(res["sd"]))
    with pytest.raises(ValueError, match="softmax"):
        predictor(str(tmp_path / "reg") + "/", likelihood=CategoricalLikelihood()).inputGradient(X)
