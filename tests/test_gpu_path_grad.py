"""GPU: tbnn_ensemble_integrated_grad (csrc/kernels_path_grad.hpp) against the fp64 reference of tests/path_grad_ref.py.  Every network's
attributions are held to the reference within its band and diff to the fp64 forward at the two end points; the three planes are held to
fp64 moments of the device's own attributions.  Also chunks, weights, transform, scale, duplicates, baseline=None, refusals, the predictor.
Measured worst err / tol of per_network on an MI355X at P = 16 / 32 / 64: headline-tanh 5.1e-6 / 5.1e-6 / 4.2e-6, relu-small 2.3e-4 /
2.0e-4 / 2.8e-4, one-input 1.6e-4 / 2.8e-4 / 2.4e-4, no-hidden 3.3e-3 / 4.0e-3 / 4.1e-3, odd-widths 1.9e-4 / 1.4e-4 / 1.8e-4, 16-outputs
9.4e-5 / 8.2e-5 / 9.3e-5, 16-row-tile 5.4e-6 (P = 16); 8 networks, exp, scale 2.5: 4.2e-6 / 3.7e-6 / 3.5e-6.  diff: at most 1.7e-2."""
import numpy as np
import pytest

import path_grad_ref as pg

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def make_chain(native, spec):
    return native.Chain(pg.ig.layers_of(spec), likelihood=1, fixed_sd=0.7, jit=False, kernel=native.KERNEL_GENERIC)


def check_planes(tag, res, w=None):
    """mean, var and abs_mean against fp64 moments of the device's own per-network attributions (the bounds of test_gpu_input_grad)"""
    a = res["per_network"].astype(np.float64)
    m = a.shape[0]
    w = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
    ws = w.reshape(-1, 1, 1, 1) / w.sum()
    mean = (ws * a).sum(axis=0)
    span, mag = np.abs(a - a[0]).max(axis=0), np.abs(a).max(axis=0)
    assert np.all(np.abs(res["mean"] - mean) <= 4 * m * U * (span + mag)), tag
    assert np.all(np.abs(res["var"] - (ws * (a - mean) ** 2).sum(axis=0)) <= 8 * m * U * span * span), tag
    assert np.all(np.abs(res["abs_mean"] - (ws * np.abs(a)).sum(axis=0)) <= 4 * m * U * mag), tag


@pytest.mark.parametrize("tag,P", pg.RUNS)
def test_attributions_diff_and_planes(native, tag, P):
    spec, X, thetas, base = pg.problem(tag)
    attr, tol, flagged, diff, dtol = pg.attributions(spec, thetas, X, base, P)
    keep = pg.check_rows(tag, flagged, P)
    ch = make_chain(native, spec)
    res = ch.ensemble_integrated_grad(thetas, X, baseline=base, points=P, per_network=True)
    ch.close()
    assert res["per_network"].shape == attr.shape and res["per_network"].dtype == np.float32
    w, at = pg.ig.worst(res["per_network"], attr, tol, keep)
    wd, atd = pg.ig.worst(res["diff"], diff, dtol, np.ones(len(X), dtype=bool))
    print(f"[path_grad] {tag} P={P}: worst err/tol {w:.2e} at (network, output, input, row) = {at}; diff {wd:.2e} at {atd}; {int(flagged.sum())} flagged")
    assert w <= 1.0 and wd <= 1.0, (tag, P, w, at, wd, atd)
    check_planes(tag, res)


@pytest.mark.parametrize("P", pg.POINTS)
def test_chunks_weights_transform_duplicates_and_no_baseline(native, monkeypatch, P):
    spec, X, thetas, base = pg.problem("headline-tanh", m=8)
    thetas[5] = thetas[1]                                                          # slots of two different chunks
    w = np.array([1, 0, 2, 3, 0.5, 1, 4, 1], dtype=np.float32)
    ch = make_chain(native, spec)
    args = dict(points=P, weights=w, xform=native.XFORM_EXP, scale=2.5, per_network=True)
    whole = ch.ensemble_integrated_grad(thetas, X, baseline=base, **args)
    none, zeros = (ch.ensemble_integrated_grad(thetas, X, baseline=b, **args) for b in (None, np.zeros_like(base)))
    budget = 3 * spec.n_params + 5
    assert min(8, budget // spec.n_params) == 3                                    # the driver's rule: 3 + 3 + 2
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    cut = ch.ensemble_integrated_grad(thetas, X, baseline=base, **args)
    ch.close()
    for k in ("mean", "var", "abs_mean", "per_network", "diff"):
        assert np.array_equal(whole[k].view(np.uint8), cut[k].view(np.uint8)), k
        assert np.array_equal(none[k].view(np.uint8), zeros[k].view(np.uint8)), k
    assert np.array_equal(whole["per_network"][1].view(np.uint32), whole["per_network"][5].view(np.uint32))
    attr, tol, flagged, diff, dtol = pg.attributions(spec, thetas, X, base, P, xform=pg.ig.XFORM_EXP, scale=2.5)
    worst, wd = pg.ig.worst(whole["per_network"], attr, tol, ~flagged), pg.ig.worst(whole["diff"], diff, dtol, ~flagged)
    print(f"[path_grad] headline-tanh P={P}, 8 networks, exp, scale 2.5: worst err/tol and where: {worst}; diff: {wd}")
    assert worst[0] <= 1.0 and wd[0] <= 1.0 and not flagged.any(), (worst, wd)
    check_planes("weighted", whole, w)


def test_refusals(native):
    spec, X, thetas, base = pg.problem("odd-widths")
    ch = make_chain(native, spec)
    for name, kw in (("points must be 16, 32 or 64", dict(points=8)), ("points must be 16, 32 or 64", dict(points=17)),
                     ("baseline 2 is not finite", dict(baseline=np.where(np.arange(33) == 2, np.nan, base))), ("SOFTMAX", dict(xform=native.XFORM_SOFTMAX))):
        with pytest.raises(RuntimeError, match=name):
            ch.ensemble_integrated_grad(thetas, X, **kw)
    ch.close()
    spec, X, thetas, base = pg.problem("16-row-tile")
    ch = make_chain(native, spec)
    with pytest.raises(RuntimeError, match="points = 32 needs the 64-row tile.*40944"):
        ch.ensemble_integrated_grad(thetas, X, baseline=base, points=32)
    ch.close()


def test_predictor_round_trip(native, tmp_path, monkeypatch):
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.likelihood import CategoricalLikelihood, GaussianLikelihood
    from tensorbnn_amd.network import network
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(72)
    X = rng.uniform(-2, 2, (40, 2)).astype(np.float32)
    Y = (np.sin(2 * X[:, :1]) + 0.3 * rng.standard_normal((40, 1))).astype(np.float32)
    net = network(np.float32, 2, X, Y, X[:20], Y[:20])
    net.add(DenseLayer(2, 8, seed=1000)); net.add(Tanh())
    net.add(DenseLayer(8, 1, seed=3000))
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    net.train(20, 2, GaussianLikelihood(sd=0.5), folderName="reg", networksPerFile=1, verbose=False)
    p = predictor(str(tmp_path / "reg") + "/", likelihood=GaussianLikelihood(sd=0.5))
    res = p.integratedGradients(X, baseline=[0.1, -0.2], points=32, perNetwork=True)
    assert res["mean"].shape == res["sd"].shape == res["abs_mean"].shape == (1, 2, 40) and res["importance"].shape == (1, 2)
    assert res["per_network"].shape == (p.numNetworks, 1, 2, 40) and res["diff_mean"].shape == res["completeness_gap"].shape == (1, 40)
    assert np.array_equal(res["importance"], res["abs_mean"].mean(axis=2)) and np.array_equal(res["importance_sd"], res["abs_mean"].std(axis=2))
    gap = res["diff_mean"] - res["mean"].sum(axis=1)
    assert np.all(np.abs(res["completeness_gap"] - gap) <= 4 * U * (np.abs(res["diff_mean"]) + np.abs(res["mean"]).sum(axis=1)))
    assert np.all(np.isfinite(res["sd"])) and np.all(res["importance"] > 0)
    with pytest.raises(ValueError, match="softmax"):
        predictor(str(tmp_path / "reg") + "/", likelihood=CategoricalLikelihood()).integratedGradients(X)
