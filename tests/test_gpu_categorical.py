"""GPU: CategoricalLikelihood (TBNN_LIK_CATEGORICAL) -- a softmax over each row's outputs -- on every kernel family that takes it: the mid,
tall and wide fused kernels (cat_delta4 on the MFMA output tile, the row's max and sums across the four lane groups), the layered family
on each of its likelihood paths (k_lay_tail, k_lay_last, k_lay_lik; any number of outputs) and the generic kernel.  Against the fp64
oracle (o.target_log_prob_and_grad under LIK_CATEGORICAL): value, gradient per tensor, forward logits, an
injected weight transition with both decisions, a hyper transition (prior only: the likelihood has no hyper), every launch repeated bit
for bit; saturated logits, soft labels; a Gaussian and a categorical chain of the same shape in one process; trainChains against solo
runs; an end-to-end fit."""
import numpy as np
import pytest

import tbnn_oracle as o
from tensor_checks import layers_of, tensor_err
from test_gpu_freerun import SEED

pytestmark = pytest.mark.gpu

FUSED = {"mid": "fast3,fast,tall,wide", "tall": "fast3,fast,mid,wide", "wide": "fast3,fast,mid,tall"}

CASES = {
    # dims, rows, hidden activation, prior, family, environment, labels
    "mid10": ([30, 80, 80, 10], 3001, o.ACT_RELU, o.PRIOR_CAUCHY, "mid", {}, "onehot"),          # ragged last tile
    "mid16_full_tile": ([12, 40, 48, 16], 1234, o.ACT_ELU, o.PRIOR_CAUCHY, "mid", {}, "onehot"),
    "mid3": ([20, 64, 64, 3], 4000, o.ACT_TANH, o.PRIOR_GAUSSIAN, "mid", {}, "soft"),
    "mid_few_rows": ([20, 64, 64, 5], 9, o.ACT_SIGMOID, o.PRIOR_CAUCHY, "mid", {}, "onehot"),
    "mid_saturated": ([20, 64, 64, 5], 2000, o.ACT_RELU, o.PRIOR_CAUCHY, "mid", {}, "saturated"),
    "tall10": ([784, 20, 20, 10], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "tall", {}, "onehot"),     # the reference's MNIST shape, ten classes
    "tall_one_hidden3": ([300, 33, 3], 333, o.ACT_ELU, o.PRIOR_CAUCHY, "tall", {}, "soft"),
    "tall_saturated": ([784, 20, 20, 10], 700, o.ACT_RELU, o.PRIOR_CAUCHY, "tall", {}, "saturated"),
    "wide10": ([10, 200, 200, 10], 3001, o.ACT_RELU, o.PRIOR_CAUCHY, "wide", {}, "onehot"),
    "wide3_three_middle": ([8, 90, 130, 70, 3], 777, o.ACT_TANH, o.PRIOR_GAUSSIAN, "wide", {}, "soft"),
    "wide_saturated": ([10, 200, 200, 10], 1000, o.ACT_RELU, o.PRIOR_CAUCHY, "wide", {}, "saturated"),
    # the layered family (no run-time instantiation, no tall registry): which likelihood kernel runs follows from lay_plan_shape
    "lay_last": ([784, 100, 100, 10], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "layered", {}, "onehot"),                       # k_lay_last
    "lay_separate": ([784, 100, 100, 10], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "layered", {"TBNN_LAY_LAST": "0"}, "onehot"),  # k_lay_lik
    "lay_tail": ([784, 20, 20, 10], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "layered", {}, "onehot"),                         # k_lay_tail
    "lay_tail_off": ([784, 20, 20, 10], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "layered", {"TBNN_LAY_TAIL": "0"}, "soft"),   # k_lay_last
    "lay_both_off": ([784, 20, 20, 10], 1205, o.ACT_RELU, o.PRIOR_CAUCHY, "layered",
                     {"TBNN_LAY_TAIL": "0", "TBNN_LAY_LAST": "0"}, "onehot"),                                            # k_lay_lik
    "lay_k20": ([20, 64, 64, 20], 1500, o.ACT_TANH, o.PRIOR_CAUCHY, "layered", {}, "onehot"),                           # k_lay_lik, K > 16
    "lay_tail_k20": ([9, 30, 20], 450, o.ACT_TANH, o.PRIOR_GAUSSIAN, "layered", {}, "soft"),                            # k_lay_tail, two tiles
    "lay_saturated": ([784, 100, 100, 10], 800, o.ACT_RELU, o.PRIOR_CAUCHY, "layered", {}, "saturated"),
    "lay_two_classes": ([20, 64, 64, 2], 1000, o.ACT_RELU, o.PRIOR_CAUCHY, "layered", {}, "onehot"),                   # K = 2: no fused kernel
    "generic": ([5, 16, 16, 4], 517, o.ACT_TANH, o.PRIOR_CAUCHY, "generic", {}, "soft"),
    "generic_saturated": ([5, 16, 16, 4], 300, o.ACT_RELU, o.PRIOR_CAUCHY, "generic", {}, "saturated"),
}


def jit_jobs():
    """the run-time instantiations this module asks for (jit.prebuild's job format)"""
    jobs = []
    for dims, _n, act, prior, fam, _env, _lab in CASES.values():
        if fam in FUSED:
            jobs.append({"layers": [list(l) for l in layers_of(spec_of(dims, act, prior))], "likelihood": o.LIK_CATEGORICAL, "skip": FUSED[fam], "flags": ""})
    for dims, act in (([30, 80, 80, 10], o.ACT_RELU), ([2, 16, 16, 3], o.ACT_RELU)):
        spec = spec_of(dims, act, o.PRIOR_CAUCHY)
        jobs.append({"layers": [list(l) for l in layers_of(spec)], "likelihood": o.LIK_CATEGORICAL, "skip": "", "flags": ""})
    gspec = o.make_spec([30, 80, 80, 10], o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN)
    jobs.append({"layers": [list(l) for l in layers_of(gspec)], "likelihood": o.LIK_GAUSSIAN, "skip": FUSED["mid"], "flags": ""})
    # the predictor's forward chain of the fitted three-class network (a fixed-sd Gaussian handle: forward passes only)
    pspec = o.make_spec([2, 16, 16, 3], o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_FIXED_GAUSSIAN)
    jobs.append({"layers": [list(l) for l in layers_of(pspec)], "likelihood": o.LIK_FIXED_GAUSSIAN, "skip": "", "flags": ""})
    return [j for i, j in enumerate(jobs) if j not in jobs[:i]]


@pytest.fixture(scope="module", autouse=True)
def prebuilt():
    """compile this module's run-time shapes side by side before any test touches the GPU (cached: a second run compiles nothing)"""
    from tensorbnn_amd import jit
    jobs = jit_jobs()
    assert jit.prebuild(jobs) == len(jobs)


def spec_of(dims, act, prior):
    return o.make_spec(dims, act, prior, o.LIK_CATEGORICAL, o.ACT_NONE)


def softmax_rows(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def problem(name):
    dims, n, act, prior, _fam, _env, labels = CASES[name]
    _g, X, Yr, theta, eta = o.synth_problem(dims, n, act, prior, o.LIK_GAUSSIAN)     # X, teacher targets [n, K], the initial state
    spec = spec_of(dims, act, prior)
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1)
    eta = np.asarray(eta[:spec.n_hypers], dtype=np.float32)          # no likelihood hyper
    if labels == "soft":
        Y = softmax_rows(2.0 * Yr).astype(np.float32)
    else:
        Y = np.eye(dims[-1], dtype=np.float32)[np.argmax(Yr, axis=1)]
    if labels == "saturated":
        # the last layer scaled so that the logits reach +-80: a naive exp overflows in fp32 there
        f = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)
        s = 80.0 / np.abs(f).max()
        ow, ob = spec.offsets()[-1]
        theta = theta.copy()
        theta[ow:] = (theta[ow:].astype(np.float64) * s).astype(np.float32)
        assert np.abs(o.forward(spec, theta, X, np.float64)).max() > 70
    return spec, X, Y, theta, eta


def make_chain(native, monkeypatch, name, spec, **kw):
    fam, env = CASES[name][4], CASES[name][5]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if fam in FUSED:
        monkeypatch.setenv("TBNN_JIT_SKIP", FUSED[fam])
        ch = native.Chain(layers_of(spec), likelihood=o.LIK_CATEGORICAL, jit=True, **kw)
        assert ch.kernel_name.startswith(f"jit-{fam}") and ",categorical;" in ch.kernel_name, ch.kernel_name
    elif fam == "layered":
        monkeypatch.setenv("TBNN_TALL", "0")
        monkeypatch.setenv("TBNN_REGISTERED", "0")
        ch = native.Chain(layers_of(spec), likelihood=o.LIK_CATEGORICAL, jit=False, **kw)
        assert ch.kernel_name.startswith("layered<"), ch.kernel_name
    else:
        ch = native.Chain(layers_of(spec), likelihood=o.LIK_CATEGORICAL, kernel=native.KERNEL_GENERIC, **kw)
        assert ch.kernel_name == "generic", ch.kernel_name
    assert ch.H == 4 * len(spec.layers)
    return ch


def check_value_gradient(name, lp, g, spec, theta, eta, X, Y):
    lp64, g64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)
    assert np.isfinite(lp) and np.all(np.isfinite(g))
    assert abs(lp - lp64) <= 4e-6 * max(abs(lp64), 1.0), (name, lp, lp64)
    assert tensor_err(spec, g, g64, 1e-3) <= 1e-4, name


@pytest.mark.parametrize("name", list(CASES))
def test_value_gradient_forward(native, monkeypatch, name):
    spec, X, Y, theta, eta = problem(name)
    ch = make_chain(native, monkeypatch, name, spec)
    ch.set_data(X, Y)
    lp, g, st = ch.logp_grad(theta, eta)
    for _ in range(2):
        lp2, g2, st2 = ch.logp_grad(theta, eta)
        assert lp2 == lp and st2 == st and np.array_equal(g, g2)
    m = min(500, X.shape[0])
    f = ch.forward(X[:m], theta)
    assert np.array_equal(f, ch.forward(X[:m], theta))
    ch.close()
    check_value_gradient(name, lp, g, spec, theta, eta, X, Y)
    f64 = o.forward(spec, theta, X[:m], np.float64)
    assert f.shape == f64.shape == (spec.layers[-1].out_dim, m)
    assert np.abs(f - f64).max() <= 1e-4 * max(1.0, np.abs(f64).max())


@pytest.mark.parametrize("name", ["mid10", "mid3", "tall10", "tall_one_hidden3", "wide10", "wide3_three_middle", "lay_last", "lay_tail",
                                  "lay_k20", "generic"])
def test_transitions(native, monkeypatch, name):
    spec, X, Y, theta, eta = problem(name)
    rng = np.random.default_rng(4)
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    ch = make_chain(native, monkeypatch, name, spec, seed=SEED, chain_id=2)
    ch.set_data(X, Y)
    vg = lambda q: o.target_log_prob_and_grad(spec, q, eta, X, Y, np.float64)
    lp64 = vg(theta)[0]
    for log_u in (-1e30, 1e30):
        ch.set_state(theta); ch.set_hypers(eta)
        out = ch.hmc_step(3e-5, 4, p0=p0, log_u=log_u)
        ref = o.hmc_step(vg, theta, 3e-5, 4, p0, log_u, np.float64)
        assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
        assert bool(out["accepted"]) == ref.accepted == (log_u < 0)
        assert np.abs(ch.get_state() - ref.theta).max() <= 1e-5 * max(1.0, np.abs(ref.theta).max())
    # the hyper transition: the layer priors only (no likelihood hyper; the oracle adds a data term for the Gaussian likelihood alone)
    ph = rng.standard_normal(spec.n_hypers).astype(np.float32)
    ch.set_state(theta); ch.set_hypers(eta)
    ch.logp_grad(theta, eta)
    out = ch.hyper_step(1e-4, 9, p0=ph, log_u=-1e30)
    ref = o.hyper_step(spec, eta, theta, X, Y, 1e-4, 9, ph, -1e30, np.float64)
    assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= 2e-2 + 1e-3 * abs(ref.log_accept_ratio)
    assert np.allclose(ch.get_hypers(), ref.theta, rtol=1e-4, atol=1e-5)
    # after the accepted hyper transition the cached gradient is refreshed for the new priors: the next weight step starts from it
    lp_new, g_new, _ = ch.logp_grad(theta, ch.get_hypers())
    check_value_gradient(name, lp_new, g_new, spec, theta, ch.get_hypers(), X, Y)
    ch.close()


def test_gaussian_then_categorical_chain_of_one_shape(native, monkeypatch):
    """a Gaussian chain registers its mid-width table first; the categorical chain of the same layers must get its own table (the Gaussian
    one computes squared residuals) and match the categorical reference"""
    spec, X, Y, theta, eta = problem("mid10")
    monkeypatch.setenv("TBNN_JIT_SKIP", FUSED["mid"])
    gspec = o.make_spec([30, 80, 80, 10], o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN)
    gch = native.Chain(layers_of(gspec), likelihood=o.LIK_GAUSSIAN, jit=True)
    assert gch.kernel_name == "jit-mid<relu,none;30,80,80,10>", gch.kernel_name
    geta = np.concatenate([eta, [np.sqrt(0.1)]]).astype(np.float32)
    gch.set_data(X, Y)
    glp, gg, _ = gch.logp_grad(theta, geta)
    ch = native.Chain(layers_of(spec), likelihood=o.LIK_CATEGORICAL, jit=True)
    assert ch.kernel_name == "jit-mid<relu,none,categorical;30,80,80,10>", ch.kernel_name
    ch.set_data(X, Y)
    lp, g, _ = ch.logp_grad(theta, eta)
    assert np.array_equal(gch.logp_grad(theta, geta)[1], gg)            # the Gaussian chain unchanged beside it
    gch.close(); ch.close()
    check_value_gradient("mismatch", lp, g, spec, theta, eta, X, Y)
    glp64 = o.target_log_prob_and_grad(gspec, theta, geta, X, Y, np.float64)[0]
    assert abs(glp - glp64) <= 4e-6 * abs(glp64)


def blobs(n, seed):
    rng = np.random.default_rng(seed)
    centres = np.array([[0.0, 3.0], [-2.6, -1.5], [2.6, -1.5]])
    k = rng.integers(0, 3, n)
    X = (centres[k] + 0.6 * rng.standard_normal((n, 2))).astype(np.float32)
    return X, np.eye(3, dtype=np.float32)[k]


def make_net(X, Y, Xv, Yv, chain_id=0):
    from tensorbnn_amd.activationFunctions import Relu
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.network import network
    net = network(np.float32, 2, X, Y, Xv, Yv, chain_id=chain_id)
    net.add(DenseLayer(2, 16, seed=1000)); net.add(Relu())
    net.add(DenseLayer(16, 16, seed=2000)); net.add(Relu())
    net.add(DenseLayer(16, 3, seed=3000))
    net.setupMCMC(stepSizeStart=2e-3, stepSizeMin=5e-4, stepSizeMax=1e-2, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    return net


def test_train_chains_equal_solo_runs(tmp_path, monkeypatch, native):
    from tensorbnn_amd.likelihood import CategoricalLikelihood
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, Y = blobs(600, 1)
    Xv, Yv = blobs(200, 2)
    C, EPOCHS = 2, 16
    grp_net = make_net(X, Y, Xv, Yv)
    rec = grp_net.trainChains(C, EPOCHS, 4, CategoricalLikelihood(), adjustHypers=True, folderName="multi", networksPerFile=2)
    assert len(rec) == EPOCHS and all(len(r["main"]) == C for r in rec)
    for c in range(C):
        net = make_net(X, Y, Xv, Yv, chain_id=c)
        solo = net.train(EPOCHS, 4, CategoricalLikelihood(), adjustHypers=True, folderName="solo%d" % c, networksPerFile=2, verbose=False)
        assert net._chain.kernel_name.startswith("jit-mid<") and "categorical" in net._chain.kernel_name
        for rg, rs in zip(rec, solo):
            assert rg["eps"][c] == rs["eps"] and rg["L"][c] == rs["L"]
            assert rg["main"][c]["log_accept_ratio"] == rs["main"]["log_accept_ratio"] and rg["main"][c]["accepted"] == rs["main"]["accepted"]
            for k in ("log_accept_ratio", "accepted", "logp_old", "logp_new", "kinetic_old", "kinetic_new", "sjd"):
                assert rg["main"][c][k] == rs["main"][k], (c, rg["iter"], k)
            assert rg["hyper"][c]["log_accept_ratio"] == rs["hyper"]["log_accept_ratio"]
            assert rg["hyper_step_size"][c] == rs["hyper_step_size"]


def test_train_reaches_accuracy_on_blobs(tmp_path, monkeypatch, native):
    from tensorbnn_amd.likelihood import CategoricalLikelihood
    from tensorbnn_amd.metrics import CategoricalAccuracy
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TBNN_JIT", "1")
    X, Y = blobs(600, 1)
    Xv, Yv = blobs(300, 2)
    net = make_net(X, Y, Xv, Yv)
    acc0 = CategoricalAccuracy()
    acc0.calculate(net.predict(True), net.predict(False), Y, Yv)
    net.train(30, 5, CategoricalLikelihood(), metricList=[CategoricalAccuracy()], folderName="blobs", networksPerFile=1, verbose=False)
    acc = CategoricalAccuracy()
    acc.calculate(net.predict(True), net.predict(False), Y, Yv)
    assert acc.accuracyValidate > 0.9, (acc0.accuracyValidate, acc.accuracyValidate)
    # the saved networks, weighted by the categorical data term of the training rows
    p = predictor(str(tmp_path / "blobs") + "/")
    w = p._data_logprob(CategoricalLikelihood(), X, Y, 1)
    assert len(w) == p.numNetworks and all(np.isfinite(w)) and max(w) <= 0          # (a perfect fit rounds to 0)
