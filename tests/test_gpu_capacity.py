"""GPU: every fused kernel family at the limits of its admission rules (tests/edge_shapes.py), against the fp64 oracle through the C ABI.

For each edge case:
  (a) the largest shape the family admits runs on that family (TBNN_JIT_SKIP naming the others; a build that refuses it fails the test), from a
      library whose compile went through the MFMA hazard check; log-prob, gradient per tensor, forward, predict and forward_many against fp64 at
      the fuzz tolerances (test_gpu_fuzz.py) with no fp32-oracle or relu-kink tier; every launch three times and bit-identical;
  (b) an injected transition with both decisions and a hyper transition on that shape, against o.weight_step / o.hyper_step;
  (c) the first refused neighbour runs, with no TBNN_JIT_SKIP, on the first family jit.families names for it (or the layered family), and is
      checked as in (a) -- a neighbour deeper than the C ABI's 16 layers must be refused by tbnn_create;
  (d) the shapes whose fused build spills (edge_shapes.MUST_REFUSE), which the estimates refuse, run on the layered family and are checked as in (a).
A few edges run with a Bernoulli likelihood as well (edge_shapes.BERNOULLI), their outputs kept off saturation.
Row counts: a ragged last row tile; TBNN_FAST_GRID makes every workgroup of the narrow, mid and tall kernels walk many row tiles, and the wide
cases take enough rows that waves carry more than one tile."""
import numpy as np
import pytest

import edge_shapes as es
import tbnn_oracle as o
from tensor_checks import layers_of, tensor_err

pytestmark = pytest.mark.gpu

CASES = es.cases()
REFUSED_BY_BUILD = [dict(name=f"{fam}-spills", family=fam, dims=list(dims)) for fam, dims in es.MUST_REFUSE]
NEIGHBOURS = [c for c in CASES if c["refused"] is not None]
PREFIX = {"fast3": "jit-fast3", "fast": "jit-fast<", "mid": "jit-mid", "tall": "jit-tall", "wide": "jit-wide", "layered": "layered<"}
GRID = 3                          # TBNN_FAST_GRID: 1007 rows = 63 row tiles over 3 workgroups
N_ROWS, N_WIDE = 1007, 17009      # wide: 1064 row tiles over at most 256 workgroups of 4 waves


def _id(c, dims=None):
    return f"{c['name']}-{'x'.join(map(str, dims or c['dims']))}"


def problem(dims, n, lik=o.LIK_GAUSSIAN):
    """test_gpu_fuzz._problem's conditioning: tanh hidden layers, a long fan-in's inputs scaled to keep its pre-activations O(1), Bernoulli
    outputs off saturation"""
    spec, X, Y, theta, eta = o.synth_problem(dims, n, o.ACT_TANH, o.PRIOR_CAUCHY, lik)
    if dims[0] > 64:
        X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)
    if lik == o.LIK_BERNOULLI:
        theta = (theta * 0.3).astype(np.float32)
        f = o.forward(spec, theta, X, np.float64)
        assert np.all((f > 1e-4) & (f < 1 - 1e-4)), "Bernoulli outputs off saturation"
    return spec, X, Y, theta, eta


def setenv(monkeypatch, family, skip):
    monkeypatch.setenv("TBNN_JIT_SKIP", skip)
    if family != "wide":
        monkeypatch.setenv("TBNN_FAST_GRID", str(GRID))
    else:
        monkeypatch.delenv("TBNN_FAST_GRID", raising=False)


def check_library(native, spec, family):
    """the run-time library the chain runs on went through the hazard check inside its compile"""
    from tensorbnn_amd import jit
    so = jit.build(layers_of(spec), spec.likelihood)
    assert so is not None, f"{family}: no library for {[spec.layers[0].in_dim] + [l.out_dim for l in spec.layers]}"
    st = jit.lint_status(so)
    assert st.startswith(family + ":") and ("listing checked" in st or "disassembly clean" in st), st


def value_gradient_forward(native, spec, X, Y, theta, eta, family):
    """(a) / (c): returns the errors against their bounds"""
    ch = native.Chain(layers_of(spec), likelihood=spec.likelihood, fixed_sd=spec.fixed_sd, jit=True)
    try:
        name = ch.kernel_name
        assert name.startswith(PREFIX[family]), f"{family}: runs on {name}"
        if family != "layered":
            check_library(native, spec, family)
        ch.set_data(X, Y)
        lp, g, _ = ch.logp_grad(theta, eta)
        f, pr = ch.forward(X, theta), ch.predict(0, theta)
        th2 = np.stack([theta, (theta * np.float32(0.97)).astype(np.float32)])
        fm = ch.forward_many(th2, None, which=0)
        for _ in range(2):
            lp2, g2, _ = ch.logp_grad(theta, eta)
            assert lp2 == lp and np.array_equal(g2, g), f"{name}: a repeated launch differs (max {np.abs(g2 - g).max():.3e})"
            assert np.array_equal(ch.forward(X, theta), f) and np.array_equal(ch.predict(0, theta), pr), f"{name}: a repeated forward differs"
            assert np.array_equal(ch.forward_many(th2, None, which=0), fm), f"{name}: a repeated forward_many differs"
    finally:
        ch.close()
    lp64, g64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[:2]
    e_lp = abs(lp - lp64) / max(abs(lp64), 1.0)
    assert e_lp <= 4e-6, f"{name}: logp {lp} against {lp64} ({e_lp:.2e} relative, bound 4e-6)"
    e_g = tensor_err(spec, g, g64, 1e-3)
    assert e_g <= 1e-4, f"{name}: gradient {e_g:.3e} of the tensor's inf-norm (1e-4)"
    e_f = 0.0
    for got, th in ((f, theta), (pr, theta), (fm[0], th2[0]), (fm[1], th2[1])):
        f64 = o.forward(spec, th, X, np.float64)
        e_f = max(e_f, float(np.abs(got - f64).max()))
    assert e_f <= 1e-4, f"{name}: forward / predict / forward_many {e_f:.3e} (1e-4)"
    print(f"{name}: logp {e_lp:.2e} (4e-6) gradient {e_g:.2e} (1e-4) forward {e_f:.2e} (1e-4)")
    return name


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_admitted_edge_vs_fp64(native, monkeypatch, c):
    setenv(monkeypatch, c["family"], es.SKIP[c["family"]])
    spec, X, Y, theta, eta = problem(c["dims"], N_WIDE if c["family"] == "wide" else N_ROWS, c["lik"])
    value_gradient_forward(native, spec, X, Y, theta, eta, c["family"])


@pytest.mark.parametrize("c", NEIGHBOURS, ids=lambda c: _id(c, c["refused"]))
def test_refused_neighbour_lands_on_the_next_family(native, monkeypatch, c):
    fam = es.landing(c["refused"])
    assert c["family"] not in es._families(c["refused"])
    if fam == "abi":                                          # deeper than TBNN_MAX_LAYERS: no kernel at all, tbnn_create refuses it
        spec = o.make_spec(c["refused"], o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, o.ACT_NONE)
        with pytest.raises(native.TbnnError, match="n_layers"):
            native.Chain(layers_of(spec), likelihood=spec.likelihood, jit=True)
        return
    setenv(monkeypatch, fam, "")
    spec, X, Y, theta, eta = problem(c["refused"], N_WIDE if fam == "wide" else N_ROWS)
    value_gradient_forward(native, spec, X, Y, theta, eta, fam)


@pytest.mark.parametrize("c", REFUSED_BY_BUILD, ids=_id)
def test_build_refused_edge_lands_on_layered(native, monkeypatch, c):
    setenv(monkeypatch, c["family"], es.SKIP[c["family"]])
    assert es.landing(c["dims"]) == "layered"
    spec, X, Y, theta, eta = problem(c["dims"], N_ROWS)
    with pytest.warns(RuntimeWarning, match="layered"):
        value_gradient_forward(native, spec, X, Y, theta, eta, "layered")


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_admitted_edge_transitions_vs_oracle(native, monkeypatch, c):
    setenv(monkeypatch, c["family"], es.SKIP[c["family"]])
    spec, X, Y, theta, eta = problem(c["dims"], N_ROWS, c["lik"])
    rng = np.random.default_rng(sum(c["dims"]))
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    eps, L = 2e-5, 3
    ch = native.Chain(layers_of(spec), likelihood=spec.likelihood, fixed_sd=spec.fixed_sd, seed=50, chain_id=2, jit=True)
    try:
        name = ch.kernel_name
        assert name.startswith(PREFIX[c["family"]]), f"{c['family']}: runs on {name}"
        ch.set_data(X, Y)
        lp64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[0]
        worst = 0.0
        for log_u in (-1e30, 1e30):                          # an accept and a reject
            outs = []
            for _ in range(3):
                ch.set_state(theta); ch.set_hypers(eta)
                out = ch.hmc_step(eps, L, p0=p0, log_u=log_u)
                outs.append((out["log_accept_ratio"], out["logp_new"], ch.get_state()))
            assert all(x[0] == outs[0][0] and x[1] == outs[0][1] and np.array_equal(x[2], outs[0][2]) for x in outs), \
                f"{name}: a repeated transition differs"
            ref = o.weight_step(spec, theta, eta, X, Y, eps, L, p0, log_u, np.float64)
            d = abs(out["log_accept_ratio"] - ref.log_accept_ratio)
            worst = max(worst, d)
            tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
            assert d <= tol, (name, out["log_accept_ratio"], ref.log_accept_ratio, tol)
            assert bool(out["accepted"]) == ref.accepted, name
            assert np.abs(ch.get_state() - ref.theta).max() <= 1e-5 * max(1.0, np.abs(ref.theta).max()), name
        ph = rng.standard_normal(spec.n_hypers).astype(np.float32)
        ch.set_state(theta); ch.set_hypers(eta)
        ch.logp_grad(theta, eta)                             # the cached statistic the hyper target uses
        out = ch.hyper_step(1e-4, 9, p0=ph, log_u=-1e30)
        ref = o.hyper_step(spec, eta, theta, X, Y, 1e-4, 9, ph, -1e30, np.float64)
        assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= 2e-2 + 1e-3 * abs(ref.log_accept_ratio), name
        assert np.allclose(ch.get_hypers(), ref.theta, rtol=1e-4, atol=1e-5), name
        print(f"{name}: transition |d log accept ratio| {worst:.2e}, hyper {abs(out['log_accept_ratio'] - ref.log_accept_ratio):.2e}")
    finally:
        ch.close()
