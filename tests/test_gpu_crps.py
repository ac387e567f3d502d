"""GPU: the continuous ranked probability score of the predictive mixture over an ensemble (tbnn_ensemble_crps, Chain.ensemble_crps,
predictor.crps) against the 40-digit restatement of its definition (tests/crps_ref.py: ref40) applied to the fp32 predictions
Chain.forward_many returns for the same thetas and rows.  The forward kernels are shared, so both sides start from the same bits and the
tests isolate the pair kernel.  Every test here fails without the entry point (Chain.ensemble_crps does not exist before this module's
feature).

Networks: tiny tanh ones, 2-8-1, 2-8-3 and, for the heteroscedastic kind, 2-8-2, on the default kernel family and under KERNEL_GENERIC.
With T = ENS_CT = 8 the kernel's network tile and E = ENS_CE = 32 its elements per workgroup, the shapes are m in {1, 2, 3, T - 1, T, T + 1,
2 T + 1} crossed with rows in {1, E - 1, E + 1, 517} on both families (the largest case spends three seconds on its 40-digit reference);
every kind and option at m = T + 1 over E + 1 rows on both families.

The band.  Per element and for each of crps, error and spread:  |gpu - ref40| <= K 2^-53 (error_ref + spread_ref),  K = 64.
K is 8 x the worst deviation of the plain fp64 NumPy restatement (crps_ref.crps_np) from ref40 on these same cases -- 4.10 of that unit, as
tests/test_crps_host.py::test_fp64_restatement_against_40_digits prints it -- rounded up to a power of two: 8 x 4.10 = 32.8 -> 64.  The
margin covers the device's erf and exp against libm's and the different order of the sums.  No element is left out of the comparison; the
NaN cases are compared as NaN patterns."""
import ctypes as C

import numpy as np
import pytest

import crps_ref as cr
from crps_ref import E, FIXED, FIXED_SD, GAUSS, HETERO, T
from tensor_checks import layers_of

pytestmark = pytest.mark.gpu

K = 64
KEYS = ("crps", "error", "spread")


def make(native, kind, m, rows, generic, handle_lik=None, seed=None):
    spec, X, thetas = cr.case_problem(kind, m, rows, seed)
    ch = native.Chain(layers_of(spec), likelihood=kind if handle_lik is None else handle_lik, fixed_sd=FIXED_SD,
                      kernel=native.KERNEL_GENERIC if generic else native.KERNEL_AUTO)
    return ch, X, thetas


def bits_equal(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in KEYS)


def check_band(tag, got, f, Y, kind, noise, sd, w):
    """every element of all three outputs within the band of the 40-digit reference; returns the worst deviation in its unit"""
    m, d_out, n = f.shape
    od = 1 if kind == HETERO else d_out
    for k in KEYS:
        assert got[k].shape == (od, n) and got[k].dtype == np.float64, (tag, k, got[k].shape)
        assert np.all(np.isfinite(got[k])), (tag, k)
    r40, _rnp = cr.case_reference(f, Y, kind, noise, sd, w)
    dev = cr.deviation_u([got[k].reshape(-1) for k in KEYS], r40)
    worst = float(dev.max())
    print(f"[crps] {tag}: m={m} rows={n} worst deviation {worst:.2f} u (crps {dev[0].max():.2f}, error {dev[1].max():.2f}, spread {dev[2].max():.2f}; K {K})")
    assert worst <= K, (tag, worst)
    assert np.all(got["crps"] >= 0)
    return worst


# ------------------------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])
@pytest.mark.parametrize("rows", cr.SHAPE_ROWS)
@pytest.mark.parametrize("m", cr.SHAPE_M)
def test_shapes(native, m, rows, generic):
    """one network to two tiles and one, one element to several workgroups and a partial one; per-network sd's over two decades, weighted
    (some weights 0) at every second row count"""
    kind, _m, _rows, noise, weighted = next(c for c in cr.shape_cases() if c[1] == m and c[2] == rows)
    ch, X, thetas = make(native, kind, m, rows, generic)
    f = ch.forward_many(thetas, X=X)
    Y = cr.case_targets(f, kind, seed=m + rows)
    sd, w = cr.sds(m), cr.weights_with_zeros(m) if weighted else None
    got = ch.ensemble_crps(thetas, Y=Y, X=X, likelihood=GAUSS, sd=sd, weights=w)
    check_band(f"shapes {'generic' if generic else 'default'} ({ch.kernel_name})", got, f, Y, kind, noise, sd, w)
    ch.close()


# ------------------------------------------------------------------------------------------------------------------- kinds and options
@pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])
@pytest.mark.parametrize("weighted", [False, True], ids=["equal", "weighted"])
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "no_noise"])
@pytest.mark.parametrize("which", ["gaussian", "fixed_own", "fixed_other", "hetero"])
def test_kinds_and_options(native, which, noise, weighted, generic):
    """TBNN_LIK_GAUSSIAN with per-network sd (three outputs); TBNN_LIK_FIXED_GAUSSIAN with the handle's fixed_sd, on a handle of its own and
    on one of another likelihood; the heteroscedastic kind (one plane from two outputs).  Without noise sd is not read: a NaN there is not
    refused.  Two calls give the same bits."""
    kind = {"gaussian": GAUSS, "fixed_own": FIXED, "fixed_other": FIXED, "hetero": HETERO}[which]
    m, rows = T + 1, E + 1
    ch, X, thetas = make(native, kind, m, rows, generic, handle_lik=GAUSS if which == "fixed_other" else None)
    f = ch.forward_many(thetas, X=X)
    Y = cr.case_targets(f, kind, seed=m + rows)
    w = cr.weights_with_zeros(m) if weighted else None
    ref_sd = cr.sds(m) if which == "gaussian" else np.full(m, np.float32(FIXED_SD))
    sd = ref_sd if which == "gaussian" else None
    if which == "gaussian" and not noise:
        sd = np.full(m, np.nan, dtype=np.float32)
    kw = dict(Y=Y, X=X, likelihood=kind, sd=sd, weights=w, noise=noise)
    got = ch.ensemble_crps(thetas, **kw)
    check_band(f"{which} noise={noise} weighted={weighted} {'generic' if generic else 'default'}", got, f, Y, kind, noise, ref_sd, w)
    assert bits_equal(got, ch.ensemble_crps(thetas, **kw))
    if not noise:
        srt = cr.crps_sorted(f[:, 0].astype(np.float64), w, Y.reshape(rows, -1)[:, 0].astype(np.float64))
        assert np.allclose(got["crps"][0], srt[0], rtol=1e-12, atol=1e-13)
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------------- edges
def test_sd_at_both_clips(native):
    """sd below 1e-8 and above 1e8 is clipped in fp32 as tbnn_ensemble_loglik clips it"""
    m, rows = 5, E + 1
    ch, X, thetas = make(native, FIXED, m, rows, False, seed=11)
    f = ch.forward_many(thetas, X=X)
    Y = cr.case_targets(f, FIXED, seed=12)
    sd = np.array([1e-9, 1e9, 0.5, 1e-8, 1e8], dtype=np.float32)
    got = ch.ensemble_crps(thetas, Y=Y, X=X, sd=sd)
    check_band("sd at both clips", got, f, Y, FIXED, True, sd, None)
    # the small scales alone: the clipped 1e-9 gives the bits of 1e-8
    a = ch.ensemble_crps(thetas, Y=Y, X=X, sd=np.array([1e-9, 0.3, 0.5, 0, 0.1], dtype=np.float32))
    b = ch.ensemble_crps(thetas, Y=Y, X=X, sd=np.array([1e-8, 0.3, 0.5, 1e-8, 0.1], dtype=np.float32))
    assert bits_equal(a, b)
    check_band("sd at the lower clip", a, f, Y, FIXED, True, np.array([1e-8, 0.3, 0.5, 1e-8, 0.1], dtype=np.float32), None)
    ch.close()


def test_all_networks_equal(native):
    """m copies of one network: the mixture is one Gaussian and spread = s / sqrt pi per element"""
    m, rows = T + 1, E + 1
    ch, X, thetas = make(native, FIXED, 1, rows, False, seed=21)
    thetas = np.repeat(thetas, m, axis=0)
    f = ch.forward_many(thetas, X=X)
    assert all(np.array_equal(f[0], f[i]) for i in range(m))
    Y = cr.case_targets(f, FIXED, seed=22)
    sd = np.full(m, np.float32(FIXED_SD))
    for w in (None, cr.weights_with_zeros(m)):
        got = ch.ensemble_crps(thetas, Y=Y, X=X, weights=w)
        check_band("all networks equal", got, f, Y, FIXED, True, sd, w)
        want = float(np.float32(FIXED_SD)) / np.sqrt(np.pi)
        assert np.all(np.abs(got["spread"] - want) <= K * cr.U * (got["error"] + want))
    none = ch.ensemble_crps(thetas, Y=Y, X=X, noise=False)
    assert not none["spread"].any() and np.array_equal(none["crps"], none["error"])
    assert np.all(np.abs(none["error"] - np.abs(Y.T.astype(np.float64) - f[0].astype(np.float64))) <= K * cr.U * none["error"])
    ch.close()


def test_targets_a_million_scales_away(native):
    m, rows = T + 1, E + 1
    ch, X, thetas = make(native, FIXED, m, rows, False, seed=31)
    f = ch.forward_many(thetas, X=X)
    sd = cr.sds(m)
    sign = np.where(np.arange(rows) % 2, -1.0, 1.0)
    Y = (f[0, 0].astype(np.float64) + sign * 1e6 * float(sd.max())).astype(np.float32)[:, None]
    for noise in (True, False):
        got = ch.ensemble_crps(thetas, Y=Y, X=X, sd=sd, noise=noise)
        check_band(f"targets 1e6 scales away, noise={noise}", got, f, Y, FIXED, noise, sd, None)
    ch.close()


def test_hetero_log_sd_beyond_the_clip(native):
    """g above log(1e8) and below -log(1e8) is read at the clip, as the likelihood reads it"""
    m, rows = 5, E + 1
    ch, X, thetas = make(native, HETERO, m, rows, False, seed=41)
    thetas[0, -1], thetas[1, -1] = 40.0, -40.0                # (theta ends with the last layer's biases: the log-sd output's is the last)
    f = ch.forward_many(thetas, X=X)
    assert f[0, 1].min() > cr.LOG_CLIP + 1 and f[1, 1].max() < -cr.LOG_CLIP - 1
    Y = cr.case_targets(f, HETERO, seed=42)
    for w in (None, np.array([0, 1, 2, 1, 1], dtype=np.float32)):
        got = ch.ensemble_crps(thetas, Y=Y, X=X, weights=w)
        check_band("hetero g beyond the clip", got, f, Y, HETERO, True, None, w)
    ch.close()


@pytest.mark.parametrize("kind", [GAUSS, HETERO], ids=["gaussian", "hetero"])
def test_nan_and_inf_predictions(native, kind):
    """a NaN input row: that row's elements alone.  A network whose predictions are all NaN or +-inf: under a network that counts every
    element is NaN; under one of weight 0 an infinity changes nothing, and a NaN makes the element NaN for the Gaussian kinds (whatever
    the weight) and is not looked at by the heteroscedastic kind"""
    m, rows = T + 1, E + 1
    ch, X, thetas = make(native, kind, m, rows, False, seed=51)
    d_out = cr.DIMS[kind][-1]
    f = ch.forward_many(thetas, X=X)
    Y = cr.case_targets(f, kind, seed=52)
    w = cr.weights_with_zeros(m)
    assert w[1] == 0 and w[0] > 0
    sd = cr.sds(m) if kind == GAUSS else None
    kw = dict(Y=Y, X=X, sd=sd, weights=w)
    clean = ch.ensemble_crps(thetas, **kw)
    Xn = X.copy()
    Xn[7, 0] = np.nan
    assert np.isnan(ch.forward_many(thetas, X=Xn)[:, :, 7]).all()
    got = ch.ensemble_crps(thetas, **dict(kw, X=Xn))
    for k in KEYS:
        bad = np.zeros_like(got[k], dtype=bool)
        bad[:, 7] = True
        assert np.array_equal(np.isnan(got[k]), bad), k
        assert np.array_equal(got[k][~bad].view(np.uint64), clean[k][~bad].view(np.uint64)), k
    mean_bias = -d_out                                          # (theta ends with the last layer's biases; output 0 is the mean everywhere)
    for value in (np.nan, np.inf, -np.inf):
        for net, counts in ((0, True), (1, False)):
            th = thetas.copy()
            th[net, mean_bias] = value
            fm = ch.forward_many(th, X=X)
            assert (np.isnan(fm[net, 0]).all() if np.isnan(value) else np.all(fm[net, 0] == value)) and np.isfinite(np.delete(fm, net, axis=0)).all()
            got = ch.ensemble_crps(th, **kw)
            every = counts or (np.isnan(value) and kind == GAUSS)
            for k in KEYS:
                if kind == GAUSS and every:
                    # (three outputs: output 0 alone holds the value)
                    assert np.isnan(got[k][0]).all() and np.array_equal(got[k][1:].view(np.uint64), clean[k][1:].view(np.uint64)), (value, net, k)
                elif every:
                    assert np.isnan(got[k]).all(), (value, net, k)
                else:
                    assert np.array_equal(got[k].view(np.uint64), clean[k].view(np.uint64)), (value, net, k)
    if kind == HETERO:
        # the log-sd output alone: NaN under a network that counts, not looked at under weight 0, and not read at all without noise
        for net, counts in ((0, True), (1, False)):
            th = thetas.copy()
            th[net, -1] = np.nan
            fm = ch.forward_many(th, X=X)
            assert np.isnan(fm[net, 1]).all() and np.isfinite(fm[net, 0]).all()
            got = ch.ensemble_crps(th, **kw)
            assert all(np.isnan(got[k]).all() for k in KEYS) if counts else bits_equal(got, clean)
            assert bits_equal(ch.ensemble_crps(th, **dict(kw, noise=False)), ch.ensemble_crps(thetas, **dict(kw, noise=False)))
    ch.close()


def test_nan_target(native):
    m, rows = 3, E + 1
    ch, X, thetas = make(native, GAUSS, m, rows, False, seed=61)
    f = ch.forward_many(thetas, X=X)
    Y = cr.case_targets(f, GAUSS, seed=62)
    sd = cr.sds(m)
    clean = ch.ensemble_crps(thetas, Y=Y, X=X, sd=sd)
    Y[3, 1] = np.nan
    for noise in (True, False):
        got = ch.ensemble_crps(thetas, Y=Y, X=X, sd=sd, noise=noise)
        for k in KEYS:
            bad = np.zeros_like(got[k], dtype=bool)
            bad[1, 3] = True
            assert np.array_equal(np.isnan(got[k]), bad), k
            if noise:
                assert np.array_equal(got[k][~bad].view(np.uint64), clean[k][~bad].view(np.uint64)), k
    ch.close()


def test_each_output_alone(native):
    """any of the three pointers may be NULL: each alone gives the bits of the three together, and the others are not written"""
    m, rows = T + 1, E + 1
    ch, X, thetas = make(native, GAUSS, m, rows, False, seed=71)
    f = ch.forward_many(thetas, X=X)
    Y = np.ascontiguousarray(cr.case_targets(f, GAUSS, seed=72))
    sd = cr.sds(m)
    all3 = ch.ensemble_crps(thetas, Y=Y, X=X, sd=sd)
    Xc = np.ascontiguousarray(X, dtype=np.float32)
    for alone in range(3):
        outs = [np.full((3, rows), 7.0) for _ in range(3)]
        ptrs = [native._pd(outs[k]) if k == alone else None for k in range(3)]
        rc = native.lib.tbnn_ensemble_crps(ch._h, native._p(thetas), m, thetas.shape[1], GAUSS, native._p(sd), None, 1, native._p(Xc),
                                           native._p(Y), rows, 1, *ptrs)
        assert rc == 0, native.lib.tbnn_last_error()
        assert np.array_equal(outs[alone].view(np.uint64), all3[KEYS[alone]].view(np.uint64))
        assert all(np.all(outs[k] == 7.0) for k in range(3) if k != alone)
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------- determinism
def test_row_blocks(native, monkeypatch):
    """517 rows in blocks of 192: three blocks, the last of 133 rows (the driver's rule: rb = floor(budget / (m d_out)) rounded down to a
    multiple of 64).  The generic kernel runs a row per thread, so a row's forward bits do not depend on its block; all three outputs are
    bit for bit those of the single-block call, with and without noise, and so are those over the staged rows and targets"""
    for kind in (GAUSS, HETERO):
        m, rows, rb = T + 1, 517, 192
        ch, X, thetas = make(native, kind, m, rows, True, seed=81)
        d_out = cr.DIMS[kind][-1]
        f = ch.forward_many(thetas, X=X)
        Y = cr.case_targets(f, kind, seed=82)
        w = cr.weights_with_zeros(m)
        calls = [dict(sd=cr.sds(m) if kind == GAUSS else None, weights=w, noise=noise) for noise in (True, False)]
        whole = [ch.ensemble_crps(thetas, Y=Y, X=X, **kw) for kw in calls]
        budget = m * d_out * rb + 7
        assert max(64, budget // (m * d_out) // 64 * 64) == rb and -(-rows // rb) == 3
        monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
        cut = [ch.ensemble_crps(thetas, Y=Y, X=X, **kw) for kw in calls]
        ch.set_data(X, Y)
        staged = [ch.ensemble_crps(thetas, which=0, **kw) for kw in calls]
        monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
        for a, b, c in zip(whole, cut, staged):
            assert bits_equal(a, b) and bits_equal(a, c), kind
        ch.close()


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_usable(native):
    dp = C.POINTER(C.c_double)
    m = 4
    ch, X, thetas = make(native, FIXED, m, E + 1, False, seed=91)
    n, Pn = X.shape[0], thetas.shape[1]
    lib, p = native.lib, native._p
    Xc = np.ascontiguousarray(X, dtype=np.float32)
    Y = np.ones((n, 1), dtype=np.float32)
    before = ch.forward_many(thetas, X=X)
    outs = [np.full((1, n), 7.0) for _ in range(3)]

    def call(lik=FIXED, sd=None, w=None, which=1, X_=Xc, Y_=Y, n_=n, noise=1, stride=Pn, m_=m, o=(True, True, True), h=None):
        return lib.tbnn_ensemble_crps(ch._h if h is None else h, p(thetas), m_, stride, lik, p(sd), p(w), which, p(X_), p(Y_), n_, noise,
                                      *[outs[k].ctypes.data_as(dp) if o[k] else None for k in range(3)])

    f32 = lambda *v: np.array(v, dtype=np.float32)
    err = lambda: lib.tbnn_last_error().decode()
    assert call(o=(False, False, False)) < 0 and err() == "ensemble_crps: every output is null"
    assert call(Y_=None) < 0 and err() == "ensemble_crps: rows X without their targets Y"
    for bad in (2, -1):
        assert call(noise=bad) < 0 and err() == "ensemble_crps: noise must be 0 (the networks' outputs alone) or 1 (with the observation noise)"
    for lik in (native.LIK_BERNOULLI, native.LIK_CATEGORICAL):
        assert call(lik=lik) < 0 and "tbnn_ensemble_uncertainty" in err() and "a label" in err()
    for lik in (native.LIK_POISSON, native.LIK_NEG_BINOMIAL):
        assert call(lik=lik) < 0 and "count distribution is not built" in err() and "no closed form" in err()
    assert call(lik=native.LIK_STUDENT_T) < 0 and "TBNN_LIK_STUDENT_T is not built" in err() and "no closed form" in err()
    assert call(lik=4) < 0 and err() == "ensemble_crps: unknown likelihood"
    assert call(lik=HETERO) < 0 and err() == "ensemble_crps: the heteroscedastic Gaussian likelihood needs exactly 2 outputs: mean and log-sd"
    assert call(m_=4097) < 0 and err() == "ensemble_crps: m = 4097 exceeds 4096 networks (the work is quadratic in m)"
    assert call(m_=0) < 0 and "m < 1" in err()
    assert call(w=f32(1, -1, 1, 1)) < 0 and "negative" in err()
    assert call(w=f32(0, 0, 0, 0)) < 0 and "all weights are zero" in err()
    assert call(w=f32(1, np.nan, 1, 1)) < 0 and "not finite" in err()
    assert call(sd=f32(1, np.nan, 1, 1)) < 0 and "not a number" in err()
    assert call(stride=Pn - 1) < 0 and "theta_stride < P" in err()
    assert call(X_=None, n_=0, which=1) < 0 and "tbnn_set_validation has not been called" in err()
    assert call(X_=None, n_=0, which=2) < 0 and "which must be" in err()
    assert call(X_=Xc, n_=0) < 0 and "n < 1" in err()
    ch.set_data(X, Y)
    assert call(X_=None, n_=n - 1, which=0) < 0 and "does not match" in err()
    assert call(h=None, m_=m, lik=FIXED, o=(True, True, True), noise=1) == 0
    assert lib.tbnn_ensemble_crps(None, p(thetas), m, Pn, FIXED, None, None, 1, p(Xc), p(Y), n, 1, *[o_.ctypes.data_as(dp) for o_ in outs]) < 0
    outs2 = [o_.copy() for o_ in outs]
    for o_ in outs:
        o_[:] = 7.0
    for args in (dict(o=(False, False, False)), dict(noise=2), dict(lik=native.LIK_POISSON), dict(m_=4097), dict(sd=f32(1, np.nan, 1, 1))):
        assert call(**args) < 0
    assert all(np.all(o_ == 7.0) for o_ in outs)                                         # nothing written
    with pytest.raises(native.TbnnError, match="tbnn_ensemble_uncertainty"):
        ch.ensemble_crps(thetas, Y=Y, X=X, likelihood=native.LIK_BERNOULLI)
    with pytest.raises(ValueError, match="targets"):
        ch.ensemble_crps(thetas, X=X)
    assert call(sd=f32(1, np.nan, 1, 1), noise=0) == 0                                    # without noise sd is not read
    again = ch.ensemble_crps(thetas, Y=Y, X=X)
    assert all(np.array_equal(again[k], outs2[i]) for i, k in enumerate(KEYS))
    assert np.array_equal(ch.forward_many(thetas, X=X), before)
    ch.close()


# ---------------------------------------------------------------------------------------------------------------- predictor, end to end
def test_predictor_end_to_end(tmp_path, monkeypatch, native):
    """a small noisy regression trained for a few epochs under a GaussianLikelihood whose sd is sampled: predictor.crps over the saved
    networks with their saved sd's against the 40-digit reference on predictor.predict's output, its summary fields, and compareCrps"""
    from tensorbnn_amd.activationFunctions import Tanh
    from tensorbnn_amd.layer import DenseLayer
    from tensorbnn_amd.likelihood import BernoulliLikelihood, GaussianLikelihood
    from tensorbnn_amd.network import network
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(71)
    X = rng.uniform(-2, 2, (120, 1)).astype(np.float32)
    Y = (np.sin(2 * X) + 0.3 * rng.standard_normal(X.shape)).astype(np.float32)
    net = network(np.float32, 1, X, Y, X[:50], Y[:50])
    net.add(DenseLayer(1, 8, seed=1000)); net.add(Tanh())
    net.add(DenseLayer(8, 1, seed=3000))
    net.setupMCMC(stepSizeStart=1e-3, stepSizeMin=1e-4, stepSizeMax=5e-3, stepSizeOptions=10, leapfrogStart=20, leapfogMin=10,
                  leapFrogMax=40, leapfrogIncrement=10, hyperStepSize=1e-3, hyperLeapfrog=10, burnin=10, averagingSteps=2, randomSteps=2)
    net.train(30, 2, GaussianLikelihood(sd=0.5), folderName="reg", networksPerFile=1, verbose=False)
    p = predictor(str(tmp_path / "reg") + "/", likelihood=GaussianLikelihood(sd=0.5))
    m = p.numNetworks
    assert m >= 4 and len(p.hypers) == m
    f = np.array(p.predict(X)).astype(np.float32)
    sd = np.array([np.float32(h[-1]) for h in p.hypers], dtype=np.float32)
    res = p.crps(X, Y)
    check_band("predictor", res, f, Y, GAUSS, True, sd, None)
    s = predictor._crps_summary(res["crps"])
    assert res["n_bad"] == 0 and np.array_equal(res["mean_crps"], s["mean_crps"]) and np.array_equal(res["se"], s["se"])
    assert res["mean_crps"].shape == (1,) and res["mean_crps"][0] == res["crps"][0].mean() and res["se"][0] > 0
    # every second network, reweighted; and the networks' outputs alone
    w = np.arange(1, len(range(0, m, 2)) + 1, dtype=np.float32)
    res2 = p.crps(X, Y, n=2, weights=w)
    check_band("predictor, every second network", res2, f[::2], Y, GAUSS, True, sd[::2], w)
    bare = p.crps(X, Y, noise=False)
    check_band("predictor, no noise", bare, f, Y, GAUSS, False, sd, None)
    c = predictor.compareCrps(res, bare)
    d = res["crps"][0] - bare["crps"][0]
    assert c["crps_diff"][0] == d.mean() and c["se_diff"][0] == np.sqrt(np.var(d, ddof=1) / d.size)
    Yn = Y.copy()
    Yn[5] = np.nan
    resn = p.crps(X, Yn)
    assert resn["n_bad"] == 1 and resn["mean_crps"][0] == np.delete(resn["crps"][0], 5).mean()
    with pytest.raises(ValueError, match="label"):
        p.crps(X, Y, likelihood=BernoulliLikelihood())
