"""GPU: split-R-hat and effective sample size over an ensemble's network axis read as chains x draws (tbnn_ensemble_diagnostics /
tbnn_series_diagnostics, Chain.ensemble_diagnostics / series_diagnostics, predictor.fromChains / predictDiagnostics / parameterDiagnostics)
against tests/diag_ref.py, the fp64 NumPy restatement of the definition in include/tbnn.h, applied to the device's own fp32 values.  Every
test here fails without the entry points (they do not exist before this module's feature).

Where the values come from.  No transform: Chain.forward_many of the same thetas and rows -- the forward kernels are shared, so both sides
see the same bits.  Scale and shift: the same predictions, t = fma(f, scale, shift) rounded to fp32 on the host (the device's one
v_fma_f32; formed in fp64, where the product of two fp32 values is exact).  exp / sigmoid / softmax: the device's own t, read back one
network at a time through Chain.ensemble_moments -- the mean of ONE network is its t, converted exactly -- and the smallest case checks
that these are the values k_ens_transform writes (their sorted order against the inverted-CDF quantiles, which return the t themselves).

Comparison rule.  R-hat is a continuous function of fp64 sums; the ESS is continuous except at the sign decision of a Geyer pair P_k.
diag_ref returns each element's margin, the smallest |P_k| it met up to and including its stop; elements with a margin below MARGIN may
be left out, at most 1 % of a case (asserted; the inputs here leave out none: the smallest margin printed is far above MARGIN).  What is
left differs by the order of fp64 sums and by fused multiply-adds only.  RTOL is 16 x the largest relative difference measured over all
cases of this module on an MI355X -- 3.538e-15, the ESS of one coordinate in test_series_of_the_thetas_themselves (R-hat: 4.692e-16);
DESIGN.md section 4.6 records the figure -- and never above 1e-8: a larger gap would mean a formula differs, not rounding."""
import ctypes as C
import math

import numpy as np
import pytest

from diag_ref import diag_ref
from test_gpu_ensemble import CASES, layers_for, make_chain

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
RTOL = min(16 * 3.538e-15, 1e-8)
ACT_TANH = 2
GEN3 = [5, 16, 16, 3]                                        # three outputs on the generic kernel; CASES["narrow"]: one output, fast3
ROWS = 70                                                    # one ragged wavefront per output


def gen3_chain(native):
    ch = native.Chain(layers_for(GEN3, ACT_TANH, 0), likelihood=1, fixed_sd=0.7, kernel=native.KERNEL_GENERIC)
    assert ch.kernel_name == "generic" and ch.d_out == 3
    return ch


def chain_for(native, name):
    return gen3_chain(native) if name == "gen3" else make_chain(native, name)


def rows_for(name, n=ROWS, seed=0):
    d_in = GEN3[0] if name == "gen3" else CASES[name][0][0]
    return (np.random.default_rng(seed).standard_normal((n, d_in)) / math.sqrt(max(d_in / 16.0, 1.0))).astype(np.float32)


def walks(P, Cn, S, seed=0, offset=0.0):
    """thetas [Cn S, P], chain-major: AR(1) walks of small steps around one base vector, phi rising from 0 to 0.9 over the chains, so the
    predictions carry real autocorrelation; offset moves the LAST chain's walk away from the others' (R-hat well above 1)"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(P) * 0.35
    out = np.empty((Cn, S, P))
    for c in range(Cn):
        phi = 0.9 * c / max(Cn - 1, 1) if Cn > 1 else 0.6
        dev = rng.standard_normal(P)
        for s in range(S):
            dev = phi * dev + math.sqrt(1 - phi * phi) * rng.standard_normal(P)
            out[c, s] = base + 0.03 * dev
    if offset:
        out[-1] += offset * rng.standard_normal(P)
    return out.reshape(Cn * S, P).astype(np.float32)


def fma32(f, scale, shift):
    return (f.astype(np.float64) * np.float64(np.float32(scale)) + np.float64(np.float32(shift))).astype(np.float32)


def device_t(ch, thetas, X, xform, scale, shift):
    """the device's transformed values [m, d_out, rows], one network at a time (module docstring)"""
    t = np.stack([ch.ensemble_moments(thetas[i:i + 1], X=X, xform=xform, scale=scale, shift=shift, var=False)[0] for i in range(thetas.shape[0])])
    assert np.array_equal(t, t.astype(np.float32).astype(np.float64))
    return t.astype(np.float32)


def compare(tag, got, t, Cn):
    """got = (rhat, ess) against diag_ref(t); prints the figures, then asserts the module docstring's rule.  Returns the largest relative
    difference."""
    rhat, ess, margin = diag_ref(t, Cn)
    assert got[0].shape == rhat.shape and got[1].shape == ess.shape and got[0].dtype == got[1].dtype == np.float64
    und = np.isnan(rhat)
    assert np.array_equal(np.isnan(got[0]), und) and np.array_equal(np.isnan(got[1]), und), tag
    keep = ~und & (margin >= MARGIN)
    left = int((~und & ~keep).sum())
    dr = np.abs(got[0] - rhat)[~und] / rhat[~und]
    de = np.abs(got[1] - ess)[keep] / ess[keep]
    worst = max(float(dr.max(initial=0.0)), float(de.max(initial=0.0)))
    print(f"[diagnostics] {tag}: C={Cn} S={t.shape[0] // Cn} elements {rhat.size} (undefined {int(und.sum())}, left out {left}), rhat "
          f"{np.nanmin(rhat):.3f} .. {np.nanmax(rhat):.3f}, ess {np.nanmin(ess):.1f} .. {np.nanmax(ess):.1f}, smallest margin "
          f"{margin.min():.3e}, rel diff rhat {dr.max(initial=0.0):.3e} ess {de.max(initial=0.0):.3e}")
    assert left <= 0.01 * rhat.size, (tag, left)
    assert worst <= RTOL, (tag, worst)
    return worst


# --------------------------------------------------------------------------------------------------------------------- smallest cases
@pytest.mark.parametrize("name,Cn,S,xform,scale,shift,offset", [
    ("narrow", 1, 8, "none", 1.0, 0.0, 0.0), ("narrow", 3, 9, "none", 1.7, -0.3, 0.0), ("narrow", 4, 64, "none", 1.0, 0.0, 0.0),
    ("narrow", 4, 64, "none", 1.0, 0.0, 0.06), ("narrow", 3, 9, "exp", 1.0, 0.0, 0.0), ("narrow", 4, 64, "sigmoid", -1.7, 0.3, 0.03),
    ("gen3", 1, 8, "softmax", 1.0, 0.0, 0.0), ("gen3", 3, 9, "softmax", 1.0, 0.0, 0.03), ("gen3", 4, 64, "softmax", 1.7, -0.3, 0.0),
    ("gen3", 4, 64, "none", 1.0, 0.0, 0.06)])
def test_against_the_restatement(native, name, Cn, S, xform, scale, shift, offset):
    """one chain of 8 (N = 4: lags 0 .. 3), three chains of 9 (odd: the middle draw dropped), four chains of 64 (N = 32: four batches of
    lags); one output on the narrow MFMA kernels, three on the generic kernel with the softmax; 70 rows"""
    code = {"none": native.XFORM_NONE, "exp": native.XFORM_EXP, "sigmoid": native.XFORM_SIGMOID, "softmax": native.XFORM_SOFTMAX}[xform]
    ch = chain_for(native, name)
    X = rows_for(name)
    thetas = walks(ch.P, Cn, S, seed=Cn * 100 + S, offset=offset)
    f = ch.forward_many(thetas, X=X)
    t = f if (scale, shift) == (1.0, 0.0) else fma32(f, scale, shift)
    if xform != "none":
        t = device_t(ch, thetas, X, code, scale, shift)
        if S == 8 or xform == "exp":                        # the t read back are the t the transform kernel writes (m <= 27 probabilities)
            m = Cn * S
            probs = [(i + 1) / m for i in range(m)]
            assert np.array_equal(ch.ensemble_quantiles(thetas, probs, X=X, method="inverted_cdf", xform=code, scale=scale, shift=shift),
                                  np.quantile(t.astype(np.float64), probs, axis=0, method="inverted_cdf"))
    got = ch.ensemble_diagnostics(thetas, chains=Cn, X=X, xform=code, scale=scale, shift=shift)
    compare(f"{name} {xform} x{scale}+{shift} offset {offset}", got, t, Cn)
    if offset >= 0.06:
        assert np.nanmax(got[0]) > 1.5                      # a chain apart is seen
    ch.close()


def test_rhat_alone_and_ess_alone(native):
    """either output may be NULL: the other is unchanged"""
    dp = C.POINTER(C.c_double)
    ch = make_chain(native, "narrow")
    X = rows_for("narrow")
    thetas = walks(ch.P, 2, 16, seed=3)
    rhat, ess = ch.ensemble_diagnostics(thetas, chains=2, X=X)
    one = np.full((1, ROWS), 7.0)
    args = (ch._h, native._p(thetas), 32, thetas.shape[1], 2, 0, 1.0, 0.0, 1, native._p(X), ROWS)
    assert native.lib.tbnn_ensemble_diagnostics(*args, one.ctypes.data_as(dp), None) == 0 and np.array_equal(one, rhat)
    assert native.lib.tbnn_ensemble_diagnostics(*args, None, one.ctypes.data_as(dp)) == 0 and np.array_equal(one, ess)
    sr = np.ascontiguousarray(thetas[:, :5])
    r5, e5 = ch.series_diagnostics(sr, chains=2)
    one = np.full(5, 7.0)
    assert native.lib.tbnn_series_diagnostics(ch._h, native._p(sr), 32, 5, 2, one.ctypes.data_as(dp), None) == 0 and np.array_equal(one, r5)
    assert native.lib.tbnn_series_diagnostics(ch._h, native._p(sr), 32, 5, 2, None, one.ctypes.data_as(dp)) == 0 and np.array_equal(one, e5)
    ch.close()


# --------------------------------------------------------------------------------------------------------------------------- row blocks
@pytest.mark.parametrize("name,xform", [("narrow", "none"), ("gen3", "softmax")])
def test_row_blocks(native, monkeypatch, name, xform):
    """130 rows in blocks of 64, 64 and 2 (the driver's rule: floor(budget / (m d_out)) rounded down to a multiple of 64): the bits of the
    unblocked call, and the staged rows give the bits of the explicit X"""
    code = native.XFORM_SOFTMAX if xform == "softmax" else native.XFORM_NONE
    ch = chain_for(native, name)
    n, Cn, S = 130, 2, 12
    X = rows_for(name, n=n, seed=1)
    thetas = walks(ch.P, Cn, S, seed=5, offset=0.03)
    kw = dict(chains=Cn, xform=code, scale=1.7, shift=-0.3)
    whole = ch.ensemble_diagnostics(thetas, X=X, **kw)
    budget = Cn * S * ch.d_out * 64 + 5
    assert max(64, budget // (Cn * S * ch.d_out) // 64 * 64) == 64
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(budget))
    cut = ch.ensemble_diagnostics(thetas, X=X, **kw)
    for a, b in zip(whole, cut):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    ch.set_data(X, np.zeros((n, ch.d_out), dtype=np.float32))
    for a, b in zip(whole, ch.ensemble_diagnostics(thetas, which=0, **kw)):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    monkeypatch.delenv("TBNN_ENS_CHUNK_FLOATS")
    t = device_t(ch, thetas, X, code, 1.7, -0.3) if xform == "softmax" else fma32(ch.forward_many(thetas, X=X), 1.7, -0.3)
    compare(f"row blocks {name} {xform}", cut, t, Cn)
    ch.close()


# ---------------------------------------------------------------------------------------------------------------------------- stability
def test_two_calls_and_a_multi_chain_handle_return_the_same_bits(native):
    dp = C.POINTER(C.c_double)
    dims, act, last, lik, _prefix, _n = CASES["narrow"]
    ch = make_chain(native, "narrow")
    X = rows_for("narrow", n=333, seed=2)
    thetas = walks(ch.P, 4, 16, seed=7, offset=0.03)
    for kw in ({}, {"xform": native.XFORM_EXP, "scale": 1.7, "shift": -0.3}):
        a = ch.ensemble_diagnostics(thetas, chains=4, X=X, **kw)
        b = ch.ensemble_diagnostics(thetas, chains=4, X=X, **kw)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), kw
    grp = native.ChainGroup(layers_for(dims, act, last), 3, likelihood=lik)
    rhat, ess = np.empty((1, 333)), np.empty((1, 333))
    rc = native.lib.tbnn_ensemble_diagnostics(grp._h, native._p(thetas), 64, thetas.shape[1], 4, native.XFORM_EXP, 1.7, -0.3, 1, native._p(X), 333,
                                              rhat.ctypes.data_as(dp), ess.ctypes.data_as(dp))
    assert rc == 0, native.lib.tbnn_last_error()
    assert np.array_equal(rhat.view(np.uint64), a[0].view(np.uint64)) and np.array_equal(ess.view(np.uint64), a[1].view(np.uint64))
    sr = np.ascontiguousarray(thetas[:, :100])
    want = ch.series_diagnostics(sr, chains=4)
    r2, e2 = np.empty(100), np.empty(100)
    assert native.lib.tbnn_series_diagnostics(grp._h, native._p(sr), 64, 100, 4, r2.ctypes.data_as(dp), e2.ctypes.data_as(dp)) == 0
    assert np.array_equal(r2.view(np.uint64), want[0].view(np.uint64)) and np.array_equal(e2.view(np.uint64), want[1].view(np.uint64))
    ch.close(); grp.close()


# ------------------------------------------------------------------------------------------------------------------------------- series
@pytest.fixture(scope="module")
def series():
    """[64, 257]: four chains of 16, AR(1) per coordinate with phi spread over the coordinates, the last chain apart in every fourth"""
    rng = np.random.default_rng(11)
    phi = np.linspace(0.0, 0.9, 257)
    x = np.empty((4, 16, 257))
    x[:, 0] = rng.standard_normal((4, 257))
    for s in range(1, 16):
        x[:, s] = phi * x[:, s - 1] + np.sqrt(1 - phi * phi) * rng.standard_normal((4, 257))
    x[3, :, ::4] += 2.0
    return x.reshape(64, 257).astype(np.float32)


@pytest.mark.parametrize("tot", [1, 63, 257])
def test_series_against_the_restatement(native, series, tot):
    ch = gen3_chain(native)
    sr = series[:, :tot]
    compare(f"series tot={tot}", ch.series_diagnostics(sr, chains=4), sr, 4)
    if tot == 1:
        a = ch.series_diagnostics(sr[:, 0], chains=4)            # a vector is one coordinate
        assert a[0].shape == (1,) and np.array_equal(a[0], ch.series_diagnostics(sr, chains=4)[0])
    ch.close()


def test_series_column_blocks(native, series, monkeypatch):
    """257 columns in blocks of 64 (four and one column left): the bits of the unblocked call"""
    ch = gen3_chain(native)
    whole = ch.series_diagnostics(series, chains=4)
    monkeypatch.setenv("TBNN_ENS_CHUNK_FLOATS", str(64 * 64 + 5))
    for a, b in zip(whole, ch.series_diagnostics(series, chains=4)):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    ch.close()


def test_series_of_the_thetas_themselves(native):
    """every coordinate of four walks of 64 draws of the narrow network (5401 coordinates: more than one workgroup per launch of 4096)"""
    ch = make_chain(native, "narrow")
    thetas = walks(ch.P, 4, 64, seed=13, offset=0.05)
    compare("series of thetas", ch.series_diagnostics(thetas, chains=4), thetas, 4)
    ch.close()


def test_nan_constant_and_infinite_coordinates(native, series):
    """one coordinate all equal, one with a NaN (in the middle draw an odd S drops: still undefined), one with an infinity: NaN in both
    outputs for exactly those, the neighbours' bits unchanged"""
    ch = gen3_chain(native)
    sr = np.ascontiguousarray(series[:60, :130])                 # four chains of 15
    clean = ch.series_diagnostics(sr, chains=4)
    assert not np.isnan(clean[0]).any() and not np.isnan(clean[1]).any()
    bad = sr.copy()
    bad[:, 5] = 2.5
    bad[15 + 7, 64] = np.nan                                     # chain 1, draw 7 of 15: the dropped middle draw
    bad[40, 66] = np.nan
    bad[3, 129] = np.inf
    got = ch.series_diagnostics(bad, chains=4)
    want = np.zeros(130, dtype=bool)
    want[[5, 64, 66, 129]] = True
    for g, c in zip(got, clean):
        assert np.array_equal(np.isnan(g), want)
        assert np.array_equal(g[~want].view(np.uint64), c[~want].view(np.uint64))
    assert np.array_equal(np.isnan(diag_ref(bad, 4)[0]), want)   # and the restatement calls the same elements undefined
    ch.close()


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(native):
    dp = C.POINTER(C.c_double)
    ch = make_chain(native, "narrow")
    X = rows_for("narrow")
    thetas = walks(ch.P, 2, 8, seed=1)
    n, Pn = X.shape[0], thetas.shape[1]
    lib, p = native.lib, native._p
    before = ch.ensemble_diagnostics(thetas, chains=2, X=X)
    r, e = np.full((1, n), 7.0), np.full((1, n), 7.0)

    def ens(m=16, chains=2, xform=0, stride=Pn, rnull=False, enull=False, which=1, X_=X, n_=n):
        return lib.tbnn_ensemble_diagnostics(ch._h, p(thetas), m, stride, chains, xform, 1.0, 0.0, which, p(X_), n_,
                                             None if rnull else r.ctypes.data_as(dp), None if enull else e.ctypes.data_as(dp))

    sr = np.ascontiguousarray(thetas[:, :n])

    def ser(m=16, chains=2, tot=n, rnull=False, enull=False, snull=False):
        return lib.tbnn_series_diagnostics(ch._h, None if snull else p(sr), m, tot, chains, None if rnull else r.ctypes.data_as(dp),
                                           None if enull else e.ctypes.data_as(dp))

    err = lambda: lib.tbnn_last_error().decode()
    for call in (ens, ser):
        assert call(rnull=True, enull=True) < 0 and "both null" in err()
        assert call(chains=0) < 0 and "n_chains must be 1 .. 64" in err()
        assert call(chains=-1) < 0 and "n_chains must be 1 .. 64" in err()
        assert call(chains=65) < 0 and "n_chains must be 1 .. 64" in err()
        assert call(chains=3) < 0 and "not divisible" in err()
        assert call(m=15, chains=3) < 0 and "fewer than 8" in err()
        assert call(chains=4) < 0 and "fewer than 8" in err()
        assert call(m=0, chains=1) < 0 and "m < 1" in err()
        # 64 rows of all m draws past the block budget: refused before anything is read
        assert call(m=(1 << 22) + 8, chains=1) < 0 and "block budget" in err()
    assert ens(xform=4) < 0 and "unknown transform" in err()
    assert ens(xform=-1) < 0 and "unknown transform" in err()
    assert ens(xform=native.XFORM_SOFTMAX) < 0 and "at least 2 outputs" in err()
    assert ens(stride=Pn - 1) < 0 and "theta_stride < P" in err()
    assert ens(X_=None, n_=0, which=1) < 0 and "tbnn_set_validation has not been called" in err()
    assert ens(X_=None, n_=0, which=2) < 0 and "which must be" in err()
    assert ser(snull=True) < 0 and "null series" in err()
    assert ser(tot=0) < 0 and "tot < 1" in err()
    assert np.all(r == 7.0) and np.all(e == 7.0)                 # nothing written
    with pytest.raises(native.TbnnError, match="fewer than 8"):
        ch.ensemble_diagnostics(thetas, chains=4, X=X)
    with pytest.raises(native.TbnnError, match="not divisible"):
        ch.series_diagnostics(sr, chains=3)
    assert ens() == 0 and np.array_equal(r, before[0]) and np.array_equal(e, before[1])      # and the accepted calls still work
    assert ser() == 0 and np.array_equal(r[0], ch.series_diagnostics(sr, chains=2)[0])
    ch.close()


# ---------------------------------------------------------------------------------------------------------------- predictor, end to end
def test_predictor_over_train_chains(tmp_path, monkeypatch, native):
    """two chains written by trainChains, read back by predictor.fromChains: predictDiagnostics is the restatement applied to predict's
    values (softmax: read back per network), thinning picks every second draw of each chain, parameterDiagnostics covers every
    parameter and hyper coordinate"""
    from test_gpu_categorical import blobs, make_net
    from tensorbnn_amd.likelihood import CategoricalLikelihood
    from tensorbnn_amd.predictor import predictor
    monkeypatch.chdir(tmp_path)
    X, Y = blobs(600, 1)
    Xv, _Yv = blobs(70, 2)
    net = make_net(X, Y, Xv, _Yv)
    net.trainChains(2, 44, 1, CategoricalLikelihood(), folderName="multi", networksPerFile=8)
    p = predictor.fromChains(str(tmp_path / "multi"), likelihood=CategoricalLikelihood())
    S = p.numNetworks // 2
    assert p.numChains == 2 and S >= 16
    solo = predictor(str(tmp_path / "multi" / "chain1"))
    assert solo.numChains == 1 and np.array_equal(solo.vectors[0], p.vectors[S])
    out = p.predictDiagnostics(Xv, transform="none", sd=2.0, mean=0.5)
    logits = np.array(p.predict(Xv))
    compare("predictor logits", (out["rhat"], out["ess"]), fma32(logits, 2.0, 0.5), 2)
    assert out["undefined"] == int(np.isnan(out["rhat"]).sum()) < out["rhat"].size
    assert out["max_rhat"] == np.nanmax(out["rhat"]) and out["min_ess"] == np.nanmin(out["ess"])
    soft = p.predictDiagnostics(Xv, n=2)                        # the softmax by default; every second draw of each chain
    picked = np.stack([p.vectors[c * S + s] for c in range(2) for s in range(0, S, 2)])
    compare("predictor softmax, thinned", (soft["rhat"], soft["ess"]), device_t(p._chain, picked, Xv, native.XFORM_SOFTMAX, 1.0, 0.0), 2)
    par = p.parameterDiagnostics()
    series = np.concatenate([np.stack(p.vectors), np.stack([np.asarray(h).reshape(-1) for h in p.hypers])], axis=1)
    assert par["rhat"].shape == (series.shape[1],) and series.shape[1] > len(p.vectors[0])
    compare("predictor parameters", (par["rhat"], par["ess"]), series, 2)
    assert par["undefined"] == int(np.isnan(par["rhat"]).sum())
