"""CPU: the datasets of tests/lik_edge_cases.py without a GPU -- (1) every dataset holds its band on every (row, output), the straddle
datasets hold both sides of the clip in every 16-row tile, the Poisson `high` datasets keep the fp32 gradient sums finite, and no last-layer
bias gradient is a cancelled sum; (2) the fp32 arm of each reference (the kernel's formula operation by operation) against its fp64 arm
at every dataset, in the suite's metrics: the printed gaps are what the GPU module's bands come from (lik_edge_cases.arms); (3) sensitivity:
seven subtly wrong element formulas, applied to a copy of the fp32 arm kept HERE (nothing in the oracle changes), are caught by at least
one named band, and the ordinary CASES problems of the likelihood modules let most of them through.

Measured here (fp32 arm against fp64 over all datasets; NOTES.md has the table): value gaps to 1.5e-5, gradient gaps to 5.5e-5, both at
`hetero lay_last straddle`; only `hetero lay_last straddle` and `hetero lay_tail straddle` leave half the project bands and take
max(project band, 8 x gap).

Mutation (g), max(mu, FLT_MIN) in the Poisson term, moves one element by at most FLT_MIN = 1.2e-38: against a log-posterior or a gradient,
whose metrics have floors (1 and 1e-3), nothing can show it, and `deep-` and `high` do not.  The statistic is judged relative to itself, so
the Poisson band `flush` (lik_edge_cases.FLUSH_TOP / FLUSH_BOTTOM) shows it: every target 0, a third of the elements just above FLT_MIN
carrying the sum (~1e-36), the rest at the bottom of the denormals, where flushing them or not moves the sum by 1.5e-7 of itself and
max(mu, FLT_MIN) doubles it (gap / band 3e5).

Gamma (seven bands, NOTES.md has the fp32 arm's gaps per band): occupancy, targets inside [FLT_MIN, 2^100] (the staging ceiling), the
conditioning cap, no overflow in the fp64 arm; mutations (h) .. (m), each caught by EVERY case of the bands named for it (GAMMA_NAMED) or
recorded as invisible with the reason (INVISIBLE): (l), the hardware's own flush of e^-f, must stay invisible at `flush` and `flush-top`.
Three `deep-` datasets with a = 200 take widened value and statistic bands (-a f against (a - 1) log y cancels: NOTES.md)."""
import math

import numpy as np
import pytest

import gamma_ref as gr
import hetero_ref as hr
import lik_edge_cases as E
import negbin_ref as nb
import student_ref as sr
import tbnn_oracle as o

FLT_MIN = np.float32(np.finfo(np.float32).tiny)
KEYS = E.all_keys() + [("negbin", E.TRAJ, "far+"), ("negbin", E.TRAJ, "deep-"), ("gamma", E.TRAJ, "deep-")]


@pytest.mark.parametrize("key", KEYS, ids=lambda k: "-".join(k))
def test_dataset_holds_its_band_and_is_well_conditioned(key):
    ds = E.dataset(*key)
    n, d_out = ds.X.shape[0], ds.spec.layers[-1].out_dim
    assert n == E.N_ROWS and n % 16 != 0 and n // 16 == 18
    d, q, z = E.deltas(ds)
    occ = E.in_band(ds, q)
    rt = E.ratio(d)
    a = E.arms(ds)
    print(f"[edges] {ds.tag}: {int(occ.sum())} of {occ.size} in the band, branch quantity [{q.min():.6g}, {q.max():.6g}], "
          f"sum|delta| / |sum delta| max {rt.max():.2f}" + (f", mixture {tuple(round(m, 2) for m in ds.mix)}" if ds.mix else "")
          + f"; fp32 arm: value gap {a['gv']:.3e}, gradient gaps max {max(a['gg']):.3e}, statistic gap {a['gs']:.3e}; GPU bands: value "
          f"{a['bv']:.3e}, gradient max {max(a['bg']):.3e}" + ("" if a["bv"] == 4e-6 and max(a["bg"]) == 1e-4 else " (widened)"))
    assert occ.all(), (ds.tag, q[~occ][:8])
    assert np.all(rt <= 4.0), (ds.tag, rt)
    assert np.isfinite(a["lp32"]) and np.all(np.isfinite(a["g32"])) and np.isfinite(a["lp64"]) and np.all(np.isfinite(a["g64"]))
    assert ds.Y.dtype == np.float32 and np.all(np.isfinite(ds.Y))
    if ds.lik in ("negbin", "poisson"):
        assert np.all(ds.Y >= 0) and np.all(ds.Y <= E.MAX_COUNT) and np.all(ds.Y == np.floor(ds.Y))
    if ds.lik == "negbin":
        assert np.isclose(sum(ds.mix), 1.0) and min(ds.mix) >= 0.1 and (ds.Y == 0).any() and ((ds.Y >= 1) & (ds.Y <= 5)).any()
    if ds.lik == "hetero":
        assert ds.Y.shape == (n,) and d_out == 2
    if ds.band == "straddle":
        g = np.abs(q[0])
        tiles = [g[i:i + 16] for i in range(0, n, 16)]
        assert all((t < E.HETERO_CLIP).any() and (t > E.HETERO_CLIP).any() for t in tiles), "both sides of the clip in every 16-row tile"
        assert (q > 0).any() and (q < 0).any() and np.all(np.abs(g - E.HETERO_CLIP) >= E.STRADDLE_DROP)
    if ds.lik == "poisson" and ds.band == "high":
        _f, acts = o.forward(ds.spec, ds.theta.astype(np.float64), ds.X.astype(np.float64), np.float64, keep=True)
        assert n * max(np.abs(acts[-2]).max(), 1.0) * math.exp(z.max()) < E.FLT_MAX / 16.0
        assert set(np.unique(ds.Y)) <= {0.0, 1e3, 1e8}
    if ds.lik == "poisson" and ds.band == "flush":
        top = z >= E.FLUSH_TOP[0]
        assert np.all(ds.Y == 0) and np.all(z[top] <= E.FLUSH_TOP[1]) and np.all((z[~top] >= E.FLUSH_BOTTOM[0]) & (z[~top] <= E.FLUSH_BOTTOM[1]))
        assert 3 * int(top.sum()) >= top.size and np.exp(z[top]).min() > float(FLT_MIN)          # normal numbers carry the sum ...
        assert np.exp(z[~top]).sum() <= 1e-6 * np.exp(z[top]).sum()                                # ... flushing the rest or not is 1e-6 of it
        assert a["st64"] < 0 and abs(a["st64"] + np.exp(z).sum()) <= 1e-12 * abs(a["st64"])        # the statistic is -sum e^f alone
        if d_out == 1:
            assert all(t.any() and not t.all() for t in (top[0, i:i + 16] for i in range(0, n, 16))), "both groups in every 16-row tile"
    if ds.lik == "poisson" and ds.band == "deep-":
        assert np.all(ds.Y[np.arange(n) % 4 != 3] == 0) and np.all((ds.Y[3::4] >= 1) & (ds.Y[3::4] <= 3))
    if ds.lik == "gamma":
        lo, hi = E.gamma_f_range(ds.band)
        assert np.all((z >= lo) & (z <= hi)), (ds.tag, z.min(), z.max())                      # the log-means, whatever the band is placed through
        assert ds.Y.shape == (n, d_out) and np.all(ds.Y >= FLT_MIN) and np.all(ds.Y <= E.Y_MAX)      # normal fp32 numbers the staging call admits
        assert ds.par["a"] == gr.CASES[ds.case][6] == ds.spec.lik_df and set(ds.par["c"]) <= set(E.GAMMA_C)
        with np.errstate(over="raise", invalid="raise", divide="raise"):                       # no overflow in the fp64 arm
            t64, d64 = o.gamma_elementwise(z, ds.Y, ds.par["a"], np.float64)
        assert np.all(np.isfinite(t64)) and np.all(np.isfinite(d64)) and np.all(np.isfinite(o.gamma_terms(z, ds.Y, ds.par["a"])))
        rho = ds.Y.astype(np.float64).T * np.exp(-z)
        if ds.band in ("deep-", "high"):          # targets from the model around c e^f: rho is O(1), no row decides the sum
            assert 0.2 <= np.median(rho) <= 4.0 and rho.max() <= 64.0, (ds.tag, np.median(rho), rho.max())
        if ds.band in E.GAMMA_FLUSHED:            # e^-f below FLT_MIN on every element, and what it multiplies at most 2^100
            assert np.all(np.exp(-z) < float(FLT_MIN)) and ds.Y.max() <= 2.0 ** 100 and rho.max() < 2.0 ** -26
        if ds.band == "high-top":                 # e^-f a normal number on every element, against targets up to the ceiling
            assert np.all(np.exp(-z) > float(FLT_MIN)) and ds.Y.max() <= 2.0 ** 100 and rho.max() > 1e-2 and rho.min() < 1e-15
        if ds.band in ("small", "big") + E.GAMMA_FLUSHED:
            assert np.all(d < 0) or np.all(d > 0)                                              # one-signed by construction


@pytest.mark.parametrize("case", E.DENORMAL_CASES)
def test_denormal_target_dataset(case):
    """the dataset of test_gpu_likelihood_edges.test_denormal_targets: nearly every target an fp32 denormal, none 0, e^-f below its overflow,
    rho on both sides of 1, well conditioned, and the fp32 arm inside half of the project's bands"""
    ds = E.measured(case, "denormal-targets")
    d, _q, z = E.deltas(ds)
    a = E.arms(ds)
    rho = ds.Y.astype(np.float64).T * np.exp(-z)
    print(f"[edges] {ds.tag}: targets [{ds.Y.min():.3g}, {ds.Y.max():.3g}], {float((ds.Y < FLT_MIN).mean()):.3f} of them denormal, f [{z.min():.2f}, {z.max():.2f}], "
          f"rho [{rho.min():.3g}, {rho.max():.3g}]; fp32 arm: value gap {a['gv']:.3e}, gradient gaps max {max(a['gg']):.3e}, statistic gap {a['gs']:.3e}")
    assert ds.Y.dtype == np.float32 and np.all(ds.Y > 0) and (ds.Y < FLT_MIN).mean() >= 0.99
    assert np.all((z >= -88.5) & (z <= -87.5)) and rho.min() < 0.1 and rho.max() > 1.2 and np.all(E.ratio(d) <= 4.0)
    assert np.isfinite(a["lp32"]) and np.all(np.isfinite(a["g32"]))
    assert a["gv"] <= 2e-6 and a["gs"] <= 2e-6 and max(a["gg"]) <= 5e-5 and (a["bv"], a["bs"], max(a["bg"])) == (4e-6, 4e-6, 1e-4)


def test_parametrisation_covers_every_case_and_band():
    keys = E.all_keys()
    assert len(keys) == 11 * 4 + 11 * 9 + 9 * 6 + 11 * 3 + 11 * len(E.GAMMA_BANDS) and len(E.GAMMA_BANDS) >= 5
    assert E.LIKS[:4] == ("student", "negbin", "hetero", "poisson")          # a dataset's seed holds the index: the order stays
    assert [E.gamma_shape(c) for c in E.CASE_NAMES[:4]] == [0.5, 10.0, 200.0, 0.5] and {E.gamma_shape(c) for c in E.CASE_NAMES} == {0.5, 2.0, 10.0, 200.0}
    assert all(gr.CASES[c][:6] == sr.CASES[c][:6] for c in E.CASE_NAMES + (E.TRAJ,))
    assert [E.dispersion(c) for c in E.CASE_NAMES[:4]] == [0.5, 1e4, 1e6, 0.5] and {E.dispersion(c) for c in E.CASE_NAMES} == set(E.R_EDGE)
    for lik in E.LIKS:
        for case in E.case_names(lik):
            ref = hr.CASES if lik == "hetero" else sr.CASES
            assert E.case_of(lik, case) == tuple(ref[case][:6])
    assert all(nb.CASES[c][:6] == sr.CASES[c][:6] for c in E.CASE_NAMES + (E.TRAJ,))


# ---------------------------------------------------------------------------------------------------------------------- the fp32 arm, copied
def log1p32(u, mut=None):
    """the oracle's log1p_kernel32; (a): log(1 + u) in fp32; (b): the switch at u < 4"""
    u = np.asarray(u, dtype=np.float32)
    one, two = np.float32(1), np.float32(2)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if mut == "a":
            return np.log(one + u).astype(np.float32)
        z = u * (one / (two + u))
        z2 = z * z
        ser = (two * z) * (z2 * (z2 * (z2 * np.float32(1.0 / 7.0) + np.float32(0.2)) + np.float32(1.0 / 3.0)) + one)
        return np.where(u < np.float32(4.0 if mut == "b" else 0.25), ser, np.log(one + u)).astype(np.float32)


def elem32(ds, f, mut=None):
    """(the statistic's terms, dL/df) of the dataset's likelihood in fp32, as the reference's fp32 arm forms them; `mut`: one mutation"""
    one = np.float32(1)
    f = np.asarray(f, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        if ds.lik == "hetero":
            y = np.asarray(o.hetero_targets(ds.Y, f.shape[1]), dtype=np.float32)
            G = np.float32(o.LOG_CLIP)
            g = f[1]
            gc = np.where(g < -G, -G, g)
            gc = np.where(g > G, G, gc).astype(np.float32)
            inside = (g >= -G) & (g <= G)
            u = np.exp(np.float32(-2) * (g if mut == "f" else gc)).astype(np.float32)
            r = (y - f[0]).astype(np.float32)
            ru = (r * u).astype(np.float32)
            q = (r * ru).astype(np.float32)
            term = (-gc - np.float32(0.5) * q).astype(np.float32)
            dg = (q - one) if mut == "e" else np.where(inside, q - one, np.float32(0))
            return term[None], np.stack([ru, dg]).astype(np.float32)
        y = np.asarray(ds.Y, dtype=np.float32).reshape(f.shape[1], -1).T
        if ds.lik == "student":
            nu32, s32 = np.float32(ds.par["nu"]), np.float32(o.student_scale(ds.spec))
            r = y - f
            k = one / (nu32 * s32 * s32)
            u = r * r * k
            d = (nu32 + one) * (r * k) * (one / (one + u))
            return log1p32(u, mut), d.astype(np.float32)
        if ds.lik == "negbin":
            r32 = np.float32(ds.par["r"])
            lr = np.log(r32)
            t = f - lr
            a = np.abs(t)
            e = np.exp(-a).astype(np.float32)
            l = log1p32(e, mut)
            nlq = np.maximum(t, np.float32(0)) + l
            rc = one / (one + e)
            s = e * rc
            pos = np.ones(t.shape, bool) if mut == "c" else t >= 0
            p, q = np.where(pos, rc, s), np.where(pos, s, rc)
            nlp = -np.log(p) if mut == "d" else np.maximum(-t, np.float32(0)) + l
            return (-(y * nlp + r32 * nlq)).astype(np.float32), (y * q - r32 * p).astype(np.float32)
        if ds.lik == "gamma":
            a32 = np.float32(ds.par["a"])
            e = np.exp(-f).astype(np.float32)
            if mut == "h":
                e = np.minimum(e, np.float32(1e30))
            if mut == "l":
                e = np.where(e < FLT_MIN, np.float32(0), e)
            ye = (y * e).astype(np.float32)
            if mut in ("i", "m"):
                ye = np.maximum(ye, np.float32(1e-6 if mut == "i" else 1e-2))
            d = (a32 * ye - one) if mut == "j" else a32 * (ye - one)
            return (ye if mut == "k" else f + ye).astype(np.float32), d.astype(np.float32)
        mu = np.exp(f)
        if mut == "g":
            mu = np.maximum(mu, FLT_MIN)
        return (y * f - mu).astype(np.float32), (y - mu).astype(np.float32)


def coefficient(ds):
    """d(log posterior) / d(sum of elem32's terms)"""
    return -0.5 * (ds.par["nu"] + 1.0) if ds.lik == "student" else -float(ds.par["a"]) if ds.lik == "gamma" else 1.0


def value_grad32(ds, a32, mut=None):
    """(log posterior, gradient, statistic) with elem32 in the place of the reference's fp32 element code: the reference's fp32 value moved by the
    change of the terms' fp64 sum, and the reference's reverse-mode layer loop over elem32's deltas"""
    dt = np.float32
    spec, theta, eta = ds.spec, ds.theta.astype(dt), ds.eta.astype(dt)
    parts = o.unflatten(spec, theta)
    f, acts = o.forward(spec, theta, ds.X, dt, keep=True)
    t0, _d0 = elem32(ds, f)
    t, d_a = elem32(ds, f, mut)
    with np.errstate(over="ignore", invalid="ignore"):
        moved = float(np.sum(t.astype(np.float64))) - float(np.sum(t0.astype(np.float64)))
        # (the statistic of `arms`: Student-t's is the sum of the terms itself, the others' the data term -- Gamma's with its factor -a)
        lp, st = a32["lp32"] + coefficient(ds) * moved, a32["st32"] + (moved if ds.lik == "student" else coefficient(ds) * moved)
        grads = [None] * len(spec.layers)
        for i in range(len(spec.layers) - 1, -1, -1):
            l = spec.layers[i]
            W, b = parts[i]
            delta = (d_a * o.act_grad_from_output(acts[i + 1], l.act)).astype(dt)
            gW = delta @ acts[i].T
            gb = np.sum(delta, axis=1, keepdims=True, dtype=dt)
            pW, pb = o.prior_grad(l, eta[4 * i:4 * i + 4], W, b, dt)
            grads[i] = ((gW + pW).astype(dt), (gb + pb).astype(dt))
            if i > 0:
                d_a = (W.T @ delta).astype(dt)
    return lp, o.flatten(grads).astype(dt), st


@pytest.mark.parametrize("key", [("student", "fast3", "switch"), ("student", "mid10", "small"), ("negbin", "wide10", "deep-"), ("negbin", "generic", "zero"),
                                 ("hetero", "fast", "straddle"), ("hetero", "lay_tail", "near-"), ("poisson", "tall", "high"), ("poisson", "mid10", "deep-"),
                                 ("gamma", "fast3", "deep-"), ("gamma", "mid10", "flush"), ("gamma", "wide10", "big"), ("gamma", "lay_tail", "small")],
                         ids=lambda k: "-".join(k))
def test_the_copy_is_the_reference_arm(key):
    """unmutated, value_grad32 gives the reference's fp32 arm: the gradient bit for bit"""
    ds = E.dataset(*key)
    a = E.arms(ds)
    lp, g, st = value_grad32(ds, a)
    assert lp == a["lp32"] and st == a["st32"] and np.array_equal(g, a["g32"])


MUTATIONS = {
    # mutation: (likelihoods it applies to, what it is)
    "a": (("student", "negbin"), "log1p_fast becomes log(1 + u) in fp32"),
    "b": (("student", "negbin"), "log1p_fast's switch moves to u < 4"),
    "c": (("negbin",), "negbin_term always takes the t >= 0 selection of p, q"),
    "d": (("negbin",), "negbin_term computes -log p as -log(p) from the formed p"),
    "e": (("hetero",), "hetero_pair uses dg = q - 1 outside the clip too"),
    "f": (("hetero",), "hetero_pair clips g but computes u from the unclipped g"),
    "g": (("poisson",), "Poisson's mu becomes max(mu, FLT_MIN)"),
    "h": (("gamma",), "gamma_term puts a ceiling on e^-f: min(e, 1e30)"),
    "i": (("gamma",), "gamma_term puts a floor under y e^-f: max(ye, 1e-6)"),
    "j": (("gamma",), "the Gamma delta becomes a ye - 1 for a (ye - 1)"),
    "k": (("gamma",), "the Gamma term loses f"),
    "l": (("gamma",), "e^-f flushed to 0 below FLT_MIN (the hardware exp's own behaviour)"),
    "m": (("gamma",), "gamma_term puts a floor under y e^-f: max(ye, 1e-2)"),
}
# the Gamma mutations and the bands named for them: EVERY case of a named band must catch the mutation; (l) is what the hardware does, and
# the band `flush` must NOT catch it on any case -- the band admits the hardware
GAMMA_NAMED = {"h": ("deep-",), "i": (), "j": tuple(b for b in E.GAMMA_BANDS if b != "big"), "k": ("high", "flush", "flush-top", "high-top"), "l": (), "m": ("small",)}
# INVISIBLE, with the reason.  (i), a floor of 1e-6 under ye: it moves one delta by at most 1e-6 a, that is 1e-6 of the deltas' own size
# (|delta| >= a (1 - 1e-3) at `small`), and one term by 1e-6 against |f| of O(1): a hundredth of the gradient band (1e-4 of a tensor's largest
# entry) and a quarter of the value band at the very most -- no band of the suite's metrics can show a change of 1e-6 relative, at `small` or
# anywhere.  The same floor at 1e-2, (m), is 1e-2 relative and every `small` dataset catches it: a floor shows once it reaches the bands.
# (l), the flush: invisible by design (above).  (j) is named for every band but `big`: there the deltas are a rho with rho from 1e3 to 1e20, the
# largest entries carry every tensor's norm, and the a - 1 that (j) adds to each is below 1e-17 of them.
INVISIBLE = ("i", "l")
# the bands the GPU builds with (a), (c), (e) in csrc/common.hpp must fail on: what this module predicts (printed; NOTES.md has the runs)


def over_band(ds, a, lp, g, st):
    """how far a (value, gradient, statistic) lies outside the dataset's GPU bands: max(gap / band) over the value, the statistic and
    every tensor; inf if not finite"""
    if not (np.isfinite(lp) and np.isfinite(st) and np.all(np.isfinite(g))):
        return math.inf
    ev, eg = E.gaps(ds.spec, lp, g, a["lp64"], a["g64"])
    return max([ev / a["bv"], abs(st - a["st64"]) / abs(a["st64"]) / a["bs"]] + [e / b for e, b in zip(eg, a["bg"])])


def ordinary(lik):
    """the likelihood module's own CASES problems as datasets: {name: Dataset}"""
    out = {}
    if lik == "poisson":
        import test_gpu_poisson as tp
        for name in tp.CASES:
            spec, X, Y, theta, eta = tp.problem(name)
            out[name] = E.Dataset(lik=lik, case=name, band="CASES", spec=spec, X=X, Y=Y, theta=theta, eta=eta, par={}, mix=None)
        return out
    mod = {"student": sr, "negbin": nb, "hetero": hr, "gamma": gr}[lik]
    for name in mod.CASES:
        spec, X, Y, theta, eta = mod.problem(name)[:5]
        par = {"nu": spec.lik_df, "s": spec.fixed_sd} if lik == "student" else {"r": spec.lik_df} if lik == "negbin" else {"a": spec.lik_df} if lik == "gamma" else {}
        out[name] = E.Dataset(lik=lik, case=name, band="CASES", spec=spec, X=X, Y=Y, theta=theta, eta=eta, par=par, mix=None)
    return out


_ORD = {}


def ordinary_arms(lik):
    if lik not in _ORD:
        _ORD[lik] = {}
        for name, ds in ordinary(lik).items():
            lp64, g64 = E.target(ds, np.float64)
            lp32, g32 = E.target(ds, np.float32)
            _ORD[lik][name] = (ds, dict(lp64=lp64, g64=g64, lp32=lp32, g32=g32, st64=E.statistic(ds, np.float64), st32=E.statistic(ds, np.float32),
                                        bv=4e-6, bs=4e-6, bg=[1e-4] * (2 * len(ds.spec.layers))))
    return _ORD[lik]


# what the ordinary CASES problems do with each mutation, at the project bands (measured here; asserted below so that it stays true):
# the cases that CATCH it -- every other case lets it through
ORDINARY_CATCHES = {
    "a": {"student": set(), "negbin": set()},
    "b": {"student": None, "negbin": None},          # (the ordinary Student-t problems hold u in [1/4, 4): most of them catch it)
    "c": {"negbin": None},                           # (every ordinary negative-binomial problem has log-rates below log r: all catch it)
    "d": {"negbin": set()},
    "e": {"hetero": set()},
    "f": {"hetero": set()},
    "g": {"poisson": set()},
    "h": {"gamma": set()},
    "i": {"gamma": set()},
    "j": {"gamma": set(gr.CASES) - {"mid10"}},       # (a delta off by a - 1 on every element; mid10, a = 0.5 on ten outputs, stays inside)
    "k": {"gamma": set(gr.CASES)},
    "l": {"gamma": set()},
    "m": {"gamma": {"fast3", "fast3_two_outputs", "lay_last", "tall", "traj"}},          # (shapes 0.5 and 2: targets below a hundredth of the mean)
}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_is_caught(mut):
    """at least one band's gap exceeds its GPU band under the mutation (the bands named in the printout).  Measured: (a) .. (f) are caught by
    9 .. 55 datasets each, (g) by the 11 `poisson flush` datasets, through the statistic"""
    liks, what = MUTATIONS[mut]
    caught = []
    for lik in liks:
        for case in E.case_names(lik):
            for band in E.BANDS[lik]:
                ds = E.dataset(lik, case, band)
                a = E.arms(ds)
                x = over_band(ds, a, *value_grad32(ds, a, mut))
                if x > 1.0:
                    caught.append((lik, case, band, x))
    bands = sorted({(l, b) for l, _c, b, _x in caught})
    print(f"[edges] mutation ({mut}) {what}: caught by {len(caught)} datasets, bands "
          + ", ".join(f"{l} {b} ({sum(1 for c in caught if (c[0], c[2]) == (l, b))} cases, gap/band to "
                      f"{max(c[3] for c in caught if (c[0], c[2]) == (l, b)):.3g})" for l, b in bands))
    if mut in INVISIBLE:
        assert not caught, f"mutation ({mut}) {what} is caught by {caught}" + (": the bands must admit the hardware" if mut == "l" else "")
        return
    assert caught, f"mutation ({mut}) {what}: no band's gap exceeds its GPU band"
    for band in GAMMA_NAMED.get(mut, ()):
        missed = [c for c in E.case_names("gamma") if ("gamma", c, band) not in {k[:3] for k in caught}]
        assert not missed, f"mutation ({mut}) {what}: the band {band} named for it lets it through on {missed}"


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_what_the_ordinary_cases_let_through(mut):
    """the same mutation on the likelihood modules' own CASES problems, at the project bands: which cases stay inside them (printed, and
    asserted as measured: ORDINARY_CATCHES) -- the gap the edge datasets close"""
    liks, what = MUTATIONS[mut]
    for lik in liks:
        catches = set()
        worst = 0.0
        for name, (ds, a) in ordinary_arms(lik).items():
            x = over_band(ds, a, *value_grad32(ds, a, mut))
            worst = max(worst, x)
            if x > 1.0:
                catches.add(name)
        print(f"[edges] mutation ({mut}) {what} on the ordinary {lik} CASES: " + (f"caught by {sorted(catches)}" if catches else "stays INSIDE the project bands on every case")
              + f" (worst gap/band {worst:.3g})")
        want = ORDINARY_CATCHES[mut][lik]
        if want is not None:
            assert catches == want, (mut, lik, catches)
