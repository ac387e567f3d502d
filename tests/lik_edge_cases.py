"""The datasets of tests/test_likelihood_edges_host.py and tests/test_gpu_likelihood_edges.py: the Poisson, Student-t, negative-binomial,
heteroscedastic Gaussian and Gamma likelihoods on the inputs where their element arithmetic (csrc/common.hpp log1p_fast, negbin_term,
hetero_pair, gamma_term; kernels_fast.hpp lik_delta's Poisson branch) changes regime.  Importable without a GPU; no reference formula is stated here -- the fp64 and
fp32 arms are the oracle's.

A BAND is a range of the quantity the element code branches on (Student-t: u = (y - f)^2 / (nu s^2); negative binomial: t = f - log r;
heteroscedastic Gaussian: g, the log-sd output; Poisson: the log-rate; Gamma: the log-mean f, or rho = y e^-f).  One dataset holds ONE band on every (row, output), so the band's
error is not diluted by well-conditioned rows.  A dataset is built as test_gpu_edges.saturated_problem builds its own: the case's shape,
activations, priors and initial state (student_ref.CASES / hetero_ref.CASES), the hidden layers left alone, the last layer rescaled and
shifted per output so that the fp64 outputs at the fp32 state land in the band over a pool of rows, N_ROWS = 301 rows (18 full 16-row tiles
and a ragged one) picked from the pool.  Student-t leaves the outputs O(1) and places u through the targets.

Conditioning: in every dataset the residual signs (one per output, alternating over outputs and datasets) or the mixture of count targets
are chosen so that the last layer's bias gradient is no cancelled sum on the fp64 reference -- sum |delta| / |sum delta| <= 4 per output.
Gamma targets drawn from the model would have E[delta] = 0: a factor c per output (2 or 1/2, alternating as the signs do) takes them off the
model's mean; the bands placed through rho are one-signed by construction.

Bands of the GPU module (`arms`): the project's (value 4e-6 relative, gradient 1e-4 of each tensor's largest entry, floor 1e-3)
wherever the fp32 arm of the reference is inside HALF of them; otherwise max(project band, 8 x the fp32 arm's gap against fp64), the rule of
test_gpu_poisson.bands.  Computed from the references alone."""
import math

import numpy as np

import gamma_ref as gr
import hetero_ref as hr
import negbin_ref as nb
import student_ref as sr
import tbnn_oracle as o
from tensor_checks import tensor_errs

N_ROWS = 301
POOL = 16000
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
LIKS = ("student", "negbin", "hetero", "poisson", "gamma")          # (a dataset's seed holds the index: new likelihoods go at the end)
# the kernels reached: narrow (fast3, fast), mid VALU / MFMA output tile, tall, wide VALU / MFMA, the three layered likelihood
# kernels, generic; the heteroscedastic Gaussian has the 2-output versions (hetero_ref.CASES: no MFMA-output case)
CASE_NAMES = ("fast3", "fast", "mid1", "mid10", "tall", "wide1", "wide10", "lay_last", "lay_separate", "lay_tail", "generic")
HETERO_NAMES = ("fast3", "fast", "mid", "tall", "wide", "lay_last", "lay_separate", "lay_tail", "generic")
TRAJ = "traj"

STUDENT_BANDS = {          # nu, s, u range
    "small": (1e4, 1.0, 1e-6, 1e-3),          # residuals 0.1 .. 3: the series, where a bare log(1 + u) loses the term
    "switch": (4.0, 1.0, 0.2, 0.3),           # either side of log1p_fast's switch at 1/4
    "big": (1.0, 0.1, 1e2, 1e6),
    "huge": (1.0, 0.1, 1e10, 1e30),           # targets to ~1e14
}
NEGBIN_BANDS = {           # sign (0: both), |t| range
    "zero": (0, -0.05, 0.05),
    "switch+": (+1, 1.30, 1.47), "switch-": (-1, 1.30, 1.47),          # e = e^-|t| either side of 1/4 (ln 4 = 1.386)
    "mid+": (+1, 5.0, 20.0), "mid-": (-1, 5.0, 20.0),
    # deep: e passes through the denormals (e^-87.3 = FLT_MIN): the hardware exp flushes them to 0 where NumPy's does not -- a difference
    # below 1e-37 absolute in l, p or q, which no band sees
    "deep+": (+1, 60.0, 104.0), "deep-": (-1, 60.0, 104.0),
    "far+": (+1, 1e3, 1e6), "far-": (-1, 1e3, 1e6),                    # far past the range of exp: e = 0
}
HETERO_CLIP = o.LOG_CLIP
HETERO_BANDS = {           # sign (0: both), |g| range
    "inside": (0, -3.0, 3.0),
    "near+": (+1, 16.0, 18.40), "near-": (-1, 16.0, 18.40),
    "outside+": (+1, 18.44, 30.0), "outside-": (-1, 18.44, 30.0),
    "straddle": (0, 17.5, 19.5),              # |g|, both signs, both sides of the clip in every 16-row tile
}
STRADDLE_DROP = 0.01                          # | |g| - log(1e8) | below this: fp32 and fp64 may decide the clip differently (test_gpu_edges.DROP)
POISSON_BANDS = {"deep-": (-104.0, -20.0), "high": (60.0, 80.0), "flush": (-104.0, -86.8)}
# `flush`: the log-rates where e^f leaves fp32's normal range (FLT_MIN = e^-87.34), every target 0, so that the statistic is -sum e^f alone
# and is judged relative to itself.  A third of the elements sit just above FLT_MIN (FLUSH_TOP) and carry the sum, ~1e-36; the rest sit at
# the bottom of the denormals (FLUSH_BOTTOM: e^f <= 1.9e-45), where their true part of the sum is 1e-7 of it -- the hardware exp may
# flush them and NumPy keep them, either inside the band -- while a term that keeps mu away from 0 (max(mu, FLT_MIN)) doubles the sum.
# With one output the two groups are rows taken in turn (every 16-row tile holds both); with more, the outputs take the groups in turn
FLUSH_TOP, FLUSH_BOTTOM = (-87.3, -86.8), (-104.0, -103.0)
# Gamma (csrc/common.hpp gamma_term: e = e^-f, ye = y e, the term f + ye, the delta a (ye - 1)): the range of the log-mean f and, where the
# targets are placed through it, of rho = y e^-f (None: targets drawn from the model, Gamma of shape a around c e^f, c in {2, 1/2})
GAMMA_BANDS = {
    "deep-": (-86.0, -20.0, None),            # e^-f to 2e37 times y down to 1e-37 (every target >= FLT_MIN), the product O(1); (a - 1) log y large in the constant
    # e^-f down to 3e-30 times targets to 2^100, the documented ceiling on a target (include/tbnn.h): model-drawn targets at log-means to 85
    # would reach ~1e37, which staging refuses since the ceiling; log-means from 68 to where e^-f leaves the normal range are `high-top`
    "high": (40.0, 68.0, None),
    "flush": (87.4, 104.0, (1.0, 2.0 ** 100)),          # e^-f denormal or 0: the term is f, the delta -a (here the third entry is the range of y itself)
    "small": (-3.0, 3.0, (1e-30, 1e-3)),      # targets far below the mean: the delta tends to -a, the term to f -- what a clamp or floor on ye changes
    "big": (-3.0, 3.0, (1e3, 1e20)),          # statistic and slabs dominated by ye: sums to ~1e25 in the fp32 slabs, still finite
    # the top of the admitted target range (include/tbnn.h: 2^100) against the largest denormal e^-f: the hardware exp flushes it and the
    # element loses rho = y e^-f up to 2^-26 -- inside every band; NumPy's fp32 arm keeps it
    "flush-top": (87.4, 88.6, (2.0 ** 90, 2.0 ** 100)),          # (the sixth band: at the end, a dataset's seed holds the index)
    # between `high` and `flush`: e^-f normal, down to 1.2e-38, times admitted targets, log-uniform over 2^60 .. 2^100: rho from ~1 down to
    # 1e-20 -- the smallest normal e^-f against the largest targets staging admits
    "high-top": (68.0, 87.3, (2.0 ** 60, 2.0 ** 100)),
}
Y_MAX = 2.0 ** 100                            # the ceiling on a Gamma target (include/tbnn.h)
GAMMA_Y_BANDS = ("flush", "flush-top", "high-top")          # the bands whose third entry is the range of the targets themselves
GAMMA_FLUSHED = ("flush", "flush-top")         # ... and those where e^-f lies below FLT_MIN on every element
GAMMA_C = (2.0, 0.5)                          # the factor that takes model-drawn targets off the model's mean: E|delta| / |E delta| <= 3 for both
BANDS = {"student": STUDENT_BANDS, "negbin": NEGBIN_BANDS, "hetero": HETERO_BANDS, "poisson": POISSON_BANDS, "gamma": GAMMA_BANDS}
R_EDGE = (0.5, 30.0, 1e4, 1e6)                # the dispersions, spread over the cases as negbin_ref._DISPERSIONS is
MIXES = ((1 / 3, 1 / 3, 1 / 3), (0.6, 0.2, 0.2), (0.2, 0.6, 0.2), (0.2, 0.2, 0.6), (0.8, 0.1, 0.1), (0.1, 0.8, 0.1), (0.1, 0.1, 0.8))
MAX_COUNT = 1e8                               # the documented ceiling on a count
WEIGHT_BAND = {"student": "switch", "negbin": "switch+", "hetero": "straddle", "poisson": "deep-", "gamma": "deep-"}


def case_names(lik, traj=False):
    names = HETERO_NAMES if lik == "hetero" else CASE_NAMES
    return names + ((TRAJ,) if traj else ())


def case_of(lik, case):
    """(dims, rows, act, prior, family, env) of the likelihood's own CASES (the Poisson and Gamma modules' shapes are student_ref's)"""
    return tuple((hr.CASES if lik == "hetero" else sr.CASES)[case][:6])


def dispersion(case):
    return R_EDGE[list(nb.CASES).index(case) % 4]


def gamma_f_range(band):
    return GAMMA_BANDS[band][:2]


def gamma_shape(case):
    """gamma_ref.CASES' own: spread over 0.5, 2, 10 and 200"""
    return gr.CASES[case][6]


class Dataset:
    """lik, case, band; spec, X, Y, theta, eta; par: nu and s (Student-t), r (negative binomial) or a and the factors c per output (Gamma);
    mix: the count mixture chosen"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def tag(self):
        return f"{self.lik} {self.case} {self.band}"


_POOL = {}


def _pool(lik, case):
    """(dims, act, prior, pool rows X, the case's initial theta and eta): once per process"""
    key = (lik == "hetero", case)
    if key not in _POOL:
        dims, _n, act, prior, _fam, _env = case_of(lik, case)
        _g, X, _Yr, theta, eta = o.synth_problem(dims, POOL, act, prior, o.LIK_GAUSSIAN)
        if dims[0] > 64:
            X = (X / np.sqrt(dims[0] / 16.0)).astype(np.float32)          # keep a long fan-in's pre-activations O(1), as the _ref modules do
        _POOL[key] = (dims, act, prior, X, np.asarray(theta, np.float32), eta)
    return _POOL[key]


LIK_CODE = {"student": o.LIK_STUDENT_T, "negbin": o.LIK_NEG_BINOMIAL, "hetero": o.LIK_HETERO_GAUSSIAN, "poisson": o.LIK_POISSON,
            "gamma": o.LIK_GAMMA}


def _spec(lik, dims, act, prior, s=1.0, df=0.0):
    """s: the Student-t scale (the other likelihoods have none); df: nu (Student-t), r (negative binomial) or a (Gamma)"""
    scale = {"fixed_sd": float(s)} if lik == "student" else {}
    return o.make_spec(dims, act, prior, LIK_CODE[lik], o.ACT_NONE, lik_df=float(df), **scale)


def _placed(spec, theta, X, ranges):
    """theta (fp32) with the last layer rescaled and shifted: output k's fp64 pre-activations over the pool, 1st to 99th percentile, on
    ranges[k] = (lo, hi) less 5 % either end (None: the output is left alone; ("sd", v[, c]): centred on c = 0 and scaled to the standard deviation v); and the fp64 outputs [d_out, pool] at that fp32 theta"""
    _f, acts = o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64, keep=True)
    a = acts[-2]                                                               # the last hidden layer's activations [h, pool]
    parts = [(W.copy(), b.copy()) for W, b in o.unflatten(spec, theta)]
    W, b = parts[-1]
    z0 = W.astype(np.float64) @ a + b.astype(np.float64)
    for k, rg in enumerate(ranges):
        if rg is None:
            continue
        if rg[0] == "sd":                  # centred, the standard deviation rg[1]: the most rows near +-rg[1]
            sc = rg[1] / z0[k].std()
            W[k] = (W[k].astype(np.float64) * sc).astype(np.float32)
            b[k] = np.float32((float(b[k, 0]) - z0[k].mean()) * sc + (rg[2] if len(rg) > 2 else 0.0))
            continue
        lo, hi = rg
        m = 0.05 * (hi - lo)
        p_lo, p_hi = np.percentile(z0[k], [1.0, 99.0])
        sc = (hi - lo - 2 * m) / (p_hi - p_lo)
        W[k] = (W[k].astype(np.float64) * sc).astype(np.float32)
        b[k] = np.float32((float(b[k, 0]) - p_lo) * sc + lo + m)
    theta = o.flatten(parts).astype(np.float32)
    z = W.astype(np.float64) @ a + b.astype(np.float64)
    return theta, z, float(np.abs(a).max())


def _sign(i, k):
    return 1.0 if (i + k) % 2 == 0 else -1.0


def ratio(delta):
    """per output: sum |delta| / |sum delta| of the data term's derivative [d_out, n] (an all-zero row of deltas is no cancelled sum: 1)"""
    d = np.asarray(delta, np.float64)
    s1, s2 = np.abs(d).sum(axis=1), np.abs(d.sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s1 == 0, 1.0, s1 / s2)


def _counts(rng, z, r, mix):
    """count targets [n, d_out] at the log-rates z [d_out, n]: zeros, small counts 1 .. 5, and draws from the model (a gamma-Poisson mixture
    of dispersion r) where the rate is below 1e6, from {1e3, 1e8} where it is not -- never round(mu)"""
    with np.errstate(over="ignore"):
        mu = np.exp(z.T)
    kind = rng.choice(3, size=mu.shape, p=mix)
    small = rng.integers(1, 6, mu.shape).astype(np.float64)
    low = mu < 1e6
    model = rng.poisson(rng.gamma(float(r), np.where(low, mu, 1.0) / float(r))).astype(np.float64)
    draw = np.where(low, np.minimum(model, MAX_COUNT), rng.choice([1e3, 1e8], mu.shape))
    return np.where(kind == 0, 0.0, np.where(kind == 1, small, draw)).astype(np.float32)


def _z64(spec, theta, X):
    return o.forward(spec, theta.astype(np.float64), X.astype(np.float64), np.float64)


def _build_gamma(case, band, f_range=None, rho_range=None):
    """a Gamma dataset: the log-means placed on the band's range, the targets drawn from the model around c e^f (rows whose targets leave
    [FLT_MIN, 2^100] in fp32 are not taken), or placed through y or rho = y e^-f, log-uniform.  The keywords are for the dataset outside
    the matrix (`measured`)."""
    lik = "gamma"
    dims, act, prior, Xp, theta0, eta0 = _pool(lik, case)
    names = case_names(lik, traj=True)
    bands = list(GAMMA_BANDS) + list(MEASURED)
    i_ds = names.index(case) + bands.index(band)
    rng = np.random.default_rng(1000 * LIKS.index(lik) + 37 * names.index(case) + bands.index(band))
    d_out = dims[-1]
    a = gamma_shape(case)
    if f_range is None:
        lo, hi, tr = GAMMA_BANDS[band]
        y_range, rho_range = (tr, None) if band in GAMMA_Y_BANDS else (None, tr)
    else:
        (lo, hi), y_range = f_range, None
    spec = _spec(lik, dims, act, prior, df=a)
    theta, z, _amax = _placed(spec, theta0, Xp, [(lo, hi)] * d_out)
    idx = np.flatnonzero(np.all((z >= lo) & (z <= hi), axis=0))
    c = np.array([GAMMA_C[0] if _sign(i_ds, k) > 0 else GAMMA_C[1] for k in range(d_out)])
    if y_range is None and rho_range is None:
        # targets from the model over every candidate row; a row is taken if all of its targets are normal fp32 numbers up to the ceiling 2^100
        Yp = rng.gamma(a, c[None, :] * np.exp(z[:, idx].T) / a).astype(np.float32)
        idx = idx[np.all((Yp >= FLT_MIN) & (Yp <= Y_MAX), axis=1)]
    assert idx.size >= N_ROWS, (lik, case, band, idx.size)
    idx = np.sort(rng.permutation(idx)[:N_ROWS])
    X = Xp[idx]
    z = _z64(spec, theta, X)
    if y_range is None and rho_range is None:
        Y = rng.gamma(a, c[None, :] * np.exp(z.T) / a)
        for _ in range(64):                    # (the second draw is independent of the first: a row may leave the range again)
            out = ~np.all((Y.astype(np.float32) >= FLT_MIN) & (Y.astype(np.float32) <= Y_MAX), axis=1)
            if not out.any():
                break
            Y[out] = rng.gamma(a, c[None, :] * np.exp(z.T[out]) / a)
        assert not out.any(), (lik, case, band)
    else:
        rg = y_range if y_range is not None else rho_range
        v = np.exp(rng.uniform(math.log(rg[0] * 1.001), math.log(rg[1] / 1.001), (N_ROWS, d_out)))
        Y = v if y_range is not None else v * np.exp(z.T)
    eta = np.asarray(eta0[:spec.n_hypers], dtype=np.float32)
    return Dataset(lik=lik, case=case, band=band, spec=spec, X=X, Y=Y.astype(np.float32), theta=theta, eta=eta, par={"a": a, "c": c}, mix=None)


# A Gamma dataset outside the matrix (keyword arguments of _build_gamma), on DENORMAL_CASES: fp32-denormal targets, which staging admits
# (include/tbnn.h) -- f just above the overflow of e^-f, rho of O(1) on both sides of 1, so that y = rho e^f lies below FLT_MIN on almost every
# element and a kernel that flushed a denormal target to 0 would turn rho into 0: tests/test_gpu_likelihood_edges.py test_denormal_targets
MEASURED = {"denormal-targets": dict(f_range=(-88.5, -87.5), rho_range=(0.05, 1.5))}
DENORMAL_CASES = ("fast3", "mid10", "lay_last")


def measured(case, kind):
    key = ("gamma", case, kind)
    if key not in _DATASETS:
        _DATASETS[key] = _build_gamma(case, kind, **MEASURED[kind])
    return _DATASETS[key]


def _build(lik, case, band):
    if lik == "gamma":
        return _build_gamma(case, band)
    dims, act, prior, Xp, theta0, eta0 = _pool(lik, case)
    names = case_names(lik, traj=True)
    i_ds = names.index(case) + list(BANDS[lik]).index(band)
    rng = np.random.default_rng(1000 * LIKS.index(lik) + 37 * names.index(case) + list(BANDS[lik]).index(band))
    d_out = dims[-1]
    par, mix = {}, None
    if lik == "student":
        nu, s, lo, hi = STUDENT_BANDS[band]
        spec = _spec(lik, dims, act, prior, s, nu)
        idx = np.sort(rng.permutation(POOL)[:N_ROWS])
        X, theta = Xp[idx], theta0
        z = _z64(spec, theta, X)
        u = np.exp(rng.uniform(math.log(lo * 1.001), math.log(hi / 1.001), (N_ROWS, d_out)))
        sg = np.array([_sign(i_ds, k) for k in range(d_out)])
        Y = (z.T + sg * o.student_scale(spec) * np.sqrt(nu * u)).astype(np.float32)
        par = {"nu": nu, "s": s}
    else:
        if lik == "negbin":
            sign, lo, hi = NEGBIN_BANDS[band]
            r = dispersion(case)
            par = {"r": r}
            shift = math.log(float(np.float32(r)))
            rg = (lo, hi) if sign == 0 else (lo, hi) if sign > 0 else (-hi, -lo)
            ranges = [(rg[0] + shift, rg[1] + shift)] * d_out
            if band.startswith("far"):
                # a last layer that spreads one output over three decades multiplies the hidden activations' own fp32 error by 1e6 / their
                # spread: relative to the rows near 1e3 that is more than the forward band.  Each output keeps to a third of a decade, so
                # that |W a| <= |z|, and the outputs take the decades in turn: output k over [hi / 3, hi] / 10^(k mod 3)
                ranges = [tuple(sorted((sign * hi / 3.0 / 10 ** (k % 3) + shift, sign * hi / 10 ** (k % 3) + shift))) for k in range(d_out)]
        elif lik == "hetero":
            sign, lo, hi = HETERO_BANDS[band]
            rg = ("sd", 18.5) if band == "straddle" else (lo, hi) if sign >= 0 else (-hi, -lo)
            ranges = [None, rg]
        elif band == "flush":
            ranges = [("sd", 8.3, -95.4)] if d_out == 1 else [FLUSH_TOP if k % 2 == 0 else FLUSH_BOTTOM for k in range(d_out)]
        else:
            ranges = [POISSON_BANDS[band]] * d_out
        spec = _spec(lik, dims, act, prior, df=par.get("r", 0.0))
        theta, z, amax = _placed(spec, theta0, Xp, ranges)
        if lik == "poisson" and band == "high":
            # the fp32 gradient slabs hold sums of e^f a over the rows: keep n max|a| e^(z_max) below FLT_MAX / 16 (still inside the band)
            top = min(80.0, math.log(FLT_MAX / 16.0 / (N_ROWS * max(amax, 1.0))) - 0.05)
            theta, z, amax = _placed(spec, theta0, Xp, [(60.0, top)] * d_out)
            ok = np.all((z >= 60.0) & (z <= top), axis=0)
        elif band == "flush" and d_out == 1:
            top = (z[0] >= FLUSH_TOP[0]) & (z[0] <= FLUSH_TOP[1])
            ok = top | ((z[0] >= FLUSH_BOTTOM[0]) & (z[0] <= FLUSH_BOTTOM[1]))
        elif band == "straddle":
            g = np.abs(z[1])
            ok = (g >= lo + 1e-3) & (g <= hi - 1e-3) & (np.abs(g - HETERO_CLIP) >= 1.2 * STRADDLE_DROP)
        else:
            ok = np.all([(z[k] >= rg_[0]) & (z[k] <= rg_[1]) for k, rg_ in enumerate(ranges) if rg_ is not None], axis=0)
        idx = np.flatnonzero(ok)
        if band == "straddle":
            # rows inside and outside the clip taken in turn: every 16-row tile holds both
            g = np.abs(z[1])
            ins, outs = rng.permutation(idx[g[idx] < HETERO_CLIP]), rng.permutation(idx[g[idx] > HETERO_CLIP])
            assert len(ins) >= (N_ROWS + 1) // 2 and len(outs) >= N_ROWS // 2, (lik, case, band, len(ins), len(outs))
            idx = np.empty(N_ROWS, np.int64)
            idx[0::2], idx[1::2] = ins[:(N_ROWS + 1) // 2], outs[:N_ROWS // 2]
        elif band == "flush" and d_out == 1:
            # one row in three just above FLT_MIN, two at the bottom of the denormals
            tops, bots = rng.permutation(idx[top[idx]]), rng.permutation(idx[~top[idx]])
            n_top = (N_ROWS + 2) // 3
            assert len(tops) >= n_top and len(bots) >= N_ROWS - n_top, (lik, case, band, len(tops), len(bots))
            idx = np.empty(N_ROWS, np.int64)
            third = np.arange(N_ROWS) % 3 == 0
            idx[third], idx[~third] = tops[:n_top], bots[:N_ROWS - n_top]
        else:
            assert idx.size >= N_ROWS, (lik, case, band, idx.size)
            idx = np.sort(rng.permutation(idx)[:N_ROWS])
        X = Xp[idx]
        z = _z64(spec, theta, X)
        if lik == "negbin":
            for mix in MIXES:
                Y = _counts(np.random.default_rng(rng.integers(1 << 30)), z, par["r"], mix)
                if ratio(o.negbin_elementwise(z, Y, par["r"], np.float64)[1]).max() <= 4.0:
                    break
        elif lik == "hetero":
            rho = np.exp(rng.uniform(math.log(1e-3), math.log(1e2), N_ROWS))
            Y = (z[0] + _sign(i_ds, 0) * rho).astype(np.float32)
        elif band == "flush":
            Y = np.zeros((N_ROWS, d_out), np.float32)
        elif band == "deep-":
            Y = np.where((np.arange(N_ROWS) % 4 == 3)[:, None], rng.integers(1, 4, (N_ROWS, d_out)), 0).astype(np.float32)
        else:
            Y = rng.choice([0.0, 1e3, 1e8], (N_ROWS, d_out)).astype(np.float32)
    eta = np.asarray(eta0[:spec.n_hypers], dtype=np.float32)          # no likelihood hyper
    return Dataset(lik=lik, case=case, band=band, spec=spec, X=X, Y=Y, theta=theta, eta=eta, par=par, mix=mix)


_DATASETS = {}


def dataset(lik, case, band):
    """computed once per process and left unchanged"""
    key = (lik, case, band)
    if key not in _DATASETS:
        _DATASETS[key] = _build(lik, case, band)
    return _DATASETS[key]


def all_keys():
    return [(lik, case, band) for lik in LIKS for case in case_names(lik) for band in BANDS[lik]]


# ---------------------------------------------------------------------------------------------------------------------- the references
def target(ds, dtype, w=None, theta=None, eta=None):
    """(log posterior, gradient) of the likelihood's reference in `dtype`"""
    th = ds.theta if theta is None else theta
    et = ds.eta if eta is None else eta
    with np.errstate(over="ignore", invalid="ignore"):
        return o.target_log_prob_and_grad(ds.spec, th, et, ds.X, ds.Y, dtype, w=w)


def statistic(ds, dtype, w=None):
    """what tbnn_logp_grad returns as `stat`, from the reference in `dtype` (Student-t: sum w log1p(u); the others: the data term with
    its constant, as the likelihood modules check it)"""
    dt = dtype
    f = o.forward(ds.spec, ds.theta.astype(dt), ds.X.astype(dt), dt)
    with np.errstate(over="ignore", invalid="ignore"):
        if ds.lik == "student":
            return o.data_statistic(ds.spec, ds.eta, f, ds.Y, dt, w)
        return float(o.log_likelihood(ds.spec, ds.eta.astype(dt), f, ds.Y, dt, w))


def deltas(ds):
    """the data term's derivative [d_out, n] on the fp64 reference, and the branch quantity [d_out or 1, n]"""
    z = _z64(ds.spec, ds.theta, ds.X)
    with np.errstate(over="ignore"):
        d = o.likelihood_grad(ds.spec, ds.eta, z, ds.Y, np.float64)
    if ds.lik == "student":
        s = o.student_scale(ds.spec)
        y = np.asarray(ds.Y, np.float64).reshape(z.shape[1], -1).T
        return d, (y - z) ** 2 / (ds.par["nu"] * s * s), z
    if ds.lik == "negbin":
        return d, z - math.log(float(np.float32(ds.par["r"]))), z
    if ds.lik == "gamma" and ds.band in ("small", "big"):          # rho = y e^-f (the log-means' own range: gamma_f_range)
        return d, np.asarray(ds.Y, np.float64).reshape(z.shape[1], -1).T * np.exp(-z), z
    return d, (z[1:2] if ds.lik == "hetero" else z), z


def in_band(ds, q):
    """the occupancy mask of the branch quantity q"""
    if ds.lik == "student":
        _nu, _s, lo, hi = STUDENT_BANDS[ds.band]
        return (q >= lo) & (q <= hi)
    if ds.lik == "poisson":
        lo, hi = POISSON_BANDS[ds.band]
        return (q >= lo) & (q <= hi)
    if ds.lik == "gamma":
        lo, hi = GAMMA_BANDS[ds.band][2] if ds.band in ("small", "big") else GAMMA_BANDS[ds.band][:2]
        return (q >= lo) & (q <= hi)
    sign, lo, hi = BANDS[ds.lik][ds.band]
    if ds.band == "straddle":
        return (np.abs(q) >= lo) & (np.abs(q) <= hi) & (np.abs(np.abs(q) - HETERO_CLIP) >= STRADDLE_DROP)
    if sign == 0:
        return (q >= lo) & (q <= hi)
    return (sign * q >= lo) & (sign * q <= hi)


def gaps(spec, lp, g, lp64, g64):
    """the suite's metrics: (value error / max(|lp64|, 1), per tensor: gradient error / max(|g64|_inf, 1e-3))"""
    return abs(lp - lp64) / max(abs(lp64), 1.0), tensor_errs(spec, g, g64, 1e-3)


def widened(project, gap):
    """the band rule: the project's band where the fp32 arm is inside half of it, else max(project band, 8 x the fp32 arm's gap)"""
    return project if gap <= 0.5 * project else max(project, 8.0 * gap)


_ARMS = {}


def arms(ds, w=None):
    """fp64 and fp32 arms at the dataset, once per process: dict(lp64, g64, st64, gv, gg, gs, bv, bg, bs) -- the fp32 arm's gaps against
    fp64 (value, per tensor, statistic) and the GPU bands they give"""
    key = (ds.lik, ds.case, ds.band, None if w is None else w.tobytes())
    if key not in _ARMS:
        lp64, g64 = target(ds, np.float64, w)
        lp32, g32 = target(ds, np.float32, w)
        st64, st32 = statistic(ds, np.float64, w), statistic(ds, np.float32, w)
        gv, gg = gaps(ds.spec, lp32, g32, lp64, g64)
        gs = abs(st32 - st64) / abs(st64)                  # (relative, as the likelihood modules check it)
        if w is not None:
            # integer weights re-weight the SAME rows: where a few rows carry the sum (r^2 u to 1e20 at the straddle), whether the fp32 arm's
            # gap shows depends on which of them drew the weight 0.  The band of a weighted run is therefore taken from the larger of the
            # fp32 arm's two gaps at this dataset, with the weights and without
            a0 = arms(ds)
            gv, gs, gg = max(gv, a0["gv"]), max(gs, a0["gs"]), [max(x, y) for x, y in zip(gg, a0["gg"])]
        _ARMS[key] = dict(lp64=lp64, g64=g64, st64=st64, lp32=lp32, g32=g32, st32=st32, gv=gv, gg=gg, gs=gs,
                          bv=widened(4e-6, gv), bg=[widened(1e-4, x) for x in gg], bs=widened(4e-6, gs))
    return _ARMS[key]
