"""The continuous ranked probability score of the predictive mixture (tbnn_ensemble_crps, include/tbnn.h) restated three ways, each written
from the definition and independent of the kernel, and the cases tests/test_crps_host.py and tests/test_gpu_crps.py share.  No test
functions here.

  ref40     the definition at 40 digits with mpmath, element by element: the reference of the band.  Networks of weight 0 are left out
            (their terms are exactly 0).
  crps_np   the plain fp64 NumPy restatement, vectorised: the full double sum over [m, m, elements] with scipy.special.erf.  Its own
            deviation from ref40 on the cases below is the yardstick the GPU band K is derived from (tests/test_crps_host.py prints it).
  crps_sorted   noise = 0 only: the O(m log m) form  spread = sum_k w_(k) f_(k) (2 C_k - w_(k) - 1)  over the sorted predictions, C_k the
            cumulative normalised weight.

Inputs everywhere: f [m, E] (the fp32 predictions, widened), s [m] or [m, E] or None (noise = 0), w [m] or None, y [E].

The unit of the band: per element u = 2^-53 (error_ref + spread_ref).  deviation_u returns |got - ref40| in that unit, the difference taken
at 40 digits, for all three outputs; an element whose unit is 0 (one network, no noise, the target on the prediction) must be met exactly
and reports 0 or inf.
"""
import math

import mpmath as mp
import numpy as np
import scipy.special as sp

import forward_ref as fr
import tbnn_oracle as o

U = 2.0 ** -53
DPS = 40
LOG_CLIP = math.log(1e8)

# the kernel's tiles (tensorbnn_amd/csrc/kernels_ensemble.hpp: ENS_CT networks per tile, ENS_CE elements per workgroup)
T, E = 8, 32
SHAPE_M = [1, 2, 3, T - 1, T, T + 1, 2 * T + 1]
SHAPE_ROWS = [1, E - 1, E + 1, 517]
GAUSS, FIXED, HETERO = o.LIK_GAUSSIAN, o.LIK_FIXED_GAUSSIAN, o.LIK_HETERO_GAUSSIAN
DIMS = {GAUSS: [2, 8, 3], FIXED: [2, 8, 1], HETERO: [2, 8, 2]}
FIXED_SD = 0.7


# ------------------------------------------------------------------------------------------------------------------ the three restatements
def clip_sd(sd):
    """sd as the library reads it: clipped to [1e-8, 1e8] in fp32, widened"""
    return np.clip(np.asarray(sd, dtype=np.float32), np.float32(1e-8), np.float32(1e8)).astype(np.float64)


def hetero_scale(g):
    """s = exp(gc), gc the fp32 log-sd output clipped to +-log(1e8), in fp64"""
    return np.exp(np.clip(np.asarray(g, dtype=np.float64), -LOG_CLIP, LOG_CLIP))


def _abs_normal_mp(mu, sigma):
    z = mu / sigma
    return sigma * (2 * mp.npdf(z) + z * mp.erf(z / mp.sqrt(2)))


def ref40(f, s, w, y):
    """(crps, error, spread), object arrays [E] of mpf at 40 digits.  s None: noise = 0, A(mu, 0) = |mu|.  s [m] or [m, E] as exact
    doubles (heteroscedastic kind: pass gc, clipped, with hetero=True semantics through ref40_hetero)"""
    return _ref40(f, s, w, y, False)


def ref40_hetero(f, g, w, y, noise=True):
    """the heteroscedastic kind: g [m, E] the fp32 log-sd outputs; s = exp(clip(g)) formed at 40 digits"""
    return _ref40(f, np.clip(np.asarray(g, dtype=np.float64), -LOG_CLIP, LOG_CLIP) if noise else None, w, y, True)


def _ref40(f, s, w, y, log_scale):
    with mp.workdps(DPS):
        f = np.asarray(f, dtype=np.float64)
        m, n = f.shape
        wv = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
        W = mp.fsum(mp.mpf(float(x)) for x in wv)
        om = [mp.mpf(float(x)) / W for x in wv]
        keep = [i for i in range(m) if wv[i] > 0]
        if s is not None:
            s = np.broadcast_to(np.asarray(s, dtype=np.float64).reshape(m, -1), (m, n))
        out = np.empty((3, n), dtype=object)
        for e in range(n):
            fe = [mp.mpf(float(f[i, e])) for i in range(m)]
            ye = mp.mpf(float(y[e]))
            if s is None:
                err = mp.fsum(om[i] * abs(ye - fe[i]) for i in keep)
                spr = mp.fsum(om[i] * om[j] * abs(fe[i] - fe[j]) for a, i in enumerate(keep) for j in keep[:a])
            else:
                se = [mp.exp(mp.mpf(float(s[i, e]))) if log_scale else mp.mpf(float(s[i, e])) for i in range(m)]
                v = [x * x for x in se]
                err = mp.fsum(om[i] * _abs_normal_mp(ye - fe[i], se[i]) for i in keep)
                spr = mp.fsum(om[i] * om[j] * _abs_normal_mp(fe[i] - fe[j], mp.sqrt(v[i] + v[j])) for a, i in enumerate(keep) for j in keep[:a])
                spr += mp.fsum(om[i] * om[i] * se[i] for i in keep) / mp.sqrt(mp.pi)      # the diagonal: 1/2 A(0, s sqrt 2) = s / sqrt pi
            out[:, e] = (err - spr, err, spr)
        return out[0], out[1], out[2]


def abs_normal(mu, sigma):
    """A(mu, sigma) = sigma [2 phi(z) + z erf(z / sqrt 2)], z = mu / sigma, in fp64"""
    z = mu / sigma
    return sigma * (2.0 * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) + z * sp.erf(z / math.sqrt(2.0)))


def crps_np(f, s, w, y):
    """the fp64 restatement: (crps, error, spread), float64 [E].  s None: noise = 0"""
    f = np.asarray(f, dtype=np.float64)
    m, n = f.shape
    wv = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
    om = wv / wv.sum()
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = f[:, None, :] - f[None, :, :]
        if s is None:
            a_err, a_pair = np.abs(y[None] - f), np.abs(d)
        else:
            s = np.broadcast_to(np.asarray(s, dtype=np.float64).reshape(m, -1), (m, n))
            a_err = abs_normal(y[None] - f, s)
            a_pair = abs_normal(d, np.sqrt(s[:, None, :] ** 2 + s[None, :, :] ** 2))
        # (a network of weight 0 adds nothing, whatever it holds)
        a_err = np.where(om[:, None] > 0, a_err, 0.0)
        a_pair = np.where((om[:, None, None] > 0) & (om[None, :, None] > 0), a_pair, 0.0)
    err = (om[:, None] * a_err).sum(axis=0)
    spr = 0.5 * (om[:, None, None] * om[None, :, None] * a_pair).sum(axis=(0, 1))
    return err - spr, err, spr


def crps_sorted(f, w, y):
    """noise = 0 through the sorted predictions: (crps, error, spread), float64 [E]"""
    f = np.asarray(f, dtype=np.float64)
    m, n = f.shape
    wv = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
    om = wv / wv.sum()
    order = np.argsort(f, axis=0, kind="stable")
    fs = np.take_along_axis(f, order, axis=0)
    ws = om[order]
    C = np.cumsum(ws, axis=0)
    spr = (ws * fs * (2.0 * C - ws - 1.0)).sum(axis=0)
    err = (om[:, None] * np.abs(np.asarray(y, dtype=np.float64)[None] - f)).sum(axis=0)
    return err - spr, err, spr


def deviation_u(got, ref):
    """got: three float64 arrays [E]; ref: ref40's three.  float64 [3, E]: |got - ref| / (2^-53 (error_ref + spread_ref)), at 40 digits"""
    out = np.empty((3, len(ref[0])))
    with mp.workdps(DPS):
        for e in range(out.shape[1]):
            unit = mp.mpf(U) * (ref[1][e] + ref[2][e])
            for k in range(3):
                d = abs(mp.mpf(float(got[k][e])) - ref[k][e])
                out[k, e] = float(d / unit) if unit > 0 else (0.0 if d == 0 else math.inf)
    return out


# --------------------------------------------------------------------------------------------------------------------------- the cases
def weights_with_zeros(m, seed=1):
    """gamma-distributed importance weights, every third network (from the second) at weight 0; one network: 2"""
    w = np.random.default_rng(seed).gamma(0.7, size=m).astype(np.float32) + np.float32(0.01)
    w[1::3] = 0.0
    if m == 1:
        w[0] = 2.0
    return w


def sds(m, seed=2):
    """per-network standard deviations over two decades"""
    s = 10.0 ** np.linspace(-1.5, 0.5, m) if m > 1 else np.array([0.4])
    return np.random.default_rng(seed).permutation(s).astype(np.float32)


def shape_cases():
    """(kind, m, rows, noise, weighted): the shapes crossed, under TBNN_LIK_GAUSSIAN with per-network sd on a 2-8-1 network; weighted at every
    second row count"""
    return [(FIXED, m, rows, True, rows in (E - 1, 517)) for m in SHAPE_M for rows in SHAPE_ROWS]


def kind_cases():
    """(kind, m, rows, noise, weighted): every kind and option at m = T + 1 over E + 1 rows"""
    return [(kind, T + 1, E + 1, noise, weighted) for kind in (GAUSS, FIXED, HETERO) for noise in (True, False) for weighted in (False, True)]


def case_problem(kind, m, rows, seed=None):
    """(spec, X, thetas): the tiny tanh network of the kind, 2-8-d_out; the heteroscedastic kind's log-sd biases spread over [-2.5, 0.5]"""
    dims = DIMS[kind]
    seed = 1000 * m + rows + 7 * kind if seed is None else seed
    spec, X, thetas = fr.problem(dims, o.ACT_TANH, o.ACT_NONE, m, rows, seed)
    if kind == HETERO:
        thetas[:, -1] = np.random.default_rng(seed + 1).uniform(-2.5, 0.5, m).astype(np.float32)
    return spec, X, thetas


def case_targets(f, kind, seed):
    """targets [rows, d] fp32 around a randomly picked network's prediction, a standard deviation or so away"""
    m, d_out, n = f.shape
    d = 1 if kind == HETERO else d_out
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, m, n)
    centre = f[pick, :d, np.arange(n)].astype(np.float64)                  # [n, d]
    return (centre + 0.8 * rng.standard_normal((n, d))).astype(np.float32)


def case_reference(f, Y, kind, noise, sd, w):
    """(ref40 of every element, crps_np of every element) for predictions f [m, d_out, rows] fp32 and targets Y [rows, d]: each three arrays
    [od * rows], plane by plane.  sd: the per-network sd's (Gaussian kinds), not read otherwise"""
    m, d_out, n = f.shape
    f64 = f.astype(np.float64)
    if kind == HETERO:
        y = Y.reshape(n, -1)[:, 0].astype(np.float64)
        r40 = ref40_hetero(f64[:, 0], f64[:, 1], w, y, noise)
        rnp = crps_np(f64[:, 0], hetero_scale(f64[:, 1]) if noise else None, w, y)
        return r40, rnp
    fe = f64.reshape(m, d_out * n)
    y = Y.reshape(n, d_out).T.astype(np.float64).reshape(-1)
    s = clip_sd(sd) if noise else None
    return ref40(fe, s, w, y), crps_np(fe, s, w, y)
