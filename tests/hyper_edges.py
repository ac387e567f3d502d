"""What the hyper-edge modules share (tests/test_hyper_edges_host.py on the CPU, tests/test_gpu_hyper_edges.py on the device): values of the
hyper vector eta away from where a chain starts, a Python restatement of the hyper kernel's wave plan, the size of what each entry of the
hyper gradient sums, a step size per case, and the bands.

eta holds, per dense layer, (loc_w, g_w, loc_b, g_b) with scale = g^2, then the root of the Gaussian likelihood's sd.  Every g of an edge is a
power of two: g g is exact in fp32, so the kernels and the fp64 oracle stand on the same side of every clamp of (1e-8, 1e8).  Within a layer
g_b = g_w / 2 and loc_b = -loc_w: the two prior groups of a layer never share a value.

Bands (none measured on the code under test).  Weight target: 4e-6 relative, 1e-4 of each tensor's inf-norm (tests/test_gpu_depth.py).  Hyper
value: 4e-6 |lp64| + 1e-3 (tests/test_gpu_parity.py).  Hyper gradient, per entry j: 2e-4 |g64_j| + 4e-6 T_j, T_j the sum of the absolute
summands of the entry (hyper_grad_terms): g g rounded to fp32 moves a summand in s^-3 by 2e-7 of itself, 4e-6 is 20 times that.  A clamped entry
has T_j = the hyper-prior pull alone, and the data term's clamped entry has band 0: the gradient there is exactly 0.  Log accept ratio:
2e-2 + 1e-4 |lar| + 4e-7 |lp64|.  eta after an accepted step: 1e-4 per entry; theta: 1e-5 of the state's size."""
import numpy as np

import tbnn_oracle as o

LOGP_RTOL, GRAD_TOL = 4e-6, 1e-4
HYP_WAVES, HYP_REG = 16, 20                    # kernels_hyper.hpp
HELD_MAX = HYP_REG * 64                        # a wave holds a share of at most 1280 elements in registers


# ---------------------------------------------------------------- eta at the edges
def _every_layer(eta, n_layers, g=None, loc=None):
    e = np.array(eta, dtype=np.float64)
    for l in range(n_layers):
        if g is not None:
            e[4 * l + 1], e[4 * l + 3] = g, g / 2
        if loc is not None:
            e[4 * l], e[4 * l + 2] = loc, -loc
    return e


def _g(v, sd_root=None):
    def f(spec, eta, S):
        e = _every_layer(eta, len(spec.layers), g=v)
        if sd_root is not None and spec.likelihood == o.LIK_GAUSSIAN:
            e[-1] = sd_root
        return e
    return f


def _sd(v):
    def f(spec, eta, S):
        e = np.array(eta, dtype=np.float64)
        e[-1] = v
        return e
    return f


def _sd_mle(spec, eta, S):
    """the sd at which the data term's hyper gradient -n/s + S/s^3 cancels: s^2 = S / (n d_out)"""
    e = np.array(eta, dtype=np.float64)
    e[-1] = float(np.float32((S[0] / S[1]) ** 0.25))
    return e


ETA_EDGES = {
    "default": lambda spec, eta, S: np.array(eta, dtype=np.float64),
    "neg_g": _g(-0.5, sd_root=-0.25),
    "loc": lambda spec, eta, S: _every_layer(eta, len(spec.layers), loc=0.5),
    "small": _g(2.0 ** -5), "large": _g(2.0 ** 5), "tiny": _g(2.0 ** -10),
    "in_lo": _g(2.0 ** -13), "clamp_lo": _g(2.0 ** -14),          # scales 1.5e-8 / 3.7e-9: either side of 1e-8
    "in_hi": _g(2.0 ** 13), "clamp_hi": _g(2.0 ** 14),            # 6.7e7 / 2.7e8: either side of 1e8
    "sd_small": _sd(2.0 ** -10), "sd_in_lo": _sd(2.0 ** -13), "sd_clamp_lo": _sd(2.0 ** -14),
    "sd_large": _sd(2.0 ** 5), "sd_in_hi": _sd(2.0 ** 13), "sd_clamp_hi": _sd(2.0 ** 14),
    "sd_mle": _sd_mle,
}
KEEP = ("neg_g", "clamp_lo", "clamp_hi", "sd_mle")                # never dropped from a test
# Dropped from the hyper TRANSITION (they stay in every other test): at sd_small and sd_in_lo the target is -S / (2 el^4) ~ 1e14 and 4e17, and
# rounding the sd root el to fp32 once moves it by 4 * 6e-8 of itself, 2e7 and 9e10 -- the size of the band's 4e-7 |lp64| term.  The fp32
# oracle's log accept ratio is off by 5.8e7 (band 3.8e7) and 2.4e11 (band 1.6e11) there: no fp32 state can meet the band, so the cases go.
HYPER_STEP_DROPPED = ("sd_small", "sd_in_lo")
HYPER_STEP_EDGES = [k for k in ETA_EDGES if k not in HYPER_STEP_DROPPED]
WEIGHT_STEP_EDGES = ("neg_g", "small", "sd_small")                # injected weight transitions
HANDOVER_EDGES = ("sd_small", "sd_clamp_lo", "sd_clamp_hi")       # a weight transition behind an accepted hyper step
assert not set(HYPER_STEP_DROPPED) & set(KEEP) and len(HYPER_STEP_DROPPED) <= 2


def residual_ss(spec, theta, X, Y):
    """(S, n d_out): the squared residuals of the fp64 forward pass, and how many there are"""
    f = o.forward(spec, np.asarray(theta, np.float64), np.asarray(X, np.float64), np.float64)
    y = np.asarray(Y, np.float64).reshape(f.shape[1], -1).T
    return float(np.sum((y - f) ** 2)), f.size


def eta_at(name, spec, eta, theta=None, X=None, Y=None):
    """the edge `name` of a default eta, as the fp32 vector a chain takes"""
    S = residual_ss(spec, theta, X, Y) if name == "sd_mle" else None
    return ETA_EDGES[name](spec, eta, S).astype(np.float32)


# ---------------------------------------------------------------- the wave plan of k_hyper
def group_sizes(dims):
    """W_0, b_0, W_1, b_1, ..."""
    out = []
    for a, b in zip(dims[:-1], dims[1:]):
        out += [a * b, b]
    return out


def hyper_plan(dims):
    """hyper_plan of kernels_hyper.hpp restated: 16 waves, one per prior group, the spare ones to whichever group has the largest share per
    wave (the first such group on a tie); from 17 groups on, groups 15 .. are folded into wave 15 and re-read memory.
    -> (per group: dict(waves, shares, held, reread, empty), the folded groups)"""
    cnt = group_sizes(dims)
    ng = len(cnt)
    direct = ng if ng <= HYP_WAVES else HYP_WAVES - 1
    nw = [1 if g < direct else 0 for g in range(ng)]
    for _ in range(HYP_WAVES - ng if ng <= HYP_WAVES else 0):
        loads = [(cnt[g] + nw[g] - 1) // nw[g] for g in range(direct)]
        nw[loads.index(max(loads))] += 1
    plan = []
    for g in range(ng):
        shares = [cnt[g] * (k + 1) // nw[g] - cnt[g] * k // nw[g] for k in range(nw[g])]
        plan.append(dict(waves=nw[g], shares=shares, held=sum(0 < s <= HELD_MAX for s in shares),
                         reread=sum(s > HELD_MAX for s in shares), empty=sum(s == 0 for s in shares)))
    return plan, list(range(direct, ng))


# the shapes that put the plan at the register limit (tests/test_hyper_edges_host.py asserts the facts noted beside them)
PLAN_SHAPES = {
    "held_at_limit": [128, 130, 1],                               # W_0: 13 waves of exactly 1280
    "mixed_paths": [129, 129, 1],                                 # W_0: 12 waves of 1280 held, one of 1281 re-read
    "sixteen_groups": [4, 16, 16, 16, 16, 40, 32, 61, 21],        # one wave each; 1280 held, 1281 and 1952 re-read
    "folded": [4, 16, 16, 16, 16, 40, 32, 61, 21, 1],             # groups 15 .. 17 in wave 15
    "empty_waves": [3, 1, 1, 1],                                  # W_0 of 3 elements over 11 waves
}


# ---------------------------------------------------------------- the hyper gradient: value, clamps, size of the sums
def hyper_grad_terms(spec, eta, theta, X, Y):
    """per hyper entry: the sum of |summand| of o.hyper_log_prob_and_grad's gradient in fp64, the hyper-prior pull and the 2 g factor included"""
    eta = np.asarray(eta, np.float64)
    T = np.zeros_like(eta)
    for i, (l, (W, b)) in enumerate(zip(spec.layers, o.unflatten(spec, np.asarray(theta, np.float64)))):
        for j, x in ((0, W), (2, b)):
            loc, gg = eta[4 * i + j], eta[4 * i + j + 1]
            scale = gg * gg
            if l.prior == o.PRIOR_CAUCHY:
                z = (x - loc) / scale
                u = 2.0 * z / (1.0 + z * z)
                t_loc = np.sum(np.abs(u / scale)) + abs(loc) / 0.2 ** 2
                t_scale = np.sum(np.abs(u * z / scale) + 1.0 / scale) + abs(scale - 0.5 ** 0.5) / 0.5 ** 2
            else:
                s = min(max(scale, 1e-8), 1e8)
                clamped = not (1e-8 < scale < 1e8)
                t_loc = np.sum(np.abs((x - loc) / (s * s))) + abs(loc) / 0.1 ** 2
                t_scale = (0.0 if clamped else 1.0 / s + np.sum((x - loc) ** 2) / s ** 3) + abs(scale - 1.0) / 0.1 ** 2
            T[4 * i + j] = t_loc
            T[4 * i + j + 1] = t_scale * abs(2.0 * gg)
    if spec.likelihood == o.LIK_GAUSSIAN:
        S, n_el = residual_ss(spec, theta, X, Y)
        sr = eta[-1] ** 2
        s = min(max(sr, 1e-8), 1e8)
        T[-1] = 0.0 if not (1e-8 < sr < 1e8) else (n_el / s + S / s ** 3) * abs(2.0 * eta[-1])
    return T


def clamped_entries(spec, eta):
    """the g entries (and the sd root) whose clamped scale gives the prior / data part of the gradient as exactly 0"""
    eta = np.asarray(eta, np.float64)
    out = []
    for i, l in enumerate(spec.layers):
        if l.prior == o.PRIOR_GAUSSIAN:
            out += [4 * i + j for j in (1, 3) if not (1e-8 < eta[4 * i + j] ** 2 < 1e8)]
    if spec.likelihood == o.LIK_GAUSSIAN and not (1e-8 < eta[-1] ** 2 < 1e8):
        out.append(eta.size - 1)
    return out


def pull_alone(spec, eta):
    """per entry of clamped_entries: the gradient that is left, the hyper-prior pull times 2 g (0 for the sd root, which has no hyper-prior)"""
    eta = np.asarray(eta, np.float64)
    return {j: (0.0 if j == eta.size - 1 and spec.likelihood == o.LIK_GAUSSIAN else -(eta[j] ** 2 - 1.0) / 0.1 ** 2 * 2.0 * eta[j])
            for j in clamped_entries(spec, eta)}


def hyper_value_band(lp64):
    return LOGP_RTOL * abs(lp64) + 1e-3


def hyper_grad_band(g64, T):
    return 2e-4 * np.abs(np.asarray(g64, np.float64)) + 4e-6 * np.asarray(T, np.float64)


def lar_band(lar64, lp64):
    return 2e-2 + 1e-4 * abs(lar64) + 4e-7 * abs(lp64)


def hyper_grad_ratio(g, g64, T):
    """the worst error of a hyper gradient in units of its per-entry band; an entry whose band is 0 must be met exactly (inf otherwise)"""
    err = np.abs(np.asarray(g, np.float64) - np.asarray(g64, np.float64))
    band = hyper_grad_band(g64, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(band > 0, err / band, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def check_hyper_target(lp, g, spec, eta, theta, X, Y, what=""):
    """value and gradient of the hyper target against the fp64 oracle; -> (value error over its band, worst gradient error over its band)"""
    lp64, g64 = o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64)
    T = hyper_grad_terms(spec, eta, theta, X, Y)
    r_v = abs(lp - lp64) / hyper_value_band(lp64)
    r_g = hyper_grad_ratio(g, g64, T)
    assert r_v <= 1.0, (what, "hyper value", lp, lp64)
    assert r_g <= 1.0, (what, "hyper gradient", np.asarray(g), g64, hyper_grad_band(g64, T))
    for j, want in pull_alone(spec, eta).items():                 # one rounding of the fp64 pull to fp32, and 0.1^2 against 0.01
        assert abs(float(g[j]) - want) <= 2.0 * np.spacing(np.float32(abs(want))) or want == 0.0 and g[j] == 0.0, (what, "clamped entry", j, g[j], want)
    return r_v, r_g


# ---------------------------------------------------------------- a step size per case
_EPS = {}


def _moves(new, old, kind):
    d = np.abs(np.asarray(new, np.float64) - np.asarray(old, np.float64))
    if kind == "hyper":                                            # per entry; a location that starts at 0 is measured against 1
        ref = np.abs(np.asarray(old, np.float64))
        return float(np.max(d / np.where(ref > 0, ref, 1.0)))
    return float(d.max() / np.abs(old).max())                      # a weight against the state's size


def pick_eps(key, kind, spec, eta, theta, X, Y, L, p0):
    """the largest power of two at which an accepted fp64 transition of L steps moves its state by at most 1e-2 (relative: _moves; a weight
    transition: 1e-3, a longer one takes the energy through zero at the small scales, where an error relative to it means nothing); the
    move is then at least 1e-4, asserted.  From the fp64 oracle alone; computed once per key."""
    if (key, kind) not in _EPS:
        S = residual_ss(spec, theta, X, Y)[0]

        def move(eps):
            with np.errstate(all="ignore"):
                if kind == "hyper":
                    r = o.hyper_step(spec, eta, theta, X, Y, eps, L, p0, -1e30, np.float64, S=S)
                    return _moves(r.theta_proposed, eta, kind) if np.isfinite(r.logp_new) else np.inf
                r = o.weight_step(spec, theta, eta, X, Y, eps, L, p0, -1e30, np.float64)
                return _moves(r.theta_proposed, theta, kind) if np.isfinite(r.logp_new) else np.inf
        eps = 2.0 ** -4
        m = move(eps)
        while not m <= (1e-2 if kind == "hyper" else 1e-3):
            eps *= 0.5
            m = move(eps)
            assert eps > 1e-40, (key, kind)
        assert m >= 1e-4, (key, kind, eps, m)
        _EPS[(key, kind)] = float(np.float32(eps))
    return _EPS[(key, kind)]


# ---------------------------------------------------------------- the small problems both modules judge
_PROBLEMS = {}
PRIORS = {"cauchy": o.PRIOR_CAUCHY, "gaussian": o.PRIOR_GAUSSIAN, "mix": None}      # mix: Cauchy and Gaussian layer by layer


def small_problem(dims, n, prior, seed=21):
    """tanh hidden layers, activations O(1), Gaussian likelihood: (spec, X, Y, theta, default eta); computed once and never modified"""
    key = (tuple(dims), n, prior, seed)
    if key not in _PROBLEMS:
        from test_gpu_layered import scaled_problem
        spec, X, Y, theta, _ = scaled_problem(dims, n, [o.ACT_TANH] * (len(dims) - 2), o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, seed=seed)
        for k, l in enumerate(spec.layers):
            l.prior = (o.PRIOR_GAUSSIAN if k % 2 else o.PRIOR_CAUCHY) if PRIORS[prior] is None else PRIORS[prior]
        _PROBLEMS[key] = (spec, X, Y, theta, o.default_hypers(spec, 0.1))
    return _PROBLEMS[key]


def momenta(spec, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(spec.n_params).astype(np.float32), rng.standard_normal(spec.n_hypers).astype(np.float32)
