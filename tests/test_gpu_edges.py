"""GPU: the fused kernels at the edges the other modules keep away from, against the fp64 oracle through the C ABI.

Every other module builds its network with the last activation "none" (Gaussian) or "sigmoid" (Bernoulli) and keeps Bernoulli outputs off
saturation.  Here:
  (a) every last-layer activation network.add accepts (relu, tanh, sigmoid, exp, elu) on every family, with <= 2 and (MFMA last layer) 3 .. 16
      outputs, and Bernoulli on raw outputs (no last activation: clipped on both sides);
  (b) exp as a hidden activation (its padded slots hold exp(0) = 1, not 0), uniform and in a per-layer mix;
  (c) saturated Bernoulli: pre-activations over [-30, 30], rows exactly on the clip's upper bound float32(1 - 1e-7) = 1 - 2^-23 (where the
      gradient passes, as it does through tf.clip_by_value), clipped above and below, with 1, 2 and >= 3 outputs, and one injected transition on the
      trajectory kernel;
  (d) the fast activations' special cases (tanh's series / exp switch and overflow, sigmoid's overflow, elu far below 0, relu exactly at 0);
  (e) the reference's classification example at full size (mn_burned.npz) on the kernel the bench runs.
Each case: log-prob, gradient per tensor and forward (forward, predict, forward_many over every row) against fp64 at the fuzz tolerances
(test_gpu_fuzz.py), every launch three times and bit-identical, and the kernel name naming the family and the last activation."""
import os

import numpy as np
import pytest

import tbnn_oracle as o
from tensor_checks import layers_of, tensor_err
from test_gpu_layered import scaled_problem

pytestmark = pytest.mark.gpu

R, T, S, X_, E, N = o.ACT_RELU, o.ACT_TANH, o.ACT_SIGMOID, o.ACT_EXP, o.ACT_ELU, o.ACT_NONE
AN = {N: "none", R: "relu", T: "tanh", S: "sigmoid", X_: "exp", E: "elu"}
GAUSS, BERN = o.LIK_GAUSSIAN, o.LIK_BERNOULLI
# family -> TBNN_JIT_SKIP, kernel-name prefix
FAM = {"fast3": ("mid,tall,wide", "jit-fast3"), "fast": ("fast3,mid,tall,wide", "jit-fast<"), "mid": ("fast3,fast,tall,wide", "jit-mid"),
       "tall": ("fast3,fast,mid,wide", "jit-tall"), "wide": ("fast3,fast,mid,tall", "jit-wide"),
       "layered": ("fast3,fast,mid,tall,wide", "layered<")}
# architectures the suite already builds (test_gpu_mixedact.CASES, tests/fuzz_shapes.py): <= 2 outputs, and 3 .. 16 outputs
DIMS = {"fast3": ([5, 20, 24, 1], None), "fast": ([4, 17, 9, 2], [4, 17, 9, 3]), "mid": ([20, 64, 64, 2], [10, 91, 20, 3]),
        "tall": ([100, 50, 50, 1], [300, 20, 20, 10]), "wide": ([10, 200, 120, 1], [31, 169, 160, 10]), "layered": ([5, 20, 24, 1], [5, 20, 24, 3])}
B_LO, B_HI = np.float32(1e-8), np.float32(1 - 1e-7)
LOG = []                                    # measured forward errors of (d), printed as they are measured


def env(monkeypatch, fam):
    monkeypatch.setenv("TBNN_JIT_SKIP", FAM[fam][0])
    if fam == "layered":
        monkeypatch.setenv("TBNN_TALL", "0")
        monkeypatch.setenv("TBNN_MID", "0")
        monkeypatch.setenv("TBNN_REGISTERED", "0")          # (a library another case registered for the same shape)


def ref_logp(spec, theta, eta, X, Y):
    """fp64 target with the Bernoulli clip at the kernels' fp32 bounds (1 - 1e-7 is 1 - 2^-23 in fp32: log(1 - p) on a clipped row
    differs by 0.18 between the two constants)"""
    lp = o.target_log_prob(spec, theta, eta, X, Y, np.float64)
    if spec.likelihood != BERN:
        return lp
    f = o.forward(spec, theta, X, np.float64)
    y = np.asarray(Y, np.float64).reshape(-1, f.shape[0]).T
    p = np.clip(f, float(B_LO), float(B_HI))
    lik = np.sum(np.where(y == 0, 0.0, y * np.log(p)) + np.where(y == 1, 0.0, (1 - y) * np.log1p(-p)))
    return lp - o.log_likelihood(spec, eta, f, Y, np.float64) + lik


def ulp_slack(spec, theta, X, Y):
    """the log-prob an ulp-level difference in p may move: 2 ulp(p) / p (label 1) or / (1 - p) (label 0) per unclipped (row, output) --
    near p -> 1, log(1 - p) amplifies the last bits of p in any fp32 evaluation, the reference's included"""
    if spec.likelihood != BERN:
        return 0.0
    f = o.forward(spec, theta, X, np.float64)
    y = np.asarray(Y, np.float64).reshape(-1, f.shape[0]).T
    inside = (f >= float(B_LO)) & (f <= float(B_HI))
    u = 2.0 * np.spacing(np.abs(f).astype(np.float32)).astype(np.float64)
    with np.errstate(divide="ignore"):
        return float(np.sum(np.where(inside, u / np.where(y == 1, f, 1.0 - f), 0.0)))


def run(native, monkeypatch, fam, spec, X, Y, theta, eta, *, ens=True):
    """value, gradient and every forward path of the chain `fam` runs on, each launch three times and bit-identical"""
    env(monkeypatch, fam)
    ch = native.Chain(layers_of(spec), likelihood=spec.likelihood, fixed_sd=spec.fixed_sd, jit=fam != "layered")
    try:
        name = ch.kernel_name
        assert name.startswith(FAM[fam][1]), f"{fam}: runs on {name}"
        if fam != "layered":           # (the layered family's name lists the widths only)
            tag = "," + AN[spec.layers[-1].act] + (",bernoulli;" if spec.likelihood == BERN else ";")
            assert tag in name, f"{name}: not the last activation {tag}"
        ch.set_data(X, Y)
        lp, g, _ = ch.logp_grad(theta, eta)
        f, pr = ch.forward(X, theta), ch.predict(0, theta)
        th2 = np.stack([theta, (theta * np.float32(0.97)).astype(np.float32)]) if ens else None
        fm = ch.forward_many(th2, None, which=0) if ens else None
        for _ in range(2):
            lp2, g2, _ = ch.logp_grad(theta, eta)
            assert lp2 == lp and np.array_equal(g2, g), f"{name}: a repeated launch differs (max {np.abs(g2 - g).max():.3e})"
            assert np.array_equal(ch.forward(X, theta), f) and np.array_equal(ch.predict(0, theta), pr), f"{name}: a repeated forward differs"
            if ens:
                assert np.array_equal(ch.forward_many(th2, None, which=0), fm), f"{name}: a repeated forward_many differs"
    finally:
        ch.close()
    return name, lp, g, f, pr, (th2, fm)


def check(native, monkeypatch, fam, spec, X, Y, theta, eta, ens=True):
    name, lp, g, f, pr, (th2, fm) = run(native, monkeypatch, fam, spec, X, Y, theta, eta, ens=ens)
    g64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[1]
    lp64 = ref_logp(spec, theta, eta, X, Y)
    tol_lp = 4e-6 * max(abs(lp64), 1.0) + ulp_slack(spec, theta, X, Y)
    assert abs(lp - lp64) <= tol_lp, f"{name}: logp {lp} against {lp64} (bound {tol_lp:.3e})"
    e_g = tensor_err(spec, g, g64, 1e-3)
    assert e_g <= 1e-4, f"{name}: gradient {e_g:.3e} of the tensor's inf-norm (1e-4)"
    f64 = o.forward(spec, theta, X, np.float64)
    fwd_tol = 1e-4 * np.maximum(1.0, np.abs(f64))                    # (exp outputs: relative above 1)
    assert np.all(np.isfinite(f)) and np.all(np.abs(f - f64) <= fwd_tol), f"{name}: forward {np.abs(f - f64).max():.3e}"
    assert np.all(np.abs(pr - f64) <= fwd_tol), f"{name}: predict {np.abs(pr - f64).max():.3e}"
    if ens:
        for k in range(2):
            fk = o.forward(spec, th2[k], X, np.float64)
            assert np.all(np.abs(fm[k] - fk) <= 1e-4 * np.maximum(1.0, np.abs(fk))), f"{name}: forward_many[{k}] {np.abs(fm[k] - fk).max():.3e}"
    return name, lp, g, f


# ------------------------------------------------------------------------------------------------ (a) the last layer's activation
def last_problem(dims, n, hidden, last, lik, seed=0):
    """the last layer rescaled so that its pre-activations z sit where its activation bends: mean / sd per output 0.5 / 0.75 for raw Bernoulli
    outputs (clipped on both sides), 0 / 0.7 under exp, 0 / 1 otherwise (outputs O(1), tanh off its flat tails: a well-conditioned fp32 problem)"""
    spec, X, Y, theta, eta = scaled_problem(dims, n, [hidden] * (len(dims) - 2), o.PRIOR_CAUCHY, lik, seed)
    spec.layers[-1].act = N
    mean, sd = (0.5, 0.75) if lik == BERN else (0.0, 0.7) if last == X_ else (0.0, 1.0)
    ow, ob = spec.offsets()[-1]
    z = o.forward(spec, theta, X, np.float64)
    sc = sd / z.std(axis=1)
    theta = theta.copy()
    theta[ow:ob] = (theta[ow:ob].reshape(dims[-1], -1) * sc[:, None]).reshape(-1)
    theta[ob:ob + dims[-1]] = mean + (theta[ob:ob + dims[-1]] - z.mean(axis=1)) * sc
    z = o.forward(spec, theta, X, np.float64)
    spec.layers[-1].act = last
    if lik == BERN:
        # raw outputs: keep the rows whose outputs are clearly clipped or clearly inside (fp32 and fp64 decide the clip alike; 1/p stays O(1))
        keep = np.all((z < -1e-3) | (z > 1 + 1e-3) | ((z > 0.1) & (z < 0.9)), axis=0)
    elif last == R:
        keep = np.all(np.abs(z) > 1e-3, axis=0)          # (no relu kink at the last layer: its fp32 sign would follow the summation order)
    else:
        keep = np.ones(X.shape[0], bool)
    X, z = X[keep], z[:, keep]
    if X.shape[0] % 16 == 0:                             # a tail
        X, z = X[:-1], z[:, :-1]
    if lik == BERN:
        Y = (np.random.default_rng(7 + seed).random((X.shape[0], dims[-1])) < 0.5).astype(np.float32)      # labels independent of z
        assert (z > 1).sum() >= 20 and (z < 0).sum() >= 20 and ((z > 0) & (z < 1)).sum() >= 20, "both clips and the interior"
    else:
        Y = (o.forward(spec, theta, X, np.float64).T + 0.3 * np.random.default_rng(3 + seed).standard_normal((X.shape[0], dims[-1]))).astype(np.float32)
    return spec, X, Y, theta.astype(np.float32), eta


LAST = []
for i_, fam_ in enumerate(FAM):
    small, many = DIMS[fam_]
    for j_, last_ in enumerate((R, T, S, X_, E)):
        LAST.append((fam_, small, 1003 if j_ % 2 else 517, T if j_ != 2 else E, last_, GAUSS))
    if many is not None:
        for j_, last_ in enumerate(((S, X_), (T, E), (E, R), (R, S), (X_, T), (T, X_))[i_]):
            LAST.append((fam_, many, 611 + 90 * j_, T, last_, GAUSS))
    LAST.append((fam_, small, 2000, T, N, BERN))
# one row count spanning many row tiles
LAST.append(("fast3", DIMS["fast3"][0], 6007, T, E, GAUSS))
LAST.append(("mid", DIMS["mid"][0], 5001, T, N, BERN))


def _lid(c):
    return f"{c[0]}-{'x'.join(map(str, c[1]))}-n{c[2]}-{AN[c[3]]}-{AN[c[4]]}-{'bern' if c[5] == BERN else 'gauss'}"


@pytest.mark.parametrize("c", LAST, ids=_lid)
def test_last_activation(native, monkeypatch, c):
    fam, dims, n, hidden, last, lik = c
    spec, X, Y, theta, eta = last_problem(dims, n, hidden, last, lik)
    check(native, monkeypatch, fam, spec, X, Y, theta, eta)


# ------------------------------------------------------------------------------------------------ (b) exp as a hidden activation
EXPH = []
for fam_, dims_ in (("fast3", [5, 20, 24, 1]), ("fast", [4, 17, 9, 3]), ("mid", [12, 40, 33, 48, 5]), ("tall", [100, 50, 50, 1]),
                    ("wide", [10, 200, 120, 1])):
    EXPH.append((fam_, dims_, [X_] * (len(dims_) - 2)))
    EXPH.append((fam_, dims_, ([X_, T, R] if len(dims_) > 4 else [T, X_])))


@pytest.mark.parametrize("c", EXPH, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-{'+'.join(AN[a] for a in c[2])}")
def test_exp_hidden(native, monkeypatch, c):
    fam, dims, acts = c
    spec, X, Y, theta, eta = scaled_problem(dims, 1501, acts, o.PRIOR_CAUCHY, GAUSS, seed=2)
    theta = (theta * 0.3).astype(np.float32)
    name = check(native, monkeypatch, fam, spec, X, Y, theta, eta)[0]
    assert "exp" in name.split(",")[0]


# ------------------------------------------------------------------------------------------------ (c) saturated Bernoulli
SAT = [("fast3", [5, 20, 24, 1]), ("fast3", [5, 20, 24, 2]), ("fast", [4, 17, 9, 3]),
       ("mid", [20, 64, 64, 1]), ("mid", [20, 64, 64, 2]), ("mid", [10, 91, 20, 3]),
       ("tall", [100, 50, 50, 1]), ("tall", [89, 34, 64, 2]), ("tall", [300, 20, 20, 10]),
       ("wide", [10, 200, 120, 1]), ("wide", [8, 90, 130, 70, 2]), ("wide", [31, 169, 160, 10]),
       ("layered", [5, 20, 24, 1]), ("layered", [5, 20, 24, 2]), ("layered", [5, 20, 24, 3])]
DROP = ((16.05, 17.0), (-18.6, -18.25))          # where fp32 and fp64 may decide the clip differently


def bands(z):
    return {"interior": np.abs(z) <= 8, "at_bound": (z >= 15.8) & (z <= 16.05), "above": z >= 17, "below": z <= -19}


def saturated_problem(dims, quota=40, pool=40000, seed=0, extra=200):
    """tanh hidden layers, the last layer scaled so that the fp64 pre-activations z spread over about [-30, 30]; rows drawn from a pool so that
    every output has `quota` rows in each band (more in the wide ones), none of a row's outputs in a DROP zone; labels independent of z"""
    spec = o.make_spec(dims, T, o.PRIOR_CAUCHY, BERN, S)
    rng = np.random.default_rng(50 + seed)
    Xp = (rng.standard_normal((pool, dims[0])) / np.sqrt(dims[0])).astype(np.float32)
    parts = [((rng.standard_normal((l.out_dim, l.in_dim)) * (2.0 / l.out_dim) ** 0.5).astype(np.float32),
              (rng.standard_normal((l.out_dim, 1)) * (2.0 / l.out_dim) ** 0.5).astype(np.float32)) for l in spec.layers]
    a = Xp.T.astype(np.float64)
    for W, b in parts[:-1]:
        a = np.tanh(W.astype(np.float64) @ a + b)
    W, b = parts[-1]
    z = W.astype(np.float64) @ a + b
    mu = z.mean(axis=1, keepdims=True)
    s = 30.0 / np.percentile(np.abs(z - mu), 99, axis=1, keepdims=True)   # per output: centred, 1 % of the rows beyond +-30
    parts[-1] = ((W * s).astype(np.float32), ((b - mu) * s).astype(np.float32))
    z = parts[-1][0].astype(np.float64) @ a + parts[-1][1]
    ok = np.ones(pool, bool)
    for lo, hi in DROP:
        ok &= ~np.any((z > lo) & (z < hi), axis=0)
    pick = set()
    for k in range(dims[-1]):
        for nm, m in bands(z[k]).items():
            idx = np.flatnonzero(m & ok)
            pick.update(rng.permutation(idx)[:quota * (1 if nm == "at_bound" else 3)].tolist())
    pick.update(rng.permutation(np.flatnonzero(ok))[:extra].tolist())
    idx = np.array(sorted(pick))
    idx = idx[:len(idx) - (0 if len(idx) % 16 else 1)]                 # a tail
    X = Xp[idx]
    Y = (rng.random((idx.size, dims[-1])) < 0.5).astype(np.float32)
    theta = o.flatten(parts).astype(np.float32)
    return spec, X, Y, theta, o.default_hypers(spec, 0.5), z[:, idx]


def check_bands(z, Y):
    for k in range(z.shape[0]):
        for nm, m in bands(z[k]).items():
            assert m.sum() >= (8 if nm == "at_bound" else 20), (k, nm, m.sum())
            assert 0 < Y[m, k].sum() < m.sum(), (k, nm, "both labels")


@pytest.mark.parametrize("c", SAT, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}")
def test_saturated_bernoulli(native, monkeypatch, c):
    fam, dims = c
    spec, X, Y, theta, eta, z = saturated_problem(dims)
    check_bands(z, Y)
    name, lp, g, f = check(native, monkeypatch, fam, spec, X, Y, theta, eta, ens=False)
    # precondition of the at-bound band: the kernel's fp32 sigmoid lands exactly on the clip bound there
    at = (z >= 15.8) & (z <= 16.05)
    assert np.all(f[at] == B_HI), f"{name}: forward on the at-bound rows {np.unique(f[at])}"
    assert np.all(f[z >= 17] > B_HI) and np.all(f[z <= -19] < B_LO)


def test_saturated_transition_on_the_trajectory_kernel(native, monkeypatch):
    spec, X, Y, theta, eta, z = saturated_problem([2, 12, 1], quota=10, pool=20000, seed=1, extra=60)
    assert X.shape[0] <= 380 and ((z >= 15.8) & (z <= 16.05)).sum() >= 8 and (z >= 17).sum() >= 8 and (z <= -19).sum() >= 8
    monkeypatch.setenv("TBNN_TRAJ", "1")
    env(monkeypatch, "fast3")
    rng = np.random.default_rng(11)
    p0 = rng.standard_normal(spec.n_params).astype(np.float32)
    eps, L = 2e-5, 4
    ch = native.Chain(layers_of(spec), likelihood=BERN, seed=50, chain_id=3, jit=True)
    try:
        assert ch.kernel_name.startswith("jit-fast3<tanh,sigmoid,bernoulli;"), ch.kernel_name
        ch.set_data(X, Y)
        lp64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[0]
        for log_u in (-1e30, 1e30):
            outs = []
            for _ in range(3):
                ch.set_state(theta); ch.set_hypers(eta)
                out = ch.hmc_step(eps, L, p0=p0, log_u=log_u)
                assert ch.last_transition_path == "trajectory"
                outs.append((out["log_accept_ratio"], out["logp_new"], ch.get_state()))
            assert all(x[0] == outs[0][0] and x[1] == outs[0][1] and np.array_equal(x[2], outs[0][2]) for x in outs)
            ref = o.weight_step(spec, theta, eta, X, Y, eps, L, p0, log_u, np.float64)
            tol = 2e-2 + 1e-4 * abs(ref.log_accept_ratio) + 4e-7 * abs(lp64)
            assert abs(out["log_accept_ratio"] - ref.log_accept_ratio) <= tol, (out["log_accept_ratio"], ref.log_accept_ratio, tol)
            assert bool(out["accepted"]) == ref.accepted
            assert np.abs(ch.get_state() - ref.theta).max() <= 1e-5 * max(1.0, np.abs(ref.theta).max())
            # p_L = p_0 + eps * (the L gradients): an at-bound label-0 row whose gradient is dropped moves the last bias's by eps * L
            g_inf = np.abs(o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[1]).max()
            assert np.abs(ch.debug_momentum() - ref.p_final).max() <= 4 * eps * L * 1e-4 * g_inf + 1e-6 * np.abs(ref.p_final).max()
    finally:
        ch.close()


# ------------------------------------------------------------------------------------------------ (d) the activations' special cases
SPECIAL = {
    # pre-activations z the rows put on every hidden unit: tanh around the series / exp switch at |z| = 0.3 and past exp(2z)'s overflow;
    # sigmoid past exp(-z)'s overflow; elu far below 0; relu exactly 0 (zero rows, zero bias: TF's ReluGrad convention a > 0)
    T: np.concatenate([np.linspace(0.28, 0.32, 161), -np.linspace(0.28, 0.32, 161), np.linspace(-1, 1, 41), [44.0, 45.0, 46.0, 60.0, 89.0, 100.0],
                       [-44.0, -45.0, -46.0, -60.0, -100.0], np.linspace(2.0, 12.0, 21)]),
    S: np.concatenate([[-120.0, -104.0, -100.0, -90.0, -89.0, -88.0, -87.0, 87.0, 88.0, 89.0, 90.0, 100.0, 120.0], np.linspace(-20, 20, 81)]),
    E: np.concatenate([[-200.0, -120.0, -104.0, -90.0, -88.0, -50.0, -20.0], -np.geomspace(1e-6, 10.0, 40), np.linspace(0, 3, 13)]),
    R: np.concatenate([np.zeros(64), np.linspace(-2, 2, 41)]),
}
SPECIAL_FAM = {"fast3": [1, 32, 2], "mid": [1, 32, 32, 2]}


def special_problem(act, dims):
    """x = z on one input; layer 0: W = 1, b = 0 (every unit's pre-activation IS x, exactly); on the mid family a second hidden layer with no
    activation and W = I passes a_1 on exactly; the last layer reads units 3 and 20 out (one-hot W, zero bias): the forward is the activation"""
    acts = [act] + [N] * (len(dims) - 3)
    spec = o.make_spec(dims, act, o.PRIOR_GAUSSIAN, GAUSS, N)
    for l, a in zip(spec.layers[:-1], acts):
        l.act = a
    U = dims[1]
    parts = [(np.ones((U, 1), np.float32), np.zeros((U, 1), np.float32))]
    for _ in range(len(dims) - 3):
        parts.append((np.eye(U, dtype=np.float32), np.zeros((U, 1), np.float32)))
    W = np.zeros((2, U), np.float32)
    W[0, 3] = W[1, 20] = 1.0
    parts.append((W, np.zeros((2, 1), np.float32)))
    theta = o.flatten(parts).astype(np.float32)
    X = SPECIAL[act].astype(np.float32).reshape(-1, 1)
    Y = np.random.default_rng(5).standard_normal((X.shape[0], 2)).astype(np.float32)
    return spec, X, Y, theta, o.default_hypers(spec, 0.5)


@pytest.mark.parametrize("fam", list(SPECIAL_FAM))
@pytest.mark.parametrize("act", [T, S, E, R], ids=lambda a: AN[a])
def test_activation_special_cases(native, monkeypatch, fam, act):
    spec, X, Y, theta, eta = special_problem(act, SPECIAL_FAM[fam])
    name, lp, g, f = check(native, monkeypatch, fam, spec, X, Y, theta, eta)
    f64 = o.forward(spec, theta, X, np.float64)
    err = float(np.max(np.abs(f - f64) / np.maximum(1.0, np.abs(f64))))
    bound = 4e-7                      # a few fp32 ulps of the outputs' scale (the fast tanh: absolute ~1e-7 over the whole line)
    LOG.append(f"{name}: max forward error {err:.2e} (bound {bound:.0e})")
    print(LOG[-1])
    assert err <= bound, LOG[-1]
    if act == R:
        zero = X[:, 0] == 0
        assert np.all(f[:, zero] == 0)
        # the gradient convention at z = 0 exactly is a > 0 (TF's ReluGrad): the zero rows add nothing to layer 0's bias gradient
        g0 = run(native, monkeypatch, fam, spec, X[zero], Y[zero], theta, eta, ens=False)[2]
        gp = o.target_log_prob_and_grad(spec, theta, eta, X[zero], Y[zero], np.float64)[1]
        ob = spec.offsets()[0][1]
        bias0 = slice(ob, ob + spec.layers[0].out_dim)
        assert np.abs(g0[bias0] - gp[bias0]).max() <= 1e-6 * max(1.0, np.abs(gp[bias0]).max()), (g0[bias0], gp[bias0])


# ------------------------------------------------------------------------------------------------ (e) the classification example at full size
def test_mn_burned_full_size(native, monkeypatch):
    import json
    from tensorbnn_amd.workloads import WORKLOADS, burned_state, synth_problem
    gold = os.path.join(os.path.dirname(__file__), "golden")
    wl = WORKLOADS["mn"]
    layers, lik, X, Y, _t, _e = synth_problem(wl["dims"], wl["n"], prior=wl["prior"], likelihood=wl["lik"], x_scale=wl.get("x_scale"))
    b = burned_state("mn", gold)
    theta, eta = b["theta"], b["eta"]
    spec = o.make_spec(wl["dims"], layers[0][2], layers[0][3], lik, layers[-1][2])
    assert layers_of(spec) == [tuple(l) for l in layers]
    want = json.load(open(os.path.join(gold, "mn_burned.json")))["kernel"]
    monkeypatch.delenv("TBNN_JIT_SKIP", raising=False)
    ch = native.Chain(layers, likelihood=lik, jit=True)
    try:
        assert ch.kernel_name == want, ch.kernel_name
        ch.set_data(X, Y)
        lp, g, _ = ch.logp_grad(theta, eta)
        for _ in range(2):
            lp2, g2, _ = ch.logp_grad(theta, eta)
            assert lp2 == lp and np.array_equal(g2, g)
        f = ch.forward(X, theta)
    finally:
        ch.close()
    clipped = int((f > B_HI).sum() + (f < B_LO).sum())
    assert clipped > 0, "the burned-in state keeps outputs outside the clip interval"
    f64 = o.forward(spec, theta, X, np.float64)
    assert np.abs(f - f64).max() <= 1e-4
    lp32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)[0]
    assert abs(lp - lp32) <= 4e-6 * abs(lp32), (lp, lp32)
    g64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)[1]
    e_g = tensor_err(spec, g, g64, 1e-3)
    print(f"mn_burned: {clipped} clipped outputs, gradient {e_g:.2e} of the tensor's inf-norm from fp64, logp {abs(lp - lp32) / abs(lp32):.2e} from fp32")
    assert e_g <= 1e-4, e_g
