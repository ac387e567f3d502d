"""Pins the CPU oracle (oracle/) -- runs without a GPU.

The reference supplies no golden vectors and cannot be imported (no TensorFlow),
so the oracle is pinned by: scipy closed forms for the density helpers (with the
reference's quirks Q1/Q2 asserted as deltas), torch.autograd (fp64) for every
hand-coded gradient (the extensions beyond the reference -- the categorical and
Poisson likelihoods, row weights -- have nothing else), HMC invariants, the committed fixtures (tests/golden) and
agreement between the NumPy and the C restatement.
"""
import math
import os

import numpy as np
import pytest
import scipy.stats as st

import tbnn_oracle as o

GOLD = os.path.join(os.path.dirname(__file__), "golden")


# ---------------------------------------------------------------- density KATs
def test_cauchy_log_prob_vs_scipy_with_sign_quirk():
    """BNN_functions.py:51-55 returns +log(1+z^2) - log(pi*gamma); scipy's cauchy.logpdf is
    -log(1+z^2) - log(pi*gamma).  Their sum is -2 log(pi*gamma) (Q1)."""
    x = np.linspace(-3, 3, 13)
    gamma, x0 = 0.5, 0.1
    ref = o.cauchy_log_prob(gamma, x0, x, np.float64)
    sp = st.cauchy.logpdf(x, loc=x0, scale=gamma)
    np.testing.assert_allclose(ref + sp, -2 * np.log(np.pi * gamma), rtol=1e-12)
    z = (x - x0) / gamma
    np.testing.assert_allclose(ref, np.log1p(z * z) - np.log(np.pi * gamma), rtol=1e-12)
    g = np.load(os.path.join(GOLD, "density_kat.npz"))
    np.testing.assert_allclose(ref, g["cauchy"], rtol=1e-12)


def test_multivariate_log_prob_vs_scipy_and_normaliser_quirk():
    x = np.linspace(-3, 3, 13)
    full = o.multivariate_log_prob(np.full(13, 0.7), 0.2, x, np.float64)
    np.testing.assert_allclose(full, st.norm.logpdf(x, 0.2, 0.7).sum(), rtol=1e-12)
    # Q2: scalar sigma => normaliser counted once (k = size(sigma) = 1)
    scal = o.multivariate_log_prob(0.7, 0.2, x, np.float64)
    one_norm = -0.5 * (2 * np.log(0.7) + np.log(2 * np.pi))
    np.testing.assert_allclose(scal, st.norm.logpdf(x, 0.2, 0.7).sum() - 12 * one_norm, rtol=1e-12)
    g = np.load(os.path.join(GOLD, "density_kat.npz"))
    np.testing.assert_allclose(full, g["mvn_vec"], rtol=1e-12)
    np.testing.assert_allclose(scal, g["mvn_scalar_sigma"], rtol=1e-12)


def test_sigma_clamp():
    assert np.isfinite(o.multivariate_log_prob(0.0, 0.0, np.array([1.0]), np.float32))
    a = o.multivariate_log_prob(1e-12, 0.0, np.array([1e-9]), np.float64)
    b = o.multivariate_log_prob(1e-8, 0.0, np.array([1e-9]), np.float64)
    assert a == b


def test_mvn_diag_scalar_vs_scipy():
    assert abs(o.mvn_diag_scalar_log_prob(0.3, 0.0, 0.2, np.float64) - st.norm.logpdf(0.3, 0, 0.2)) < 1e-12


# ---------------------------------------------------------------- gradients vs torch.autograd (fp64)
def _torch_target(spec, theta, eta, X, Y, w=None):
    """w: row weights of the likelihood term (None: every row counts once)"""
    import torch
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    et = torch.tensor(np.asarray(eta, dtype=np.float64), requires_grad=True)
    Xt, Yt = torch.tensor(X, dtype=torch.float64), torch.tensor(Y, dtype=torch.float64)
    wt = torch.ones(len(X), dtype=torch.float64) if w is None else torch.tensor(np.asarray(w, dtype=np.float64))

    def N(loc, sc):
        return torch.distributions.Normal(torch.tensor(loc, dtype=torch.float64), torch.tensor(sc, dtype=torch.float64))

    def prior(l, h4, W, b, hyper):
        tot = 0
        for x, loc, g in ((W, h4[0], h4[1]), (b, h4[2], h4[3])):
            sc = g ** 2
            if l.prior == o.PRIOR_CAUCHY:
                tot = tot + (torch.log(1 + ((x - loc) / sc) ** 2) - torch.log(math.pi * sc)).sum()
                if hyper:
                    tot = tot + N(0.0, 0.2).log_prob(loc) + \
                        N(0.5 ** 0.5, 0.5).log_prob(sc)
            else:
                s = torch.clamp(sc, 1e-8, 1e8)
                tot = tot - 0.5 * (2 * torch.log(s) + (((x - loc) / s) ** 2).sum() + math.log(2 * math.pi))
                if hyper:
                    tot = tot + N(0.0, 0.1).log_prob(loc) + \
                        N(1.0, 0.1).log_prob(sc)
        return tot

    def lik(f):
        if spec.likelihood == o.LIK_BERNOULLI:
            p = torch.clamp(f, 1e-8, 1 - 1e-7)
            y = Yt.reshape(-1, f.shape[0]).T
            return (wt * (torch.xlogy(y, p) + torch.xlogy(1 - y, 1 - p))).sum()
        y = Yt.reshape(f.shape[1], -1).T
        if spec.likelihood == o.LIK_CATEGORICAL:
            return (wt * y * torch.log_softmax(f, dim=0)).sum()
        if spec.likelihood == o.LIK_POISSON:
            return (wt * (y * f - torch.exp(f) - torch.lgamma(y + 1))).sum()
        if spec.likelihood == o.LIK_STUDENT_T:
            nu, s = (torch.tensor(v, dtype=torch.float64) for v in (spec.lik_df, spec.fixed_sd))
            return (wt * torch.distributions.StudentT(nu, f, s).log_prob(y)).sum()
        if spec.likelihood == o.LIK_NEG_BINOMIAL:
            r = torch.tensor(spec.lik_df, dtype=torch.float64)
            lden = torch.logaddexp(f, torch.log(r))
            return (wt * (torch.lgamma(y + r) - torch.lgamma(r) - torch.lgamma(y + 1) + y * (f - lden) + r * (torch.log(r) - lden))).sum()
        if spec.likelihood == o.LIK_GAMMA:              # shape a, mean exp(f): rate a exp(-f)
            a = torch.tensor(spec.lik_df, dtype=torch.float64)
            return (wt * torch.distributions.Gamma(a, a * torch.exp(-f)).log_prob(y)).sum()
        if spec.likelihood == o.LIK_HETERO_GAUSSIAN:
            gc = torch.clamp(f[1], -math.log(1e8), math.log(1e8))
            return (wt * (-0.5 * math.log(2 * math.pi) - gc - 0.5 * (y[0] - f[0]) ** 2 * torch.exp(-2 * gc))).sum()
        assert spec.likelihood in (o.LIK_GAUSSIAN, o.LIK_FIXED_GAUSSIAN)
        s = torch.clamp(et[-1] ** 2, 1e-8, 1e8) if spec.likelihood == o.LIK_GAUSSIAN else torch.tensor(spec.fixed_sd, dtype=torch.float64)
        n_el = wt.sum() * f.shape[0]                     # (unweighted: f.numel(), exactly)
        return -0.5 * (2 * n_el * torch.log(s) + (wt * ((y - f) / s) ** 2).sum() + n_el * math.log(2 * math.pi))

    def run(hyper):
        a = Xt.T
        tot = 0
        off = 0
        for i, l in enumerate(spec.layers):
            W = th[off:off + l.in_dim * l.out_dim].reshape(l.out_dim, l.in_dim)
            off += l.in_dim * l.out_dim
            b = th[off:off + l.out_dim].reshape(l.out_dim, 1)
            off += l.out_dim
            tot = tot + prior(l, et[4 * i:4 * i + 4], W, b, hyper)
            z = W @ a + b
            a = {o.ACT_NONE: lambda v: v, o.ACT_RELU: torch.relu, o.ACT_TANH: torch.tanh, o.ACT_SIGMOID: torch.sigmoid, o.ACT_EXP: torch.exp, o.ACT_ELU: torch.nn.functional.elu}[l.act](z)
        if not hyper or spec.likelihood == o.LIK_GAUSSIAN:
            tot = tot + lik(a)
        return tot

    lp = run(False)
    g_th, = torch.autograd.grad(lp, th)
    hl = run(True)
    g_et, = torch.autograd.grad(hl, et, allow_unused=True)
    return float(lp.detach()), g_th.numpy(), float(hl.detach()), g_et.numpy()


CASES = {
    "c1": ([1, 10, 10, 1], 64, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN),
    "trainreg": ([1, 10, 10, 10, 1], 11, o.ACT_TANH, o.PRIOR_GAUSSIAN, o.LIK_FIXED_GAUSSIAN),
    "c2": ([5, 50, 50, 50, 1], 96, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN),
    "c5": ([20, 100, 100, 2], 64, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_BERNOULLI),
    "sig": ([4, 7, 3], 50, o.ACT_SIGMOID, o.PRIOR_GAUSSIAN, o.LIK_GAUSSIAN),
    "elu": ([3, 20, 17, 2], 40, o.ACT_ELU, o.PRIOR_GAUSSIAN, o.LIK_GAUSSIAN),
    "exp": ([2, 6, 1], 30, o.ACT_EXP, o.PRIOR_CAUCHY, o.LIK_FIXED_GAUSSIAN),
}


@pytest.mark.parametrize("case", list(CASES))
def test_hand_coded_gradients_match_autograd(case):
    dims, n, act, prior, lik = CASES[case]
    spec, X, Y, theta, eta = o.synth_problem(dims, n, act, prior, lik)
    rng = np.random.default_rng(1)
    eta = (eta + 0.05 * rng.standard_normal(eta.size)).astype(np.float32)
    lp_t, g_t, hl_t, hg_t = _torch_target(spec, theta, eta, X, Y)
    lp, g = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)
    assert abs(lp - lp_t) <= 1e-10 * abs(lp_t)
    np.testing.assert_allclose(g, g_t, rtol=1e-9, atol=1e-9 * np.abs(g_t).max())
    hl, hg = o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64)
    assert abs(hl - hl_t) <= 1e-10 * abs(hl_t)
    np.testing.assert_allclose(hg, hg_t, rtol=1e-8, atol=1e-9 * np.abs(hg_t).max())
    # closed-form data term (sufficient statistic S) == full evaluation
    if spec.likelihood == o.LIK_GAUSSIAN:
        f = o.forward(spec, theta, X, np.float64)
        S = np.sum((Y.reshape(n, -1).T - f) ** 2)
        hl2, hg2 = o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64, S=S)
        assert abs(hl2 - hl) <= 1e-9 * abs(hl)
        np.testing.assert_allclose(hg2, hg, rtol=1e-9, atol=1e-9 * np.abs(hg).max())


# the last layer's activation: every one network.add takes after the final dense layer (Gaussian), and a Bernoulli likelihood on raw outputs,
# clipped on both sides of [1e-8, 1 - 1e-7]
LAST_CASES = {
    "gauss_relu": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, o.ACT_RELU),
    "gauss_tanh": ([3, 12, 9, 2], 60, o.ACT_ELU, o.PRIOR_GAUSSIAN, o.LIK_GAUSSIAN, o.ACT_TANH),
    "gauss_sigmoid": ([4, 10, 3], 50, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, o.ACT_SIGMOID),
    "gauss_exp": ([2, 8, 8, 1], 40, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, o.ACT_EXP),
    "gauss_elu": ([5, 16, 7, 3], 70, o.ACT_SIGMOID, o.PRIOR_GAUSSIAN, o.LIK_GAUSSIAN, o.ACT_ELU),
    "bern_none": ([4, 12, 12, 3], 80, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_BERNOULLI, o.ACT_NONE),
}


@pytest.mark.parametrize("case", list(LAST_CASES))
def test_hand_coded_gradients_match_autograd_last_activation(case):
    dims, n, act, prior, lik, last = LAST_CASES[case]
    spec, X, Y, theta, eta = o.synth_problem(dims, n, act, prior, lik)
    spec.layers[-1].act = last
    if last == o.ACT_NONE:
        f = o.forward(spec, theta, X, np.float64)
        assert (f > 1 - 1e-7).sum() > 10 and (f < 1e-8).sum() > 10 and ((f > 1e-8) & (f < 1 - 1e-7)).sum() > 10     # both clips + interior
    rng = np.random.default_rng(1)
    eta = (eta + 0.05 * rng.standard_normal(eta.size)).astype(np.float32)
    lp_t, g_t, hl_t, hg_t = _torch_target(spec, theta, eta, X, Y)
    lp, g = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)
    assert abs(lp - lp_t) <= 1e-10 * abs(lp_t)
    np.testing.assert_allclose(g, g_t, rtol=1e-9, atol=1e-9 * np.abs(g_t).max())
    hl, hg = o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64)
    assert abs(hl - hl_t) <= 1e-10 * abs(hl_t)
    np.testing.assert_allclose(hg, hg_t, rtol=1e-8, atol=1e-9 * np.abs(hg_t).max())


# the extensions beyond the reference (the categorical, Poisson, Student-t, negative-binomial, heteroscedastic Gaussian and Gamma
# likelihoods, per-row likelihood weights): autograd is all that pins them
EXT_CASES = {
    # dims, rows, hidden activation, prior, likelihood, targets (Student-t: nu, at the scale STUDENT_S; negative binomial: r; Gamma: the
    # shape a; heteroscedastic: None, or the last bias of output 1 that puts every row's log-sd beyond the clip), weighted
    "cat_onehot": ([4, 12, 12, 3], 80, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_CATEGORICAL, "onehot", False),
    "cat_soft": ([4, 12, 12, 3], 80, o.ACT_ELU, o.PRIOR_GAUSSIAN, o.LIK_CATEGORICAL, "soft", False),
    "cat_large_logits": ([4, 12, 12, 3], 80, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_CATEGORICAL, "large", False),
    "pois": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_POISSON, "counts", False),
    "pois_gaussian_prior": ([3, 12, 9, 2], 60, o.ACT_ELU, o.PRIOR_GAUSSIAN, o.LIK_POISSON, "counts", False),
    "weighted_gauss": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAUSSIAN, None, True),
    "weighted_fixed_gauss": ([3, 12, 9, 2], 60, o.ACT_RELU, o.PRIOR_GAUSSIAN, o.LIK_FIXED_GAUSSIAN, None, True),
    "weighted_bern": ([4, 12, 12, 3], 80, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_BERNOULLI, None, True),
    "weighted_cat": ([4, 12, 12, 3], 80, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_CATEGORICAL, "soft", True),
    "weighted_pois": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_POISSON, "counts", True),
    "student_nu1": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_STUDENT_T, 1.0, False),
    "student_nu2.5": ([4, 12, 12, 2], 80, o.ACT_ELU, o.PRIOR_GAUSSIAN, o.LIK_STUDENT_T, 2.5, False),
    "student_nu1e4": ([3, 12, 9, 2], 60, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_STUDENT_T, 1e4, False),
    "negbin_r0.5": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_GAUSSIAN, o.LIK_NEG_BINOMIAL, 0.5, False),
    "negbin_r30": ([4, 12, 12, 2], 80, o.ACT_SIGMOID, o.PRIOR_CAUCHY, o.LIK_NEG_BINOMIAL, 30.0, False),
    "negbin_r1e4": ([3, 12, 9, 2], 60, o.ACT_ELU, o.PRIOR_CAUCHY, o.LIK_NEG_BINOMIAL, 1e4, False),
    "hetero": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_HETERO_GAUSSIAN, None, False),
    "hetero_gaussian_prior": ([4, 12, 12, 2], 80, o.ACT_RELU, o.PRIOR_GAUSSIAN, o.LIK_HETERO_GAUSSIAN, None, False),
    "hetero_clip_above": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_HETERO_GAUSSIAN, 25.0, False),
    "hetero_clip_below": ([3, 12, 9, 2], 60, o.ACT_ELU, o.PRIOR_GAUSSIAN, o.LIK_HETERO_GAUSSIAN, -25.0, False),
    "weighted_student": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_STUDENT_T, 2.5, True),
    "weighted_negbin": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_NEG_BINOMIAL, 30.0, True),
    "weighted_hetero": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_HETERO_GAUSSIAN, None, True),
    "gamma_a0.5_one_output": ([3, 12, 9, 1], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAMMA, 0.5, False),
    "gamma_a10": ([4, 12, 12, 3], 80, o.ACT_ELU, o.PRIOR_GAUSSIAN, o.LIK_GAMMA, 10.0, False),
    "gamma_a200": ([3, 12, 9, 2], 60, o.ACT_RELU, o.PRIOR_CAUCHY, o.LIK_GAMMA, 200.0, False),
    "weighted_gamma": ([3, 12, 9, 2], 60, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_GAMMA, 2.0, True),
    "weighted_gamma_a0.5_one_output": ([3, 12, 9, 1], 60, o.ACT_ELU, o.PRIOR_GAUSSIAN, o.LIK_GAMMA, 0.5, True),
}
STUDENT_S = 0.25                         # (exact in fp32: the oracle takes the scale as the library receives it)
COUNTS = (o.LIK_POISSON, o.LIK_NEG_BINOMIAL)


def _ext_problem(case):
    dims, n, act, prior, lik, targets, weighted = EXT_CASES[case]
    if lik not in (o.LIK_GAUSSIAN, o.LIK_FIXED_GAUSSIAN, o.LIK_BERNOULLI):
        _g, X, Yr, theta, eta = o.synth_problem(dims, n, act, prior, o.LIK_GAUSSIAN)        # standardised teacher outputs [n, K]
        spec = o.make_spec(dims, act, prior, lik, o.ACT_NONE, fixed_sd=STUDENT_S,
                           lik_df=targets if lik in (o.LIK_STUDENT_T, o.LIK_NEG_BINOMIAL, o.LIK_GAMMA) else 0.0)
        eta = eta[:spec.n_hypers]                                                           # no likelihood hyper
    else:
        spec, X, Y, theta, eta = o.synth_problem(dims, n, act, prior, lik)
    ow, ob = spec.offsets()[-1]
    theta = theta.astype(np.float64)
    if lik == o.LIK_CATEGORICAL:
        e = np.exp(2.0 * Yr - (2.0 * Yr).max(axis=1, keepdims=True))
        Y = e / e.sum(axis=1, keepdims=True) if targets == "soft" else np.eye(dims[-1])[np.argmax(Yr, axis=1)]
        if targets == "large":           # the last layer scaled until the logits pass +-70: exp(f) without the max shift overflows in fp32
            theta[ow:] *= 80.0 / np.abs(o.forward(spec, theta, X, np.float64)).max()
            assert np.abs(o.forward(spec, theta, X, np.float64)).max() > 70
    if lik in COUNTS:
        Y = np.random.default_rng(11).poisson(np.exp(np.clip(1.5 + 1.5 * Yr, -3.0, 6.0))).astype(np.float64)
        Y[::5] = 0.0                     # zero counts
        Y[1::5] += 0.5                   # counts need not be integers: lgamma(y + 1)
        f = o.forward(spec, theta, X, np.float64)
        if np.abs(f).max() > 5.0:        # the state's own log-rates within [-5, 5]
            theta[ow:] *= 5.0 / np.abs(f).max()
        assert np.abs(o.forward(spec, theta, X, np.float64)).max() <= 5.0 + 1e-9 and (Y == 0).any() and (Y % 1 != 0).any()
    if lik == o.LIK_GAMMA:               # positive targets of shape a around exp(0.5 + 0.8 z), every fifth row far off its mean on either side;
        f = o.forward(spec, theta, X, np.float64)                   # the state's own log-means within [-5, 5]
        if np.abs(f).max() > 5.0:
            theta[ow:] *= 5.0 / np.abs(f).max()
        Y = np.maximum(np.random.default_rng(11).gamma(targets, np.exp(0.5 + 0.8 * Yr) / targets), 1e-30)
        Y[::5] *= 50.0
        Y[1::5] /= 50.0
        assert np.abs(o.forward(spec, theta, X, np.float64)).max() <= 5.0 + 1e-9 and np.all(Y > 0)
    if lik == o.LIK_STUDENT_T:           # the teacher's outputs plus N(0, s^2), every tenth row moved by 30 s: both ends of r^2 / (nu s^2)
        Y = Yr + STUDENT_S * np.random.default_rng(11).standard_normal(Yr.shape)
        Y[::10] += 30.0 * STUDENT_S
    if lik == o.LIK_HETERO_GAUSSIAN:     # one target per row; the state's own outputs within [-5, 5], so that exp(-2 g) stays moderate
        Y = Yr[:, 0] + 0.3 * np.random.default_rng(11).standard_normal(n)
        theta[ow:] *= min(1.0, 5.0 / np.abs(o.forward(spec, theta, X, np.float64)).max())
        if targets is not None:          # the clip: every row's log-sd beyond +-log(1e8), dL/dg exactly 0
            theta[ob + 1] = targets
            if targets > 0:              # above the clip u = exp(-2 G) = 1e-16: residuals of 1e16 keep dL/df = r u at O(1), where an error in it shows
                Y = Y + 1e16 * (-1.0) ** np.arange(n)
            f = o.forward(spec, theta, X, np.float64)
            assert np.all(np.abs(f[1]) > o.LOG_CLIP) and np.all(o.likelihood_grad(spec, eta, f, Y, np.float64)[1] == 0)
    return spec, X, np.asarray(Y, np.float64), theta, eta, (_real_weights(n) if weighted else None)


def _real_weights(n, seed=3):
    """the recipe of tests/test_gpu_row_weights.py: gamma-distributed, every seventh weight 0"""
    w = np.random.default_rng(seed).gamma(0.7, 1.5, n).astype(np.float32)
    w[::7] = 0.0
    return w


@pytest.mark.parametrize("case", list(EXT_CASES))
def test_extension_gradients_match_autograd(case):
    spec, X, Y, theta, eta, w = _ext_problem(case)
    eta = (eta + 0.05 * np.random.default_rng(1).standard_normal(eta.size)).astype(np.float32)
    lp_t, g_t, hl_t, hg_t = _torch_target(spec, theta, eta, X, Y, w)
    lp, g = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64, w=w)
    assert abs(lp - lp_t) <= 1e-10 * abs(lp_t)
    assert lp == o.target_log_prob(spec, theta, eta, X, Y, np.float64, w=w)
    np.testing.assert_allclose(g, g_t, rtol=1e-9, atol=1e-9 * np.abs(g_t).max())
    hl, hg = o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64, w=w)
    assert abs(hl - hl_t) <= 1e-10 * abs(hl_t) and hl == o.hyper_log_prob(spec, eta, theta, X, Y, np.float64, w=w)
    np.testing.assert_allclose(hg, hg_t, rtol=1e-8, atol=1e-9 * np.abs(hg_t).max())
    if spec.likelihood == o.LIK_GAUSSIAN:        # the weighted closed form: S = sum_i w_i sum_k (y - f)^2, n = sum(w) d_out
        f = o.forward(spec, theta, X, np.float64)
        S = np.sum(w.astype(np.float64) * (Y.T - f) ** 2)
        hl2, hg2 = o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64, S=S, w=w)
        assert abs(hl2 - hl_t) <= 1e-10 * abs(hl_t)
        np.testing.assert_allclose(hg2, hg_t, rtol=1e-8, atol=1e-9 * np.abs(hg_t).max())


@pytest.mark.parametrize("case", ["weighted_gauss", "weighted_fixed_gauss", "weighted_bern", "weighted_cat", "weighted_pois",
                                  "weighted_student", "weighted_negbin", "weighted_hetero", "weighted_gamma",
                                  "weighted_gamma_a0.5_one_output"])
def test_integer_weights_are_repeated_rows(case):
    spec, X, Y, theta, eta, _w = _ext_problem(case)
    w = np.random.default_rng(11).integers(0, 4, len(X))
    assert (w == 0).any() and (w == 3).any()
    Xr, Yr = np.repeat(X, w, axis=0), np.repeat(Y, w, axis=0)
    lp, g = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64, w=w)
    lp_r, g_r = o.target_log_prob_and_grad(spec, theta, eta, Xr, Yr, np.float64)
    assert abs(lp - lp_r) <= 1e-12 * abs(lp_r)
    np.testing.assert_allclose(g, g_r, rtol=0, atol=1e-12 * np.abs(g_r).max())
    hl, hg = o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64, w=w)
    hl_r, hg_r = o.hyper_log_prob_and_grad(spec, eta, theta, Xr, Yr, np.float64)
    assert abs(hl - hl_r) <= 1e-12 * abs(hl_r)
    np.testing.assert_allclose(hg, hg_r, rtol=0, atol=1e-12 * np.abs(hg_r).max())


@pytest.mark.parametrize("case", ["weighted_cat", "weighted_pois", "weighted_student", "weighted_negbin", "weighted_hetero",
                                  "weighted_gamma", "weighted_gamma_a0.5_one_output"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_unit_weights_are_exactly_unweighted(case, dtype):
    spec, X, Y, theta, eta, _w = _ext_problem(case)
    lp, g = o.target_log_prob_and_grad(spec, theta, eta, X, Y, dtype)
    lp1, g1 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, dtype, w=np.ones(len(X), np.float32))
    assert lp1 == lp and np.array_equal(g1, g)


@pytest.mark.parametrize("code", [4, 6, -1, 7, 9, 11])
def test_unknown_likelihood_code_raises(code):
    """a code the oracle does not know is an error in every target, never another likelihood's chain"""
    spec, X, Y, theta, eta = o.synth_problem([3, 5, 2], 10, o.ACT_TANH, o.PRIOR_CAUCHY, o.LIK_FIXED_GAUSSIAN)
    spec.likelihood = code
    f = o.forward(spec, theta, X, np.float64)
    for call in (lambda: o.log_likelihood(spec, eta, f, Y, np.float64),
                 lambda: o.target_log_prob(spec, theta, eta, X, Y, np.float64),
                 lambda: o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64),
                 lambda: o.hyper_log_prob(spec, eta, theta, X, Y, np.float64),
                 lambda: o.hyper_log_prob_and_grad(spec, eta, theta, X, Y, np.float64),
                 lambda: o.weight_step(spec, theta, eta, X, Y, 1e-3, 2, np.zeros_like(theta), -1.0, np.float64)):
        with pytest.raises(ValueError):
            call()


def _tie_problem(last):
    """1 -> 4 -> 1 relu, Bernoulli, every product and sum exact in fp32: the last layer's pre-activation of row r IS x_r.  last = sigmoid:
    x over [15.5, 16.5), where the fp32 sigmoid returns exactly float32(1 - 1e-7) = 1 - 2^-23 (the clip's upper bound) on most rows; last = none:
    raw outputs x exactly on both bounds, inside and outside them"""
    if last == o.ACT_SIGMOID:
        x = np.float32(15.5) + np.arange(64, dtype=np.float32) / np.float32(64)
    else:
        b_lo, b_hi = np.float32(1e-8), np.float32(1 - 1e-7)
        x = np.array([b_lo] * 8 + [b_hi] * 8 + [0.25, 0.5, 0.75, 1.5, 2.0, -1.0, 1e-9, 0.0] * 2, np.float32)
    spec = o.make_spec([1, 4, 1], o.ACT_RELU, o.PRIOR_GAUSSIAN, o.LIK_BERNOULLI, last)
    W1, b1 = np.array([[1.0], [0.5], [-1.0], [2.0]], np.float32), np.zeros((4, 1), np.float32)
    W2, b2 = np.array([[0.5, 1.0, 0.25, 0.0]], np.float32), np.zeros((1, 1), np.float32)
    theta = o.flatten([(W1, b1), (W2, b2)]).astype(np.float32)
    Y = (np.arange(x.size) % 4 == 3).astype(np.float32).reshape(-1, 1)                              # mostly label 0
    return spec, x.reshape(-1, 1).astype(np.float32), Y, theta, o.default_hypers(spec, 0.5)


@pytest.mark.parametrize("last", [o.ACT_SIGMOID, o.ACT_NONE])
def test_fp32_clip_ties_match_autograd(last):
    """tf.clip_by_value (likelihood.py:226-231) is minimum / maximum, whose gradients pass on ties, as torch.clamp's do: an fp32 output exactly on
    a bound keeps its gradient (a label-0 row at 1 - 2^-23 behind a sigmoid: dL/dz = -p, about -1).  fp64 never meets the tie; this compares the
    fp32 arms of the oracle and of autograd on rows that sit on it."""
    import torch
    from torch_ref import TorchTarget
    spec, X, Y, theta, eta = _tie_problem(last)
    f32 = o.forward(spec, theta, X, np.float32)
    b_lo, b_hi = np.float32(1e-8), np.float32(1 - 1e-7)
    tt = TorchTarget(spec, X, Y, torch.float32)
    th = torch.tensor(theta)
    a = tt.Xt
    for i, l in enumerate(spec.layers):                      # the same forward in torch: the ties must be the same rows
        W, b = (torch.from_numpy(p) for p in o.unflatten(spec, theta)[i])
        a = W @ a + b
        a = torch.relu(a) if l.act == o.ACT_RELU else torch.sigmoid(a) if l.act == o.ACT_SIGMOID else a
    assert np.array_equal(a.numpy(), f32)
    on = (f32 == b_hi) | (f32 == b_lo)
    assert on.sum() >= (32 if last == o.ACT_SIGMOID else 16) and (f32 == b_hi).any() and ((f32 == b_hi) & (Y.T == 0)).sum() >= 4
    lp_t, g_t = tt.value_and_grad(theta, eta)
    lp, g = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)
    assert abs(lp - lp_t) <= 1e-6 * abs(lp_t)
    for a_, b_ in ((0, 4), (4, 8), (8, 12), (12, 13)):
        assert np.abs(g[a_:b_] - g_t[a_:b_]).max() <= 1e-5 * max(np.abs(g_t[a_:b_]).max(), 1e-3), (a_, g[a_:b_], g_t[a_:b_])
    # the last bias collects dL/dz of every row: each label-0 row on the upper bound adds -p (or -1/(1-p) on raw outputs)
    if last == o.ACT_SIGMOID:
        at = (f32 == b_hi) & (Y.T == 0)
        assert g[12] <= -0.99 * at.sum()


@pytest.mark.parametrize("case", ["c1", "c2"])
def test_float32_arm_within_stated_tolerance(case):
    """the reference's own arithmetic (fp32) sits inside the tolerance band the GPU tests use"""
    dims, n, act, prior, lik = CASES[case]
    spec, X, Y, theta, eta = o.synth_problem(dims, n, act, prior, lik)
    lp64, g64 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float64)
    lp32, g32 = o.target_log_prob_and_grad(spec, theta, eta, X, Y, np.float32)
    assert abs(lp32 - lp64) <= 4e-6 * abs(lp64)
    assert np.abs(g32 - g64).max() <= 1e-4 * np.abs(g64).max()


# ---------------------------------------------------------------- HMC invariants
def _std_normal_vg(q):
    return -0.5 * float(np.sum(q.astype(np.float64) ** 2)), (-q).astype(q.dtype)


def test_leapfrog_reversibility():
    rng = np.random.default_rng(3)
    q0, p0 = rng.standard_normal(20), rng.standard_normal(20)
    r = o.hmc_step(_std_normal_vg, q0, 0.1, 25, p0, -1e30, np.float64)
    back = o.hmc_step(_std_normal_vg, r.theta_proposed, 0.1, 25, -r.p_final, -1e30, np.float64)
    np.testing.assert_allclose(back.theta_proposed, q0, atol=1e-12)


def test_energy_error_is_second_order():
    rng = np.random.default_rng(4)
    q0, p0 = rng.standard_normal(10), rng.standard_normal(10)
    errs = []
    for eps, L in ((0.1, 10), (0.05, 20), (0.025, 40)):
        errs.append(abs(o.hmc_step(_std_normal_vg, q0, eps, L, p0, 0.0, np.float64).log_accept_ratio))
    assert errs[1] < errs[0] / 3 and errs[2] < errs[1] / 3


def test_small_eps_accepts_and_nonfinite_rejects():
    rng = np.random.default_rng(5)
    q0, p0 = rng.standard_normal(10), rng.standard_normal(10)
    r = o.hmc_step(_std_normal_vg, q0, 1e-4, 5, p0, np.log(0.999), np.float64)
    assert r.accepted and r.accept_prob > 0.999
    bad = lambda q: (float("nan"), np.zeros_like(q))
    r = o.hmc_step(bad, q0, 1e-2, 3, p0, -1e30, np.float64)
    assert not r.accepted and r.log_accept_ratio == -np.inf and r.sjd == 0.0


def test_acceptance_rate_standard_normal():
    """mean accept prob over many transitions on N(0,I) matches exp(min(0,dH)) statistics: > 0.9 at eps=0.2"""
    rng = np.random.default_rng(6)
    q = rng.standard_normal(16)
    acc = []
    for _ in range(300):
        r = o.hmc_step(_std_normal_vg, q, 0.2, 10, rng.standard_normal(16), np.log(rng.random()), np.float64)
        q = r.theta
        acc.append(r.accept_prob)
    assert 0.9 < np.mean(acc) <= 1.0


# ---------------------------------------------------------------- fixtures + C restatement
@pytest.mark.parametrize("name", ["c1", "trainreg", "c2", "c5"])
def test_oracle_reproduces_golden(name):
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    spec = o.make_spec(list(g["dims"]), int(g["act"]), int(g["prior"]), int(g["lik"]),
                       o.ACT_SIGMOID if int(g["lik"]) == o.LIK_BERNOULLI else o.ACT_NONE)
    lp, gr = o.target_log_prob_and_grad(spec, g["theta"], g["eta"], g["X"], g["Y"], np.float64)
    assert abs(lp - g["logp64"]) <= 1e-12 * abs(g["logp64"])
    np.testing.assert_allclose(gr, g["grad64"], rtol=1e-10, atol=1e-12)
    r = o.weight_step(spec, g["theta"], g["eta"], g["X"], g["Y"], float(g["eps"]), 5, g["p0"], np.log(0.5), np.float64)
    np.testing.assert_allclose(r.trace_logp, g["step_half_trace"], rtol=1e-12)
    assert abs(r.log_accept_ratio - g["step_half_lar"]) < 1e-8
    # fp32 arithmetic (the reference's) gives the same decision within the stated band
    assert abs(g["step_half_lar32"] - g["step_half_lar"]) <= 2e-2 + 1e-4 * abs(g["step_half_lar"])


@pytest.mark.parametrize("name", ["c1", "trainreg", "c2", "c5"])
def test_c_restatement_matches_numpy(name):
    import c_oracle
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    spec = o.make_spec(list(g["dims"]), int(g["act"]), int(g["prior"]), int(g["lik"]),
                       o.ACT_SIGMOID if int(g["lik"]) == o.LIK_BERNOULLI else o.ACT_NONE)
    co = c_oracle.COracle(spec, g["X"], g["Y"])
    lp, gr, _ = co.logp_grad(g["theta"], g["eta"])
    assert abs(lp - g["logp64"]) <= 4e-6 * abs(g["logp64"]) + 1e-3
    assert np.abs(gr - g["grad64"]).max() <= 1e-4 * np.abs(g["grad64"]).max()
    th, acc, lar, lo, ln = co.hmc_step(g["theta"], g["eta"], float(g["eps"]), 5, g["p0"], np.log(0.5))
    assert abs(lar - g["step_half_lar"]) <= 2e-2 + 1e-4 * abs(g["step_half_lar"])
    assert acc == bool(g["step_half_accepted"])


def test_philox_known_answer():
    """Philox4x32-10 known-answer vectors (Random123 kat_vectors): counter/key all zero, and all ones... """
    assert o.philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert o.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    z = o.philox_normals(4000, 50, 0, 1, 0)
    assert abs(z.mean()) < 0.06 and abs(z.std() - 1) < 0.05


def test_dual_averaging_golden():
    g = np.load(os.path.join(GOLD, "c1.npz"))
    stt = o.DualAveragingState(hyper_step_size=0.01, burnin=100)
    for ep, lar in enumerate(g["da_lars"]):
        acc = o.dual_averaging_update(stt, ep, lar)
        np.testing.assert_allclose([acc, stt.h, stt.log_eps_bar, stt.eps_h], g["da_trace"][ep], rtol=1e-6)


def test_sample_files_roundtrip(tmp_path):
    """writer (network.py:545-663) -> reader (predictor.py:43-113)"""
    spec, X, Y, theta, eta = o.synth_problem([1, 10, 10, 1], 8)
    parts = o.unflatten(spec, theta)
    shapes = [s.shape for pr in parts for s in pr]
    w = o.SampleWriter(str(tmp_path / "run"), shapes, ["dense", "relu", "dense", "relu", "dense"], spec.n_hypers,
                       burnin=2, sampling_step=2, networks_per_file=2)
    saved = []
    for it in range(1, 12):
        th = (theta + it).astype(np.float32)
        st_ = [s for pr in o.unflatten(spec, th) for s in pr]
        w.after_epoch(it, st_, [eta[i:i + 1] + it for i in range(eta.size)])
        if it > 2 and it % 2 == 0:
            saved.append(th)
    w.close()
    mats, hyp = o.load_networks(str(tmp_path / "run"))
    n_vis = mats[0].shape[0]          # the last, partially filled file is invisible to the reader
    assert n_vis == 4 and len(hyp) == 4
    for k in range(n_vis):
        got = np.concatenate([m[k].reshape(-1) for m in mats])
        np.testing.assert_allclose(got, saved[k], rtol=1e-6)


def test_hyper_chain_collapses_under_Q1():
    """Why BASELINE configs[4] (Cauchy DenseLayers, hyper-HMC on) has a degenerate hyper chain whatever runs it: with the
    reference's Cauchy 'log-density' (Q1, BNN_functions.py:51-55: + log(1+z^2)) the hyper target of a layer grows like
    -3 cnt log(g^2) as the scale g^2 -> 0, i.e. it is improper with a pole at g = 0.  Driven by the reference's own dual
    averaging (network.py:457-469) the fp64 oracle's chain -- no GPU code involved -- falls onto the pole: the scale of
    the 10,000-weight layer drops by orders of magnitude within 100 epochs and the mean acceptance stays far below the
    0.95 target.  With GaussianDenseLayer priors (a proper target) the same loop settles near the target."""
    res = {}
    for name, prior in (("cauchy", o.PRIOR_CAUCHY), ("gaussian", o.PRIOR_GAUSSIAN)):
        spec, X, Y, theta, eta = o.synth_problem([20, 100, 100, 2], 16, o.ACT_RELU, prior, o.LIK_BERNOULLI)
        # the pole: the target increases monotonically as g_w of layer 1 shrinks (cauchy only)
        vals = []
        for g in (0.7, 0.07, 0.007, 0.0007):
            e = eta.astype(np.float64).copy(); e[5] = g
            vals.append(o.hyper_log_prob(spec, e, theta, X, Y, np.float64))
        res[name + "_monotone"] = all(b > a for a, b in zip(vals, vals[1:]))
        da = o.DualAveragingState(hyper_step_size=1e-2, burnin=10 ** 9)
        rng = np.random.default_rng(99)
        e, acc = eta.astype(np.float64), []
        with np.errstate(all="ignore"):
            for ep in range(100):
                p0 = rng.standard_normal(spec.n_hypers).astype(np.float32)
                r = o.hyper_step(spec, e, theta, X, Y, float(np.float32(da.eps_h)), 100, p0, float(np.log(rng.random())), np.float64)
                e = r.theta.astype(np.float64)
                acc.append(o.dual_averaging_update(da, ep, r.log_accept_ratio))
        res[name] = (abs(e[5]) / eta[5], float(np.mean(acc[50:])))
    assert res["cauchy_monotone"] and not res["gaussian_monotone"]
    assert res["cauchy"][0] < 0.5 and res["cauchy"][1] < 0.5, res          # scale collapsing, acceptance poor
    assert 0.5 < res["gaussian"][0] < 2.0 and res["gaussian"][1] > 0.7, res
