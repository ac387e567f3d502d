"""What tbnn_forward_many and the ensemble reductions refuse, message for message.  Every case below calls one entry point through
native.lib with exactly ONE bad argument and pins the return code (< 0) and the whole tbnn_last_error() text; after each, a valid
tbnn_ensemble_moments call on the same handle still succeeds.  The texts are those of the library's host code (csrc/ensemble_api.hpp); the
numbers test the other GPU modules.  Every case is refused before a kernel runs, so the shapes are as small as they can be.

Two handles: A, a 2-3-2 tanh network under a Gaussian likelihood with 16 training rows staged and no validation rows (P = 17); B, the same
as 2-3-1 (P = 13), for the two messages that need one output.  m = 16 networks, thetas [16, P], theta_stride = P.

Left out, because two arguments are wrong at once there and the entry points did not agree on which to report (NOTES.md lists them): a
row count that does not match the staged rows together with null thetas or theta_stride < P.  "No staged targets" needs rows staged
without targets, which no binding of this package does.  The over-budget m is given with the 16-network thetas (and a chain count
of 1, so that m divides): the call has to be refused before thetas, sd or weights are read beyond what exists -- all five entry points
with a block budget judge it before they read thetas, so none is left out."""
import ctypes as C
import math

import numpy as np
import pytest

FP, DP = C.POINTER(C.c_float), C.POINTER(C.c_double)
LIK_GAUSSIAN, LIK_BERNOULLI, LIK_CATEGORICAL, LIK_POISSON = 0, 2, 3, 5
XFORM_SOFTMAX, QUANT_LINEAR, QUANT_INVERTED_CDF = 3, 0, 1
M, ROWS = 16, 16
DIMS = {"A": [2, 3, 2], "B": [2, 3, 1]}

_rng = np.random.default_rng(2026)
TH = {k: (_rng.standard_normal((M, sum(d[i] * d[i + 1] + d[i + 1] for i in range(2)))) * 0.35).astype(np.float32) for k, d in DIMS.items()}
X = _rng.standard_normal((ROWS, 2)).astype(np.float32)
Y = {k: _rng.standard_normal((ROWS, d[-1])).astype(np.float32) for k, d in DIMS.items()}
W = np.linspace(0.5, 2.0, M).astype(np.float32)


def changed(a, i, v):
    b = a.copy()
    b[i] = v
    return b


W_NEG, W_INF, W_NAN, W_ZERO = changed(W, 3, -1.0), changed(W, 3, math.inf), changed(W, 3, math.nan), np.zeros(M, dtype=np.float32)
SD = np.full(M, 0.5, dtype=np.float32)
SD_NAN = changed(SD, 5, math.nan)
PROBS = np.array([0.1, 0.5, 0.9])
PROBS65 = np.linspace(0.01, 0.99, 65)
SERIES = _rng.standard_normal((M, 5)).astype(np.float32)
O32, O64 = [np.empty(4096, dtype=np.float32)], [np.empty(4096) for _ in range(5)]      # results (none is read)
TH_, P_, Y_ = "thetas of the handle", "P of the handle", "targets of the handle"

# the arguments of every entry point after the handle, in order, with values that make a valid call
ARGS = {
    "forward_many": dict(thetas=TH_, m=M, theta_stride=P_, which=0, X=None, n=0, out=O32[0]),
    "ensemble_moments": dict(thetas=TH_, m=M, theta_stride=P_, net_w=None, xform=0, scale=C.c_float(1.0), shift=C.c_float(0.0), which=0, X=None,
                             n=0, mean_out=O64[0], var_out=O64[1]),
    "ensemble_quantiles": dict(thetas=TH_, m=M, theta_stride=P_, net_w=None, method=QUANT_LINEAR, xform=0, scale=C.c_float(1.0),
                               shift=C.c_float(0.0), which=0, X=None, n=0, probs=PROBS, n_probs=3, out=O64[0]),
    "ensemble_diagnostics": dict(thetas=TH_, m=M, theta_stride=P_, n_chains=2, xform=0, scale=C.c_float(1.0), shift=C.c_float(0.0), which=0,
                                 X=None, n=0, rhat_out=O64[0], ess_out=O64[1]),
    "series_diagnostics": dict(series=SERIES, m=M, tot=5, n_chains=2, rhat_out=O64[0], ess_out=O64[1]),
    "ensemble_loglik": dict(thetas=TH_, m=M, theta_stride=P_, likelihood=LIK_GAUSSIAN, sd=SD, net_w=None, which=0, X=None, Y=None, n=0,
                            per_net=O64[0], lppd_rows=O64[1]),
    "ensemble_predictive": dict(thetas=TH_, m=M, theta_stride=P_, likelihood=LIK_GAUSSIAN, sd=SD, net_w=None, which=0, X=None, Y=None, n=0,
                                probs=PROBS, n_probs=3, q_out=O64[0], cdf_out=O64[1], cdf_below_out=None),
    "ensemble_loo": dict(thetas=TH_, m=M, theta_stride=P_, likelihood=LIK_GAUSSIAN, sd=SD, which=0, X=None, Y=None, n=0,
                         r_eff=C.c_double(1.0), elpd_loo_rows=O64[0], pareto_k_rows=O64[1], lppd_rows=O64[2], p_waic_rows=O64[3], pointwise=O64[4]),
}

NULL_M_STRIDE = "{who}: null pointer, m < 1 or theta_stride < P"
WHICH = "which must be 0 (training rows) or 1 (validation rows)"
NO_VALIDATION = "tbnn_set_validation has not been called"
BUDGET = "{who}: 64 rows of all m networks exceed the block budget of 2^28 floats"
XFORM = "{who}: unknown transform"
SOFTMAX = "{who}: a softmax needs at least 2 outputs (one logit per class)"
LIK = "{who}: unknown likelihood"
CATEGORICAL = "{who}: the categorical likelihood needs at least 2 outputs (one logit per class)"
X_NO_Y = "{who}: rows X without their targets Y"
MISMATCH = "{who}: n = 15 does not match the 16 staged rows"
SD_MSG = "{who}: sd 5 is not a number"
N_PROBS = "{who}: n_probs must be 1 .. 64"
# what every entry point over thetas and rows refuses alike (ensemble_api.hpp: EnsStage::stage_rows)
ROWS_CASES = [(dict(thetas=None), NULL_M_STRIDE), (dict(theta_stride=-1), NULL_M_STRIDE), (dict(which=1), NO_VALIDATION), (dict(which=2), WHICH),
              (dict(X=X, n=0, Y=Y_), "{who}: n < 1")]
WEIGHT_CASES = [(dict(net_w=W_NEG), "{who}: weight 3 is negative"), (dict(net_w=W_INF), "{who}: weight 3 is not finite"),
                (dict(net_w=W_NAN), "{who}: weight 3 is not finite"), (dict(net_w=W_ZERO), "{who}: all weights are zero")]
CHAIN_CASES = [(dict(rhat_out=None, ess_out=None), "{who}: rhat_out and ess_out are both null"),
               (dict(n_chains=0), "{who}: n_chains must be 1 .. 64"), (dict(n_chains=65), "{who}: n_chains must be 1 .. 64"),
               (dict(m=0), NULL_M_STRIDE), (dict(n_chains=3), "{who}: m is not divisible by n_chains"),
               (dict(n_chains=4), "{who}: fewer than 8 draws per chain")]

# entry point -> [(handle, the one argument changed, the message)]; theta_stride = -1 stands for P - 1
TABLE = {
    "forward_many": [("A", dict(out=None), NULL_M_STRIDE), ("A", dict(m=0), NULL_M_STRIDE)] + [("A", a, e) for a, e in ROWS_CASES],
    "ensemble_moments": [("A", dict(mean_out=None), "{who}: null mean_out"), ("A", dict(xform=4), XFORM), ("A", dict(xform=-1), XFORM),
                         ("B", dict(xform=XFORM_SOFTMAX), SOFTMAX), ("A", dict(m=0), NULL_M_STRIDE)]
                        + [("A", a, e) for a, e in WEIGHT_CASES + ROWS_CASES],
    "ensemble_quantiles": [("A", dict(probs=None), "{who}: null probs or out"), ("A", dict(out=None), "{who}: null probs or out"),
                           ("A", dict(n_probs=0), N_PROBS), ("A", dict(probs=PROBS65, n_probs=65), N_PROBS),
                           ("A", dict(probs=changed(PROBS, 1, 1.5)), "{who}: probability 1 is not in [0, 1]"),
                           ("A", dict(probs=changed(PROBS, 2, math.nan)), "{who}: probability 2 is not in [0, 1]"),
                           ("A", dict(method=2), "{who}: unknown method"), ("A", dict(xform=4), XFORM), ("B", dict(xform=XFORM_SOFTMAX), SOFTMAX),
                           ("A", dict(m=0), NULL_M_STRIDE),
                           ("A", dict(net_w=W), "{who}: TBNN_QUANT_LINEAR takes no weights (TBNN_QUANT_INVERTED_CDF does)"),
                           ("A", dict(m=(1 << 21) + 1), BUDGET)]
                          + [("A", dict(a, method=QUANT_INVERTED_CDF), e) for a, e in WEIGHT_CASES] + [("A", a, e) for a, e in ROWS_CASES],
    "ensemble_diagnostics": [("A", a, e) for a, e in CHAIN_CASES]
                            + [("A", dict(xform=4), XFORM), ("B", dict(xform=XFORM_SOFTMAX), SOFTMAX), ("A", dict(m=(1 << 21) + 1, n_chains=1), BUDGET)]
                            + [("A", a, e) for a, e in ROWS_CASES],
    "series_diagnostics": [("A", a, e) for a, e in CHAIN_CASES]
                          + [("A", dict(series=None), "{who}: null series or tot < 1"), ("A", dict(tot=0), "{who}: null series or tot < 1"),
                             ("A", dict(m=(1 << 22) + 1, n_chains=1), "{who}: 64 columns of all m draws exceed the block budget of 2^28 floats")],
    "ensemble_loglik": [("A", dict(per_net=None, lppd_rows=None), "{who}: per_net and lppd_rows are both null"), ("A", dict(likelihood=4), LIK),
                        ("A", dict(likelihood=6), LIK), ("B", dict(likelihood=LIK_CATEGORICAL), CATEGORICAL), ("A", dict(X=X, n=ROWS), X_NO_Y),
                        ("A", dict(m=0), NULL_M_STRIDE), ("A", dict(sd=SD_NAN), SD_MSG), ("A", dict(Y=Y_, n=15), MISMATCH)]
                       + [("A", a, e) for a, e in WEIGHT_CASES + ROWS_CASES],
    "ensemble_predictive": [("A", dict(q_out=None, cdf_out=None), "{who}: q_out and cdf_out are both null"),
                            ("A", dict(probs=None), "{who}: null probs with q_out"),
                            ("A", dict(likelihood=LIK_POISSON, cdf_out=None, cdf_below_out=O64[2]), "{who}: cdf_below_out without cdf_out"),
                            ("A", dict(X=X, n=ROWS), X_NO_Y), ("A", dict(n_probs=0), N_PROBS), ("A", dict(probs=PROBS65, n_probs=65), N_PROBS),
                            ("A", dict(probs=changed(PROBS, 0, 0.0)), "{who}: probability 0 is not in (0, 1)"),
                            ("A", dict(probs=changed(PROBS, 2, 1.0)), "{who}: probability 2 is not in (0, 1)"),
                            ("A", dict(likelihood=LIK_BERNOULLI),
                             "{who}: the predictive distribution of a label is its posterior-mean probability: tbnn_ensemble_moments returns it"),
                            ("A", dict(likelihood=4), LIK),
                            ("A", dict(cdf_below_out=O64[2]), "{who}: cdf_below_out is for TBNN_LIK_POISSON (a continuous CDF has no step)"),
                            ("A", dict(m=0), NULL_M_STRIDE), ("A", dict(m=(1 << 21) + 1), BUDGET), ("A", dict(sd=SD_NAN), SD_MSG),
                            ("A", dict(Y=Y_, n=15), MISMATCH)]
                           + [("A", a, e) for a, e in WEIGHT_CASES + ROWS_CASES],
    "ensemble_loo": [("A", dict(elpd_loo_rows=None, pareto_k_rows=None, lppd_rows=None, p_waic_rows=None, pointwise=None), "{who}: every output is null"),
                     ("A", dict(r_eff=C.c_double(0.0)), "{who}: r_eff must be finite and > 0"),
                     ("A", dict(r_eff=C.c_double(math.inf)), "{who}: r_eff must be finite and > 0"), ("A", dict(likelihood=4), LIK),
                     ("B", dict(likelihood=LIK_CATEGORICAL), CATEGORICAL), ("A", dict(X=X, n=ROWS), X_NO_Y),
                     ("A", dict(m=1), "{who}: fewer than 2 networks"), ("A", dict(m=1_500_000), BUDGET), ("A", dict(sd=SD_NAN), SD_MSG),
                     ("A", dict(Y=Y_, n=15), MISMATCH)]
                    + [("A", a, e) for a, e in ROWS_CASES],
}
CASES = [(entry, hd, chg, msg.format(who=entry)) for entry, rows in TABLE.items() for hd, chg, msg in rows]


def call(native, entry, handle, key, changes):
    """the entry point with ARGS[entry] and `changes` (those it takes: the shared row cases name Y, which not every entry point has), the
    placeholders resolved for the handle `key`"""
    args = dict(ARGS[entry])
    args.update({k: v for k, v in changes.items() if k in args})
    th = TH[key]
    out = []
    for name, v in args.items():
        if isinstance(v, str):
            v = {TH_: th, P_: th.shape[1], Y_: Y[key]}[v]
        if name == "theta_stride" and v == -1:
            v = th.shape[1] - 1
        if isinstance(v, np.ndarray):
            v = v.ctypes.data_as(FP if v.dtype == np.float32 else DP)
        out.append(v)
    return getattr(native.lib, "tbnn_" + entry)(handle, *out)


@pytest.fixture(scope="module")
def handles(native):
    hs = {}
    for key, d in DIMS.items():
        ch = native.Chain([(d[0], d[1], native.ACT_TANH, 0), (d[1], d[2], native.ACT_NONE, 0)], likelihood=native.LIK_GAUSSIAN, fixed_sd=0.7)
        ch.set_data(X, Y[key])
        hs[key] = ch
    yield hs
    for ch in hs.values():
        ch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(ARGS))
def test_the_unchanged_arguments_are_accepted(native, handles, entry):
    for key in DIMS:
        assert call(native, entry, handles[key]._h, key, {}) == 0, native.lib.tbnn_last_error().decode()


@pytest.mark.gpu
@pytest.mark.parametrize("entry,key,changes,message", CASES, ids=[f"{e}-{k}-{i}" for i, (e, k, _c, _m) in enumerate(CASES)])
def test_one_bad_argument(native, handles, entry, key, changes, message):
    rc = call(native, entry, handles[key]._h, key, changes)
    assert rc < 0 and native.lib.tbnn_last_error().decode() == message, (rc, native.lib.tbnn_last_error().decode())
    assert call(native, "ensemble_moments", handles[key]._h, key, {}) == 0, native.lib.tbnn_last_error().decode()


def test_null_handle(native):
    for entry in ARGS:
        assert call(native, entry, None, "A", {}) < 0, entry
        assert native.lib.tbnn_last_error().decode() == "null handle", entry
