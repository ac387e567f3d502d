"""Likelihood plug-ins (reference: tensorBNN/likelihood.py).

Descriptors for the native library (``kind``, ``fixed_sd``, ``hypers``,
``mainProbsInHypers``) with the reference's class names and keyword
constructors.  ``makeResponseLikelihood`` keeps the reference's keyword
protocol as a NumPy helper for post-processing code; the sampler evaluates the
likelihood inside the fused HIP kernel, never through it.
"""
import math

import numpy as np

from . import _native as nat
from .layer import _multivariate_log_prob


class Likelihood(object):
    kind = None
    fixed_sd = 0.1

    def __init__(self, *argv, **kwargs):
        self.hypers = []
        self.mainProbsInHypers = False

    def makeResponseLikelihood(self, *argv, **kwargs):
        self.hypers = []

    def calcultateLogProb(self, *argv, **kwargs):   # (sic) likelihood.py:98
        pass

    def display(self, hypers):
        pass


class GaussianLikelihood(Likelihood):
    """likelihood.py:63-133: sd is a hyper-parameter stored as sqrt(sd)."""
    kind = nat.LIK_GAUSSIAN

    def __init__(self, *argv, **kwargs):
        self.hypers = [[kwargs["sd"] ** 0.5]]          # :66
        self.mainProbsInHypers = True                  # :67

    def makeResponseLikelihood(self, *argv, **kwargs):
        sd = np.float32(np.asarray(kwargs["hyperStates"][-1]).reshape(-1)[0] ** 2)    # :88
        current = np.asarray(kwargs["predict"](True, argv[0])).T                       # :90-91
        real = np.asarray(kwargs["realVals"], dtype=np.float32).reshape(current.shape)
        return _multivariate_log_prob(np.ones_like(current) * sd, current, real)

    def display(self, hypers):
        print("Loss Standard Deviation: ", float(np.asarray(hypers[-1]).reshape(-1)[0]) ** 2)   # :132


class FixedGaussianLikelihood(Likelihood):
    """likelihood.py:136-202: fixed sd (not squared), no hyper."""
    kind = nat.LIK_FIXED_GAUSSIAN

    def __init__(self, *argv, **kwargs):
        self.hypers = []
        self.sd = kwargs["sd"]
        self.fixed_sd = float(kwargs["sd"])
        self.mainProbsInHypers = False

    def makeResponseLikelihood(self, *argv, **kwargs):
        current = np.asarray(kwargs["predict"](True, argv[0])).T
        real = np.asarray(kwargs["realVals"], dtype=np.float32).reshape(current.shape)
        return _multivariate_log_prob(np.ones_like(current) * np.float32(self.sd), current, real)


class BernoulliLikelihood(Likelihood):
    """likelihood.py:205-243"""
    kind = nat.LIK_BERNOULLI

    def __init__(self, *argv, **kwargs):
        self.hypers = []
        self.mainProbsInHypers = False

    def makeResponseLikelihood(self, *argv, **kwargs):
        p = np.clip(np.asarray(kwargs["predict"](True, argv[0]), dtype=np.float32), 1e-8, 1 - 1e-7)   # :226-231
        y = np.asarray(kwargs["realVals"], dtype=np.float32).reshape(-1, p.shape[0]).T
        return np.where(y == 0, 0, y * np.log(p)) + np.where(1 - y == 0, 0, (1 - y) * np.log1p(-p))

    def calcultateLogProb(self, *argv, **kwargs):
        return [np.float32(0) for _ in range(len(kwargs["hypers"]))]


def log_softmax(f, axis=0):
    """log softmax of logits along `axis`, shifted by their max (finite for any finite logits)"""
    f = np.asarray(f, dtype=np.float64)
    d = f - np.max(f, axis=axis, keepdims=True)
    return d - np.log(np.sum(np.exp(d), axis=axis, keepdims=True))


class CategoricalLikelihood(Likelihood):
    """Multi-class classification: the last dense layer's d_out >= 2 outputs, with no activation after it, are a row's logits, and
    the data term is sum_rows sum_k y_k log softmax_k(f) for one-hot or probability rows y (include/tbnn.h TBNN_LIK_CATEGORICAL).
    Unlike K BernoulliLikelihood outputs, the class probabilities of a row sum to one.  No hyper-parameter."""
    kind = nat.LIK_CATEGORICAL

    def __init__(self, *argv, **kwargs):
        self.hypers = []
        self.mainProbsInHypers = False

    def makeResponseLikelihood(self, *argv, **kwargs):
        """y_k log softmax_k(f) per (output, row), [d_out, rows] as BernoulliLikelihood's; the sum is the data term"""
        f = np.asarray(kwargs["predict"](True, argv[0]), dtype=np.float64)        # [d_out, rows]
        y = np.asarray(kwargs["realVals"], dtype=np.float64).reshape(-1, f.shape[0]).T
        return y * log_softmax(f, axis=0)

    def calcultateLogProb(self, *argv, **kwargs):
        return [np.float32(0) for _ in range(len(kwargs["hypers"]))]


class PoissonLikelihood(Likelihood):
    """Count data: the last dense layer's outputs, with no activation after it, are the LOGS of the rates (log link), one independent
    rate per output, and the data term is sum over (row, output) of y f - exp(f) - lgamma(y + 1) for targets y >= 0 (non-integers
    allowed; include/tbnn.h TBNN_LIK_POISSON).  No hyper-parameter."""
    kind = nat.LIK_POISSON

    def __init__(self, *argv, **kwargs):
        self.hypers = []
        self.mainProbsInHypers = False

    def makeResponseLikelihood(self, *argv, **kwargs):
        """y f - exp(f) - lgamma(y + 1) per (output, row) in float64, [d_out, rows] as BernoulliLikelihood's; the sum is the data term"""
        f = np.asarray(kwargs["predict"](True, argv[0]), dtype=np.float64)        # [d_out, rows]: log-rates
        y = np.asarray(kwargs["realVals"], dtype=np.float64).reshape(-1, f.shape[0]).T
        return y * f - np.exp(f) - np.vectorize(math.lgamma, otypes=[np.float64])(y + 1.0)

    def calcultateLogProb(self, *argv, **kwargs):
        return [np.float32(0) for _ in range(len(kwargs["hypers"]))]


class StudentTLikelihood(Likelihood):
    """Robust regression: independent Student-t noise of fixed scale `sd` and `df` degrees of freedom around each output (any
    activation the Gaussian kinds take).  Per (row, output), r = y - f:
    log p = lgamma((df+1)/2) - lgamma(df/2) - 1/2 log(df pi) - log sd - (df+1)/2 log1p(r^2 / (df sd^2))  (include/tbnn.h
    TBNN_LIK_STUDENT_T).  A row's pull on the fit, (df+1) r / (df sd^2 + r^2), is bounded: a few gross outliers do not decide the
    posterior as they do under FixedGaussianLikelihood, which this likelihood approaches as df grows.  No hyper-parameter."""
    kind = nat.LIK_STUDENT_T

    def __init__(self, *argv, **kwargs):
        self.hypers = []
        self.sd = kwargs["sd"]
        self.fixed_sd = float(kwargs["sd"])
        self.df = float(kwargs["df"])
        if not (self.fixed_sd > 0 and math.isfinite(self.fixed_sd)) or not (self.df > 0 and math.isfinite(self.df)):
            raise ValueError("StudentTLikelihood needs sd > 0 and df > 0, both finite")
        self.mainProbsInHypers = False

    def logDensity(self, f, y, sd=None):
        """the log density of y around f, element by element in float64 (sd: the scale, default the likelihood's own)"""
        s = np.clip(np.float64(self.fixed_sd if sd is None else sd), 1e-8, 1e8)          # (clipped as the Gaussian kinds clip theirs)
        nu = self.df
        c = math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi) - np.log(s)
        r = (np.asarray(y, dtype=np.float64) - np.asarray(f, dtype=np.float64)) / s
        return c - 0.5 * (nu + 1.0) * np.log1p(r * r / nu)

    def makeResponseLikelihood(self, *argv, **kwargs):
        """the log density per (output, row) in float64, [d_out, rows] as PoissonLikelihood's; the sum is the data term"""
        f = np.asarray(kwargs["predict"](True, argv[0]), dtype=np.float64)        # [d_out, rows]
        y = np.asarray(kwargs["realVals"], dtype=np.float64).reshape(-1, f.shape[0]).T
        return self.logDensity(f, y)

    def calcultateLogProb(self, *argv, **kwargs):
        return [np.float32(0) for _ in range(len(kwargs["hypers"]))]


class NegativeBinomialLikelihood(Likelihood):
    """Over-dispersed counts: as PoissonLikelihood, the last dense layer's outputs (no activation after it) are the LOGS of the means, and
    each count is negative binomial with mean mu = exp(f) and variance mu + mu^2 / dispersion (dispersion -> inf: Poisson).  Per
    (row, output), p = mu / (dispersion + mu):
    log p(y | f) = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y log p + r log(1 - p)  (include/tbnn.h TBNN_LIK_NEG_BINOMIAL), targets
    y >= 0 (non-integers allowed).  A row's pull on the fit, r (y - mu) / (r + mu), is bounded by r from below however large the rate.
    No hyper-parameter: the dispersion is fixed (NegativeBinomialLikelihood(dispersion=r))."""
    kind = nat.LIK_NEG_BINOMIAL

    def __init__(self, *argv, **kwargs):
        self.hypers = []
        self.dispersion = float(kwargs["dispersion"])
        if not (self.dispersion > 0 and math.isfinite(self.dispersion)):
            raise ValueError("NegativeBinomialLikelihood needs dispersion > 0 and finite")
        self.mainProbsInHypers = False

    def logDensity(self, f, y):
        """the log density of the counts y at log-means f, element by element in float64, in the form the kernels use: with
        t = f - log r, -log p = max(-t, 0) + log1p(e^-|t|) and -log(1 - p) = max(t, 0) + log1p(e^-|t|)"""
        r = self.dispersion
        lg = np.vectorize(math.lgamma, otypes=[np.float64])
        f = np.asarray(f, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        t = f - math.log(r)
        l = np.log1p(np.exp(-np.abs(t)))
        return (lg(y + r) - math.lgamma(r) - lg(y + 1.0)) - (y * (np.maximum(-t, 0.0) + l) + r * (np.maximum(t, 0.0) + l))

    def makeResponseLikelihood(self, *argv, **kwargs):
        """the log density per (output, row) in float64, [d_out, rows] as PoissonLikelihood's; the sum is the data term"""
        f = np.asarray(kwargs["predict"](True, argv[0]), dtype=np.float64)        # [d_out, rows]: log-means
        y = np.asarray(kwargs["realVals"], dtype=np.float64).reshape(-1, f.shape[0]).T
        return self.logDensity(f, y)

    def calcultateLogProb(self, *argv, **kwargs):
        return [np.float32(0) for _ in range(len(kwargs["hypers"]))]


class HeteroscedasticGaussianLikelihood(Likelihood):
    """Regression whose noise scale the network predicts: the last dense layer has EXACTLY 2 outputs with no activation after it, output 0
    the mean f and output 1 the log of the standard deviation g, and y ~ N(f, exp(g)^2) row by row (include/tbnn.h
    TBNN_LIK_HETERO_GAUSSIAN).  With G = log(1e8), gc = clip(g, -G, G):  log p(y | f, g) = -1/2 log(2 pi) - gc - 1/2 (y - f)^2 exp(-2 gc).
    One target per row (trainY [n] or [n, 1]; [n, 2] is taken with column 1 ignored).  predict returns both outputs, [2, rows]: the mean
    and the log-sd.  No hyper-parameter."""
    kind = nat.LIK_HETERO_GAUSSIAN
    LOG_CLIP = math.log(1e8)

    def __init__(self, *argv, **kwargs):
        self.hypers = []
        self.mainProbsInHypers = False

    def logDensity(self, f, g, y):
        """the log density of y under N(f, exp(g)^2), element by element in float64 (g clipped to +-log(1e8))"""
        gc = np.clip(np.asarray(g, dtype=np.float64), -self.LOG_CLIP, self.LOG_CLIP)
        r = np.asarray(y, dtype=np.float64) - np.asarray(f, dtype=np.float64)
        return -0.5 * math.log(2.0 * math.pi) - gc - 0.5 * r * r * np.exp(-2.0 * gc)

    def makeResponseLikelihood(self, *argv, **kwargs):
        """the log density per row in float64, [1, rows]; the sum is the data term.  realVals: [rows], [rows, 1] or [rows, 2] (column 0)"""
        f = np.asarray(kwargs["predict"](True, argv[0]), dtype=np.float64)        # [2, rows]: mean, log-sd
        y = np.asarray(kwargs["realVals"], dtype=np.float64)
        y = y.reshape(-1) if y.size == f.shape[1] else y.reshape(f.shape[1], -1)[:, 0]
        return self.logDensity(f[0], f[1], y)[None, :]

    def calcultateLogProb(self, *argv, **kwargs):
        return [np.float32(0) for _ in range(len(kwargs["hypers"]))]


class GammaLikelihood(Likelihood):
    """Positive, continuous, right-skewed targets (durations, amounts, concentrations): the last dense layer's outputs (no activation after
    it) are the LOGS of the means, and each target is Gamma distributed with mean mu = exp(f) and the fixed shape a:
    Var = mu^2 / shape, a constant coefficient of variation 1 / sqrt(shape); shape = 1 is the exponential distribution.  Per (row, output):
    log p(y | f) = a log a - lgamma(a) + (a - 1) log y - a f - a y exp(-f)  (include/tbnn.h TBNN_LIK_GAMMA), targets finite, > 0 and at most 2^100
    (1.27e30: the staging call refuses a larger one, and zero).
    No hyper-parameter: the shape is fixed (GammaLikelihood(shape=a))."""
    kind = nat.LIK_GAMMA

    def __init__(self, *argv, **kwargs):
        self.hypers = []
        self.shape = float(kwargs["shape"])
        if not (self.shape > 0 and math.isfinite(self.shape)):
            raise ValueError("GammaLikelihood needs shape > 0 and finite")
        self.mainProbsInHypers = False

    def logDensity(self, f, y):
        """the log density of the targets y > 0 at log-means f, element by element in float64"""
        a = self.shape
        f = np.asarray(f, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        return (a * math.log(a) - math.lgamma(a)) + (a - 1.0) * np.log(y) - a * (f + y * np.exp(-f))

    def makeResponseLikelihood(self, *argv, **kwargs):
        """the log density per (output, row) in float64, [d_out, rows] as PoissonLikelihood's; the sum is the data term"""
        f = np.asarray(kwargs["predict"](True, argv[0]), dtype=np.float64)        # [d_out, rows]: log-means
        y = np.asarray(kwargs["realVals"], dtype=np.float64).reshape(-1, f.shape[0]).T
        return self.logDensity(f, y)

    def calcultateLogProb(self, *argv, **kwargs):
        return [np.float32(0) for _ in range(len(kwargs["hypers"]))]


class WeibullLikelihood(Likelihood):
    """Times to an event, some rows right-censored (survival data: time to failure, to relapse, to churn): the last dense layer's outputs
    (no activation after it) are the LOGS of the Weibull scales, lambda = exp(f) (the accelerated-failure-time parameterisation), and the
    shape k is fixed (WeibullLikelihood(shape=k)); shape = 1 is the exponential model.  Censoring travels in the SIGN of the target:
    y > 0 is an event observed at time y, y < 0 a row still running at time |y| (`encode` builds such targets).  With t = |y| and
    u = (t exp(-f))^k, per (row, output): an event gives log p = log k + (k - 1) log t - k f - u, a censored row log S = -u
    (include/tbnn.h TBNN_LIK_WEIBULL); targets finite, nonzero, 2^-100 <= |y| <= 2^100.  No hyper-parameter."""
    kind = nat.LIK_WEIBULL

    def __init__(self, *argv, **kwargs):
        self.hypers = []
        self.shape = float(kwargs["shape"])
        if not (self.shape > 0 and math.isfinite(self.shape)):
            raise ValueError("WeibullLikelihood needs shape > 0 and finite")
        self.mainProbsInHypers = False

    @staticmethod
    def encode(times, observed):
        """the signed float32 targets of the event times `times` (> 0) and the flags `observed` (true: the event was seen at that time;
        false: the row was right-censored then): +t for an event, -t for a censored row, in the shape of `times`"""
        t = np.asarray(times, dtype=np.float32)
        d = np.broadcast_to(np.asarray(observed).astype(bool), t.shape)
        if not (np.all(np.isfinite(t)) and np.all(t > 0)):
            raise ValueError("WeibullLikelihood.encode: times must be finite and > 0 (the sign of a target is its censoring flag)")
        return np.where(d, t, -t).astype(np.float32)

    def logDensity(self, f, y):
        """element by element in float64, at log-scales f: the log density of an event target (y > 0), the log survival function of a
        right-censored one (y < 0)"""
        k = self.shape
        f = np.asarray(f, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        lt = np.log(np.abs(y))
        u = np.exp(k * (lt - f))
        return np.where(y > 0, (math.log(k) + (k - 1.0) * lt - k * f) - u, -u)

    def makeResponseLikelihood(self, *argv, **kwargs):
        """the term per (output, row) in float64, [d_out, rows] as GammaLikelihood's; the sum is the data term"""
        f = np.asarray(kwargs["predict"](True, argv[0]), dtype=np.float64)        # [d_out, rows]: log-scales
        y = np.asarray(kwargs["realVals"], dtype=np.float64).reshape(-1, f.shape[0]).T
        return self.logDensity(f, y)

    def calcultateLogProb(self, *argv, **kwargs):
        return [np.float32(0) for _ in range(len(kwargs["hypers"]))]
