"""Ensemble prediction over saved networks (reference: tensorBNN/predictor.py:15-155).

Reads the reference's on-disk sample format (summary.txt, <n>.<k>.txt,
hypers<k>.txt, architecture.txt; writer network.py:545-663) and runs the
forward pass of every saved network through the native forward kernel.
``trainProbs`` / ``reweight`` (predictor.py:157-273) follow the reference where the
reference runs (likelihood=None: the per-network sum of ``calculateHyperProbs``) and its
intent where it cannot: with a likelihood the reference raises (GaussianLikelihood reads a
``sd`` keyword nobody passes, likelihood.py:116-119; the Fixed-Gaussian one transposes the
rows twice, predictor.py:174 + :141, and never reduces over them) -- here the data term is
the summed log-likelihood of the training rows under each saved network, computed from one
``tbnn_forward_many`` call.  ``autocorrelation`` / ``autoCorrelationLength``
(predictor.py:275-312) use ``emcee.autocorr`` in the reference (un-vendored, emcee 3.x):
``function_1d`` and ``integrated_time`` are restated below from its published algorithm
(FFT autocorrelation; Sokal's automatic window with c = 5).
"""
import math
import os
from decimal import Decimal

import numpy as np

from . import _native as nat
from .activationFunctions import Relu, Sigmoid, Tanh
from .layer import CauchyDenseLayer, DenseLayer, GaussianDenseLayer
from .likelihood import GaussianLikelihood


class predictor(object):
    def __init__(self, directoryPath, dtype=np.float32, customLayerDict={}, likelihood=None, device=0):
        self.layerDict = {"relu": Relu, "sigmoid": Sigmoid, "tanh": Tanh, "dense": DenseLayer,
                          "denseGaussian": GaussianDenseLayer}                 # predictor.py:30-36
        self.layerDict.update(customLayerDict)
        self.directoryPath = directoryPath if directoryPath.endswith("/") else directoryPath + "/"
        self.dtype = np.float32
        self.device = device
        self.loadNetworks()
        self.loadArchitecture()
        self.likelihood = likelihood if likelihood is not None else GaussianLikelihood(sd=0.1)
        self._chain = None
        self.numChains = 1                                                      # fromChains: the networks are chains x draws, chain-major
        self.weightsTrain = []                                                  # predictor.py:40
        self.weights = []

    @classmethod
    def fromChains(cls, folderName, **kwargs):
        """The ensemble network.trainChains wrote: folderName/chain0 ... chain<C-1>, each a directory predictor(dir) reads.  The chains'
        networks are concatenated chain-major (network i = c S + s, S saved networks per chain) and numChains = C, which is what
        predictDiagnostics / parameterDiagnostics split by; every other method sees one ensemble of C S networks.  Chains with different
        numbers of saved networks or different architectures are refused."""
        dirs = []
        while os.path.isdir(os.path.join(folderName, "chain%d" % len(dirs))):
            dirs.append(os.path.join(folderName, "chain%d" % len(dirs)))
        if not dirs:
            raise ValueError(f"no chain0 directory under {folderName}")
        parts = [cls(d, **kwargs) for d in dirs]
        p = parts[0]
        shape = lambda q: ([type(l).__name__ for l in q.layers], [m.shape[1:] for m in q.matrices], len(q.hypers[0]) if len(q.hypers) else 0)
        for c, q in enumerate(parts[1:], 1):
            if q.numNetworks != p.numNetworks:
                raise ValueError(f"chain{c} holds {q.numNetworks} saved networks, chain0 {p.numNetworks}")
            if shape(q) != shape(p):
                raise ValueError(f"chain{c} has another architecture than chain0")
        p.matrices = [np.concatenate([q.matrices[i] for q in parts]) for i in range(p.numMatrices)]
        p.hypers = [h for q in parts for h in q.hypers]
        p.vectors = [v for q in parts for v in q.vectors]
        p.numChains = len(parts)
        p.numNetworks = p.numChains * p.numNetworks
        return p

    def loadNetworks(self):
        """predictor.py:43-113"""
        summary = []
        with open(self.directoryPath + "summary.txt", "r") as file:
            for line in iter(file):
                summary.append(line.split())
        numNetworks = int(summary[-2][0])
        numFiles = int(summary[-2][1])
        numMatrices = int(summary[-2][2])
        numHypers = int(summary[-1][0])
        numNetworks //= numFiles
        matrices = []
        for n in range(numMatrices):
            d1 = int(summary[n][0])
            d2 = int(summary[n][1]) if len(summary[n]) == 2 else 1
            weights0 = np.zeros((numNetworks * numFiles, d1, d2), dtype=np.float32)
            for m in range(numFiles):
                weights = np.loadtxt(self.directoryPath + str(n) + "." + str(m) + ".txt", dtype=np.float32, ndmin=2)
                for k in range(numNetworks):
                    weights0[m * numNetworks + k, :, :] = weights[d1 * k:d1 * (k + 1), :d2]
            matrices.append(weights0)
        hypers = []
        if numHypers > 0:
            for m in range(numFiles):
                weights = np.loadtxt(self.directoryPath + "hypers" + str(m) + ".txt", dtype=np.float32, ndmin=1)
                for k in range(numNetworks):
                    hypers.append(weights[numHypers * k:numHypers * (k + 1)])
        self.numNetworks = numNetworks * numFiles
        self.numMatrices = numMatrices
        self.matrices = matrices
        self.hypers = hypers
        self.vectors = [np.concatenate([mat[i].reshape(-1) for mat in matrices]) for i in range(self.numNetworks)]

    def loadArchitecture(self, architecture=None):
        """predictor.py:115-130: layer classes looked up by name, built with (1, 1)."""
        path = self.directoryPath + "architecture.txt" if architecture is None else architecture
        self.layers = []
        with open(path, "r") as file:
            for line in iter(file):
                self.layers.append(self.layerDict[line.replace("\n", "")](inputDims=1, outputDims=1))

    def _descriptor(self):
        dense, mi = [], 0
        for layer in self.layers:
            if layer.numTensors > 0:
                out_dim, in_dim = self.matrices[mi].shape[1], self.matrices[mi].shape[2]
                dense.append([in_dim, out_dim, nat.ACT_NONE, layer.prior_kind])
                mi += layer.numTensors
            else:
                dense[-1][2] = layer.act_kind
        return dense

    def predict(self, inputMatrix, n=1):
        """predictor.py:132-155: list of [d_out, rows] predictions, every n-th network."""
        self._ensure_chain()
        x = np.asarray(inputMatrix, dtype=np.float32)
        # one native call for the whole ensemble (tbnn_forward_many): the rows are staged once, narrow networks run
        # as one batched launch of the forward-only MFMA kernel
        picked = np.stack([self.vectors[m] for m in range(0, self.numNetworks, n)])
        out = self._chain.forward_many(picked, X=x)
        assert out.shape[0] == math.ceil(self.numNetworks / n)
        return [out[i] for i in range(out.shape[0])]

    # ---- re-weighting (predictor.py:157-273) ----
    def _data_logprob(self, likelihood, trainX, trainY, n):
        """summed log-likelihood of the training rows under every n-th network (see the module docstring)"""
        from .layer import _multivariate_log_prob
        from .likelihood import (BernoulliLikelihood, CategoricalLikelihood, FixedGaussianLikelihood, GammaLikelihood,
                                 HeteroscedasticGaussianLikelihood, NegativeBinomialLikelihood, PoissonLikelihood, StudentTLikelihood,
                                 WeibullLikelihood, log_softmax)
        preds = self.predict(trainX, n)
        y = np.asarray(trainY, dtype=np.float32)
        out = []
        for i, f in enumerate(preds):
            cur = np.asarray(f, dtype=np.float32).T                             # [rows, d_out]
            if isinstance(likelihood, HeteroscedasticGaussianLikelihood):       # one target per row against the (mean, log-sd) pair
                out.append(np.float32(np.sum(likelihood.makeResponseLikelihood(None, predict=lambda *_a, _f=cur.T: _f, realVals=y))))
                continue
            real = y.reshape(cur.shape)
            if isinstance(likelihood, CategoricalLikelihood):
                out.append(np.float32(np.sum(real * log_softmax(cur, axis=1))))     # sum_rows sum_k y_k log softmax_k
                continue
            if isinstance(likelihood, (PoissonLikelihood, StudentTLikelihood, NegativeBinomialLikelihood, GammaLikelihood, WeibullLikelihood)):
                terms = likelihood.makeResponseLikelihood(None, predict=lambda *_a, _f=cur.T: _f, realVals=real)
                out.append(np.float32(np.sum(terms)))                           # sum of y f - exp(f) - lgamma(y + 1) / of the t / negative-binomial log densities
                continue
            if isinstance(likelihood, BernoulliLikelihood):
                out.append(np.float32(0))                                       # likelihood.py:239-243
                continue
            if isinstance(likelihood, FixedGaussianLikelihood):
                sd = np.float32(likelihood.sd)                                  # likelihood.py:195 (not squared)
            else:
                m = i * n
                sd = np.float32(self.hypers[m][-1]) if len(self.hypers) else np.float32(0.1)   # likelihood.py:116-117
            out.append(np.float32(np.sum(_multivariate_log_prob(np.ones_like(cur) * sd, cur, real))))
        return out

    # ---- reductions over the saved networks on the device (tbnn_ensemble_moments / tbnn_ensemble_quantiles / tbnn_ensemble_loglik) ----
    _TRANSFORMS = {"none": nat.XFORM_NONE, "exp": nat.XFORM_EXP, "sigmoid": nat.XFORM_SIGMOID, "softmax": nat.XFORM_SOFTMAX}

    def _transform(self, transform):
        """the name of the transform asked for; None: the one the predictor's likelihood implies"""
        from .likelihood import CategoricalLikelihood, GammaLikelihood, NegativeBinomialLikelihood, PoissonLikelihood, WeibullLikelihood
        if transform is None:
            transform = ("softmax" if isinstance(self.likelihood, CategoricalLikelihood) else
                         "exp" if isinstance(self.likelihood, (PoissonLikelihood, NegativeBinomialLikelihood, GammaLikelihood, WeibullLikelihood)) else "none")
        if transform not in self._TRANSFORMS:
            raise ValueError(f"transform must be one of {sorted(self._TRANSFORMS)} or None")
        return transform

    @staticmethod
    def _central_probs(level):
        """(1 - level) / 2, 1 / 2, (1 + level) / 2 -- in decimal, so that level = 0.9 asks for 0.05 and 0.95 themselves: (1 - 0.9) / 2 in
        binary is the double below 0.05"""
        level = float(level)
        if not 0.0 < level < 1.0:
            raise ValueError("level must lie in (0, 1)")
        d = Decimal(repr(level))
        return [float((1 - d) / 2), 0.5, float((1 + d) / 2)]

    def _picked(self, n, weights):
        picked = np.stack([self.vectors[m] for m in range(0, self.numNetworks, n)])
        w = None if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
        if w is not None and w.size != picked.shape[0]:
            raise ValueError(f"weights must hold one value per picked network ({picked.shape[0]})")
        return picked, w

    def predictMoments(self, inputMatrix, n=1, weights=None, transform=None, sd=1.0, mean=0.0, countVariance=False, noiseVariance=False):
        """Posterior-predictive mean and population variance of every n-th network's predictions, (mean, var) as float64 [d_out, rows],
        reduced on the device: only the two results cross to the host.  Per value t = transform(f) * sd + mean (the de-normalisation of
        the metrics).  transform None: softmax under a CategoricalLikelihood -- class probabilities averaged over the posterior, not
        averaged logits --, exp under a PoissonLikelihood or NegativeBinomialLikelihood -- the posterior mean and variance of the RATE --
        and none otherwise; "exp" / "sigmoid" / "softmax" / "none" override.  weights: one per picked network, e.g. what reweight
        returns.  countVariance (with the exp transform, sd = 1, mean = 0): the second array is the total predictive variance of a
        COUNT, E[rate] + Var[rate] (the Poisson noise plus the posterior spread of the rate) -- under a NegativeBinomialLikelihood
        E[rate] + Var[rate] + E[rate^2] / dispersion, E[rate^2] = Var[rate] + E[rate]^2 --, added on the host to the two arrays the
        device returns.
        Under a HeteroscedasticGaussianLikelihood the two outputs are the mean f and the log-sd g, and the plain call (like predict)
        returns the moments of both, [2, rows].  noiseVariance=True (that likelihood only; transform None, sd = 1, mean = 0): (E[f],
        Var[f] + E[s^2]), each [1, rows], s = exp(g) -- the total predictive variance of a new observation, the epistemic spread of the
        mean plus the expected noise variance; E[s^2] = Var[s] + E[s]^2 from a second reduction on the device under the exp transform.
        Under a GammaLikelihood the default transform is exp too (the mean mu itself), and noiseVariance=True (transform None or "exp",
        sd = 1, mean = 0) returns (E[mu], Var[mu] + E[mu^2] / shape): the posterior spread of the mean plus the expected Gamma noise
        variance mu^2 / shape, added on the host as countVariance is.
        Under a WeibullLikelihood the default transform is exp as well (the scale lambda), and noiseVariance=True (the same conditions)
        returns (E[m_i], Var[m_i] + E[v_i]) of the time to the event: each network's mean m_i = lambda_i Gamma(1 + 1/k) and variance
        v_i = lambda_i^2 (Gamma(1 + 2/k) - Gamma(1 + 1/k)^2), from the moments of lambda the device returns."""
        from .likelihood import GammaLikelihood, HeteroscedasticGaussianLikelihood, NegativeBinomialLikelihood, WeibullLikelihood
        if noiseVariance and isinstance(self.likelihood, WeibullLikelihood):
            if transform not in (None, "exp") or float(sd) != 1.0 or float(mean) != 0.0 or countVariance:
                raise ValueError("noiseVariance under a WeibullLikelihood needs the scale itself: transform None or 'exp', sd = 1, mean = 0, no "
                                 "countVariance")
            picked, w = self._picked(n, weights)
            m, v = self._ensure_chain().ensemble_moments(picked, X=np.asarray(inputMatrix, dtype=np.float32), weights=w, xform=nat.XFORM_EXP)
            k = self.likelihood.shape
            g1, g2 = math.gamma(1.0 + 1.0 / k), math.gamma(1.0 + 2.0 / k)
            return g1 * m, g1 * g1 * v + (g2 - g1 * g1) * (v + m * m)
        if noiseVariance and isinstance(self.likelihood, GammaLikelihood):
            if transform not in (None, "exp") or float(sd) != 1.0 or float(mean) != 0.0 or countVariance:
                raise ValueError("noiseVariance under a GammaLikelihood needs the mean itself: transform None or 'exp', sd = 1, mean = 0, no "
                                 "countVariance")
            picked, w = self._picked(n, weights)
            m, v = self._ensure_chain().ensemble_moments(picked, X=np.asarray(inputMatrix, dtype=np.float32), weights=w, xform=nat.XFORM_EXP)
            return m, v + (v + m * m) / self.likelihood.shape
        if noiseVariance:
            if not isinstance(self.likelihood, HeteroscedasticGaussianLikelihood):
                raise ValueError("noiseVariance needs a HeteroscedasticGaussianLikelihood: only there does the network predict its noise")
            if transform is not None or float(sd) != 1.0 or float(mean) != 0.0 or countVariance:
                raise ValueError("noiseVariance takes the outputs as they are: transform None, sd = 1, mean = 0, no countVariance")
            picked, w = self._picked(n, weights)
            ch = self._ensure_chain()
            x = np.asarray(inputMatrix, dtype=np.float32)
            m, v = ch.ensemble_moments(picked, X=x, weights=w, xform=nat.XFORM_NONE)
            ms, vs = ch.ensemble_moments(picked, X=x, weights=w, xform=nat.XFORM_EXP)
            return m[:1], v[:1] + (vs[1:2] + ms[1:2] * ms[1:2])
        transform = self._transform(transform)
        if countVariance and (transform != "exp" or float(sd) != 1.0 or float(mean) != 0.0):
            raise ValueError("countVariance needs the rate itself: transform 'exp' (the default under a PoissonLikelihood), sd = 1, mean = 0")
        picked, w = self._picked(n, weights)
        ch = self._ensure_chain()
        m, v = ch.ensemble_moments(picked, X=np.asarray(inputMatrix, dtype=np.float32), weights=w, xform=self._TRANSFORMS[transform],
                                   scale=float(sd), shift=float(mean))
        if countVariance and isinstance(self.likelihood, NegativeBinomialLikelihood):
            return m, m + v + (v + m * m) / self.likelihood.dispersion
        return (m, m + v) if countVariance else (m, v)

    def predictQuantiles(self, inputMatrix, probs, n=1, weights=None, transform=None, sd=1.0, mean=0.0, method=None):
        """Posterior quantiles of every n-th network's predictions at the probabilities `probs`, float64 [n_probs, d_out, rows] (a scalar
        `probs`: [d_out, rows]), selected on the device: only the result crosses to the host.  Per value t = transform(f) * sd + mean,
        transform None as in predictMoments (softmax under a CategoricalLikelihood, exp under a PoissonLikelihood, none otherwise) and
        applied before the ranking.  method "linear" is np.quantile's default and takes no weights; "inverted_cdf" returns one of the
        networks' values and takes weights (np.quantile(method="inverted_cdf", weights=weights)), e.g. what reweight returns.  method None:
        "linear" without weights, "inverted_cdf" with them."""
        transform = self._transform(transform)
        if method is None:
            method = "linear" if weights is None else "inverted_cdf"
        if method not in ("linear", "inverted_cdf"):
            raise ValueError("method must be 'linear', 'inverted_cdf' or None")
        if method == "linear" and weights is not None:
            raise ValueError("method 'linear' takes no weights (np.quantile refuses them too): use 'inverted_cdf'")
        picked, w = self._picked(n, weights)
        pr = np.asarray(probs, dtype=np.float64)
        ch = self._ensure_chain()
        q = ch.ensemble_quantiles(picked, pr.reshape(-1), X=np.asarray(inputMatrix, dtype=np.float32), weights=w, method=method,
                                  xform=self._TRANSFORMS[transform], scale=float(sd), shift=float(mean))
        return q[0] if pr.ndim == 0 else q

    def predictInterval(self, inputMatrix, level=0.9, **kwargs):
        """(lower, median, upper), each float64 [d_out, rows]: the quantiles at (1 - level) / 2, 1 / 2 and (1 + level) / 2 from one call
        of predictQuantiles, whose other arguments pass through.  This is the central CREDIBLE interval of the network's output -- the
        rate, the class probability, the regression mean -- under the posterior the saved networks sample; the predictive interval
        for a new observation, which adds the observation noise (sigma, the Poisson scatter), is predictiveInterval's."""
        q = self.predictQuantiles(inputMatrix, self._central_probs(level), **kwargs)
        return q[0], q[1], q[2]

    # ---- convergence diagnostics on the device (tbnn_ensemble_diagnostics / tbnn_series_diagnostics) ----
    @staticmethod
    def _diagnostics(rhat, ess):
        bad = np.isnan(rhat) | np.isnan(ess)
        ok = ~bad
        return {"rhat": rhat, "ess": ess, "max_rhat": float(rhat[ok].max()) if ok.any() else float("nan"),
                "min_ess": float(ess[ok].min()) if ok.any() else float("nan"), "undefined": int(bad.sum())}

    def _chain_draws(self, n=1):
        """network indices of every n-th draw of each chain, chain-major, and the draws per chain"""
        C = getattr(self, "numChains", 1)
        if self.numNetworks % C:
            raise ValueError(f"{self.numNetworks} networks do not divide into {C} chains")
        S = self.numNetworks // C
        picked = [c * S + s for c in range(C) for s in range(0, S, n)]
        if len(picked) // C < 8:
            raise ValueError(f"{len(picked) // C} draws per chain: the diagnostics need at least 8")
        return picked, C

    def predictDiagnostics(self, inputMatrix, n=1, transform=None, sd=1.0, mean=0.0):
        """Have the chains converged, and how many independent draws are the saved networks worth?  Split-R-hat and the effective sample
        size (Geyer's initial monotone sequence; the definition is in include/tbnn.h) of t = transform(f) * sd + mean per (output, row),
        over the numChains chains of fromChains (a plain predictor: one chain, split in two), reduced on the device.  Returns a dict:
        rhat, ess float64 [d_out, rows] (NaN where an element is constant or holds a NaN), max_rhat and min_ess over the defined
        elements, undefined: the number of NaN elements.  transform None resolves as in predictMoments; n thins WITHIN each chain (every
        n-th draw of each), which needs at least 8 draws left per chain."""
        transform = self._transform(transform)
        picked, C = self._chain_draws(n)
        ch = self._ensure_chain()
        rhat, ess = ch.ensemble_diagnostics(np.stack([self.vectors[i] for i in picked]), chains=C, X=np.asarray(inputMatrix, dtype=np.float32),
                                            xform=self._TRANSFORMS[transform], scale=float(sd), shift=float(mean))
        return self._diagnostics(rhat, ess)

    def parameterDiagnostics(self):
        """The dict of predictDiagnostics over the parameters themselves: every weight and bias coordinate in the order of the flattened
        networks, followed by the hypers where any were saved -- rhat, ess float64 [P + H]."""
        _picked, C = self._chain_draws()
        series = np.stack(self.vectors)
        if len(self.hypers):
            series = np.concatenate([series, np.stack([np.asarray(h, dtype=np.float32).reshape(-1) for h in self.hypers])], axis=1)
        return self._diagnostics(*self._ensure_chain().series_diagnostics(series, chains=C))

    def logPredictiveDensity(self, inputMatrix, realVals, n=1, weights=None, likelihood=None):
        """(per_network, per_row) under `likelihood` (None: the predictor's own): per_network[i] the summed log-likelihood of the rows
        under the i-th picked network (the data term of trainProbs / reweight, in fp64), per_row[r] the log of the weighted mixture of
        the networks' likelihoods of row r, whose sum is the log predictive density of held-out rows.  Under a GaussianLikelihood the
        standard deviation of each network is its saved last hyper, read as _data_logprob reads it."""
        lik = self.likelihood if likelihood is None else likelihood
        picked, w = self._picked(n, weights)
        sd = self._network_sd(lik, n)
        ch = self._ensure_chain()
        return ch.ensemble_loglik(picked, Y=np.asarray(realVals, dtype=np.float32), X=np.asarray(inputMatrix, dtype=np.float32),
                                  likelihood=lik.kind, sd=sd, weights=w)

    # ---- out-of-sample model comparison on the device: PSIS-LOO and WAIC (tbnn_ensemble_loo) ----
    def _loo_rows(self, inputMatrix, realVals, n, likelihood, r_eff, pointwise, psis=True):
        lik = self.likelihood if likelihood is None else likelihood
        picked, _w = self._picked(n, None)
        ch = self._ensure_chain()
        return ch.ensemble_loo(picked, Y=np.asarray(realVals, dtype=np.float32), X=np.asarray(inputMatrix, dtype=np.float32),
                               likelihood=lik.kind, sd=self._network_sd(lik, n), r_eff=float(r_eff), pointwise=pointwise, psis=psis), picked.shape[0]

    @staticmethod
    def _elpd_summary(name, ic, rows, lppd):
        """the sum of the rows, its standard error sqrt(n var(rows, ddof=1)) and the effective number of parameters sum(lppd - rows)"""
        rows = np.asarray(rows, dtype=np.float64)
        total = float(rows.sum())
        se = float(np.sqrt(rows.size * np.var(rows, ddof=1))) if rows.size > 1 else float("nan")
        return {"elpd_" + name: total, "se": se, "p_" + name: float(np.sum(lppd - rows)), ic: -2.0 * total}

    def loo(self, inputMatrix, realVals, n=1, likelihood=None, r_eff=1.0, pointwise=False):
        """Which model predicts better out of sample?  Pareto-smoothed importance-sampling leave-one-out cross-validation of every n-th
        network over the rows (Vehtari, Gelman, Gabry 2017; the R package loo's algorithm, stated in include/tbnn.h), formed and smoothed
        on the device.  Returns a dict: elpd_loo (the sum over the rows), se = sqrt(rows var(elpd_loo_rows, ddof=1)),
        p_loo = sum(lppd_rows - elpd_loo_rows), looic = -2 elpd_loo; the row arrays elpd_loo_rows, lppd_rows and pareto_k (float64 [rows];
        +inf where a row's ratios were not smoothed), k_threshold = min(1 - 1 / log10(m), 0.7) and n_bad_k, the number of rows above it,
        where the estimate cannot be trusted; with pointwise=True also pointwise, float64 [m, rows]: the log-likelihood matrix (ArviZ's
        log_likelihood group).  likelihood None: the predictor's own; under a GaussianLikelihood each network's standard deviation is its
        saved last hyper, as in logPredictiveDensity.  r_eff: the relative efficiency of the draws (1: independent; predictDiagnostics'
        ess over the number of draws is an estimate).  compareLoo compares two results over the same rows."""
        res, m = self._loo_rows(inputMatrix, realVals, n, likelihood, r_eff, pointwise)
        out = self._elpd_summary("loo", "looic", res["elpd_loo"], res["lppd"])
        thr = min(1.0 - 1.0 / np.log10(m), 0.7)
        k = res["pareto_k"]
        out.update(elpd_loo_rows=res["elpd_loo"], lppd_rows=res["lppd"], pareto_k=k, k_threshold=float(thr), n_bad_k=int(np.sum(k > thr)))
        if pointwise:
            out["pointwise"] = res["pointwise"]
        return out

    def waic(self, inputMatrix, realVals, n=1, likelihood=None, pointwise=False):
        """The widely applicable information criterion over the same matrix: elpd_waic (the sum over the rows of lppd - p_waic), se, p_waic
        (the sum of the rows' centred variances of the log-likelihood over the networks), waic = -2 elpd_waic, and the row arrays
        elpd_waic_rows, lppd_rows, p_waic_rows; with pointwise=True also the matrix.  Arguments as loo's."""
        res, _m = self._loo_rows(inputMatrix, realVals, n, likelihood, 1.0, pointwise, psis=False)      # (the smoothing kernel is not launched)
        rows = res["lppd"] - res["p_waic"]
        out = self._elpd_summary("waic", "waic", rows, res["lppd"])
        out.update(elpd_waic_rows=rows, lppd_rows=res["lppd"], p_waic_rows=res["p_waic"])
        if pointwise:
            out["pointwise"] = res["pointwise"]
        return out

    @staticmethod
    def compareLoo(a, b):
        """Two results of loo (or of waic) over the SAME rows, possibly of two predictors: elpd_diff = elpd(a) - elpd(b), the sum of the
        rows' differences, and se_diff = sqrt(rows var(a_rows - b_rows, ddof=1)), the paired standard error.  Host only."""
        def rows(r):
            for key in ("elpd_loo_rows", "elpd_waic_rows"):
                if key in r:
                    return np.asarray(r[key], dtype=np.float64).reshape(-1)
            raise ValueError("compareLoo takes the dicts loo or waic return")
        ra, rb = rows(a), rows(b)
        if ra.size != rb.size:
            raise ValueError(f"the results cover {ra.size} and {rb.size} rows: a comparison needs the same rows")
        d = ra - rb
        return {"elpd_diff": float(d.sum()), "se_diff": float(np.sqrt(d.size * np.var(d, ddof=1))) if d.size > 1 else float("nan")}

    def _network_sd(self, lik, n):
        """the standard deviation of every n-th network under a Gaussian kind of likelihood, float32 [picked]: the fixed sd, or each
        network's saved last hyper (0.1 where none was saved), read as _data_logprob reads it; the scale of a StudentTLikelihood; None
        for the other likelihoods"""
        from .likelihood import FixedGaussianLikelihood, GammaLikelihood, NegativeBinomialLikelihood, StudentTLikelihood, WeibullLikelihood
        picked = len(range(0, self.numNetworks, n))
        if isinstance(lik, (GammaLikelihood, WeibullLikelihood)):
            # no scale; its shape set on the forward chain (a fixed-sd Gaussian handle) before the reduction that judges under it
            self._ensure_chain().set_lik_df(lik.shape)
            return None
        if isinstance(lik, NegativeBinomialLikelihood):
            # no scale; its dispersion set on the forward chain (a fixed-sd Gaussian handle) before the reduction that judges under it
            self._ensure_chain().set_lik_df(lik.dispersion)
            return None
        if isinstance(lik, StudentTLikelihood):
            # its scale, one per network as the fixed sd -- and its degrees of freedom set on the forward chain (a fixed-sd Gaussian handle)
            # before the reduction that judges under it
            self._ensure_chain().set_lik_df(lik.df)
            return np.full(picked, np.float32(lik.sd), dtype=np.float32)
        if isinstance(lik, FixedGaussianLikelihood):
            return np.full(picked, np.float32(lik.sd), dtype=np.float32)                        # likelihood.py:195 (not squared)
        if isinstance(lik, GaussianLikelihood):
            return np.array([np.float32(self.hypers[m][-1]) if len(self.hypers) else np.float32(0.1)
                             for m in range(0, self.numNetworks, n)], dtype=np.float32)         # likelihood.py:116-117
        return None

    # ---- the predictive distribution of a new observation: observation noise included (tbnn_ensemble_predictive) ----
    def _predictive_likelihood(self, likelihood):
        from .likelihood import BernoulliLikelihood, CategoricalLikelihood, StudentTLikelihood
        lik = self.likelihood if likelihood is None else likelihood
        if isinstance(lik, (BernoulliLikelihood, CategoricalLikelihood)):
            raise ValueError("the predictive distribution of a label is its posterior-mean probability: predictMoments returns it")
        if isinstance(lik, StudentTLikelihood):
            raise ValueError("predictive quantiles, intervals and the predictive CDF are not built for a StudentTLikelihood (the mixture of t "
                             "CDFs needs the incomplete beta function on the device); logPredictiveDensity, loo and waic are")
        return lik

    def predictiveQuantiles(self, inputMatrix, probs, n=1, weights=None, likelihood=None, sd=1.0, mean=0.0):
        """Quantiles of the PREDICTIVE distribution of a new observation at the probabilities `probs` (each in (0, 1)), float64
        [n_probs, d_out, rows] (a scalar `probs`: [d_out, rows]): the mixture over every n-th network of the observation model around
        its prediction, inverted on the device -- under a Gaussian kind of likelihood N(f_i, s_i^2) with s_i the network's own standard
        deviation (its saved last hyper as logPredictiveDensity reads it, or the fixed sd), under a PoissonLikelihood the counts'
        Poisson(exp(f_i)) and under a NegativeBinomialLikelihood their negative binomial of mean exp(f_i) and the likelihood's
        dispersion, whose quantile is the smallest count k with F(k) >= p; under a GammaLikelihood the Gamma of mean exp(f_i) and
        the likelihood's shape, a continuous distribution on y > 0 inverted as the Gaussian mixture is, and under a WeibullLikelihood the
        Weibull of scale exp(f_i) and the likelihood's shape, the distribution of the time to the event, by the same search.  likelihood None: the predictor's own.  weights: one
        per picked network, e.g. what reweight returns.  The result is q * sd + mean, the de-normalisation of the metrics, applied on
        the host in fp64: sd > 0, and counts, Gamma targets and Weibull times take none (sd = 1, mean = 0).  predictQuantiles gives the credible quantiles of the
        network's output instead; Bernoulli and categorical likelihoods are refused (predictMoments returns a label's probability)."""
        from .likelihood import GammaLikelihood, NegativeBinomialLikelihood, PoissonLikelihood, WeibullLikelihood
        lik = self._predictive_likelihood(likelihood)
        sd, mean = float(sd), float(mean)
        if not sd > 0.0:
            raise ValueError("sd must be > 0 (a negative scale would turn the quantiles round)")
        if isinstance(lik, GammaLikelihood) and (sd != 1.0 or mean != 0.0):
            raise ValueError("Gamma targets are not de-normalised: sd = 1, mean = 0 under a GammaLikelihood")
        if isinstance(lik, WeibullLikelihood) and (sd != 1.0 or mean != 0.0):
            raise ValueError("Weibull times are not de-normalised: sd = 1, mean = 0 under a WeibullLikelihood")
        if isinstance(lik, (PoissonLikelihood, NegativeBinomialLikelihood)) and (sd != 1.0 or mean != 0.0):
            raise ValueError("counts are not de-normalised: sd = 1, mean = 0 under a PoissonLikelihood or NegativeBinomialLikelihood")
        picked, w = self._picked(n, weights)
        pr = np.asarray(probs, dtype=np.float64)
        ch = self._ensure_chain()
        q, _F, _Fb = ch.ensemble_predictive(picked, probs=pr.reshape(-1), X=np.asarray(inputMatrix, dtype=np.float32), likelihood=lik.kind,
                                            sd=self._network_sd(lik, n), weights=w)
        if sd != 1.0 or mean != 0.0:
            q = q * sd + mean
        return q[0] if pr.ndim == 0 else q

    def predictiveInterval(self, inputMatrix, level=0.9, **kwargs):
        """(lower, median, upper), each float64 [d_out, rows]: the predictive quantiles at (1 - level) / 2, 1 / 2 and (1 + level) / 2 from
        one call of predictiveQuantiles, whose other arguments pass through -- the central PREDICTIVE interval, which a new observation
        falls into with probability `level` (predictInterval's credible interval covers the network's output only)."""
        q = self.predictiveQuantiles(inputMatrix, self._central_probs(level), **kwargs)
        return q[0], q[1], q[2]

    def predictiveCDF(self, inputMatrix, realVals, n=1, weights=None, likelihood=None):
        """The PIT values of the rows: the predictive CDF of predictiveQuantiles at the observed targets realVals, float64 [d_out, rows]
        -- uniform on (0, 1) over held-out rows when the predictive distribution is calibrated.  Targets in the networks' own
        (normalised) units.  Under a PoissonLikelihood or NegativeBinomialLikelihood the pair (F(y - 1), F(y)): a count's PIT value lies
        anywhere on its step.  Under a GammaLikelihood F alone, as under the Gaussian kinds: the CDF is continuous.  Under a WeibullLikelihood F alone
        too, read at |y|: the sign of a target is its censoring flag, and on a censored row the PIT value lies in [F, 1]."""
        from .likelihood import NegativeBinomialLikelihood, PoissonLikelihood
        lik = self._predictive_likelihood(likelihood)
        picked, w = self._picked(n, weights)
        ch = self._ensure_chain()
        _q, F, Fb = ch.ensemble_predictive(picked, Y=np.asarray(realVals, dtype=np.float32), X=np.asarray(inputMatrix, dtype=np.float32),
                                           likelihood=lik.kind, sd=self._network_sd(lik, n), weights=w)
        return (Fb, F) if isinstance(lik, (PoissonLikelihood, NegativeBinomialLikelihood)) else F

    def survival(self, X, times, n=1, weights=None, likelihood=None):
        """The posterior-mean survival curve of every row of X under a WeibullLikelihood: S(t) = 1 - F(t), the probability that the event
        has not happened by time t, float64 [len(times), d_out, rows].  times: finite and > 0.  n, weights, likelihood: as
        predictiveCDF's.  (A host loop of predictiveCDF over the times, one device reduction per time: there is no time grid on the
        device.)"""
        from .likelihood import WeibullLikelihood
        lik = self.likelihood if likelihood is None else likelihood
        if not isinstance(lik, WeibullLikelihood):
            raise ValueError("survival needs a WeibullLikelihood: the survival curve is that of a time to an event")
        ts = np.asarray(times, dtype=np.float64).reshape(-1)
        if ts.size < 1 or not (np.all(np.isfinite(ts)) and np.all(ts > 0)):
            raise ValueError("survival: times must be finite and > 0, at least one")
        x = np.asarray(X, dtype=np.float32)
        rows = x.shape[0]
        d_out = self._ensure_chain().d_out
        out = []
        for t in ts:                                                   # the host loop: one predictiveCDF per time
            y = np.full((rows, d_out), np.float32(t), dtype=np.float32)
            out.append(1.0 - self.predictiveCDF(x, y, n=n, weights=weights, likelihood=lik))
        return np.stack(out, axis=0)

    # ---- the continuous ranked probability score of the predictive mixture (tbnn_ensemble_crps) ----
    def _crps_likelihood(self, likelihood):
        from .likelihood import (BernoulliLikelihood, CategoricalLikelihood, GammaLikelihood, NegativeBinomialLikelihood,
                                 PoissonLikelihood, StudentTLikelihood, WeibullLikelihood)
        lik = self.likelihood if likelihood is None else likelihood
        if isinstance(lik, WeibullLikelihood):
            raise ValueError("the CRPS is not built for a WeibullLikelihood (no kernel forms the pair term of two Weibull distributions, and a "
                             "censored row has no observed value to score); logPredictiveDensity, loo, waic, predictiveInterval, "
                             "predictiveCDF and survival are")
        if isinstance(lik, GammaLikelihood):
            raise ValueError("the CRPS is not built for a GammaLikelihood (the pair term of two Gamma distributions has no closed form); "
                             "logPredictiveDensity, loo, waic, predictiveInterval and predictiveCDF are")
        if isinstance(lik, (BernoulliLikelihood, CategoricalLikelihood)):
            raise ValueError("the CRPS is a score of a real-valued prediction: predictUncertainty and calibration judge a label")
        if isinstance(lik, (PoissonLikelihood, NegativeBinomialLikelihood)):
            raise ValueError("the CRPS is not built for a PoissonLikelihood or NegativeBinomialLikelihood (the pair term of two count "
                             "distributions has no closed form); logPredictiveDensity, loo, waic and predictiveCDF are")
        if isinstance(lik, StudentTLikelihood):
            raise ValueError("the CRPS is not built for a StudentTLikelihood (the pair term of two t distributions has no closed form); "
                             "logPredictiveDensity, loo and waic are")
        return lik

    def crps(self, inputMatrix, realVals, n=1, weights=None, likelihood=None, noise=True):
        """The continuous ranked probability score of the rows: a proper score in the units of the target that rewards calibration and
        sharpness together, bounded where the log score is not.  The predictive distribution is predictiveQuantiles' -- the mixture over
        every n-th network of N(f_i, s_i^2), s_i the network's own standard deviation (its saved last hyper as logPredictiveDensity reads
        it, or the fixed sd; exp of the log-sd output under a HeteroscedasticGaussianLikelihood) -- and the score its closed form over
        all pairs of networks, on the device (the definition is in include/tbnn.h).  Targets in the networks' own (normalised) units, as
        predictiveCDF's.  noise=False: the ensemble CRPS of the networks' outputs alone.  Returns a dict: crps, error = E|Y - y| and
        spread = 1/2 E|Y - Y'| (crps = error - spread), float64 [d_out, rows]; mean_crps [d_out], the mean over the rows that are not
        NaN; se [d_out] = sqrt(var(rows, ddof=1) / rows) over the same rows; n_bad, the number of NaN elements.  compareCrps compares
        two results over the same rows.  weights: one per picked network, e.g. what reweight returns."""
        lik = self._crps_likelihood(likelihood)
        picked, w = self._picked(n, weights)
        ch = self._ensure_chain()
        res = ch.ensemble_crps(picked, Y=np.asarray(realVals, dtype=np.float32), X=np.asarray(inputMatrix, dtype=np.float32),
                               likelihood=lik.kind, sd=self._network_sd(lik, n) if noise else None, weights=w, noise=bool(noise))
        res.update(self._crps_summary(res["crps"]))
        return res

    @staticmethod
    def _crps_summary(rows):
        """mean_crps and se per output over the rows that are not NaN, and the count of NaN elements"""
        rows = np.asarray(rows, dtype=np.float64)
        ok = ~np.isnan(rows)
        mean, se = np.full(rows.shape[0], np.nan), np.full(rows.shape[0], np.nan)
        for k in range(rows.shape[0]):
            v = rows[k][ok[k]]
            if v.size:
                mean[k] = v.mean()
            if v.size > 1:
                se[k] = np.sqrt(np.var(v, ddof=1) / v.size)
        return {"mean_crps": mean, "se": se, "n_bad": int((~ok).sum())}

    @staticmethod
    def compareCrps(a, b):
        """Two results of crps over the SAME rows, possibly of two predictors: crps_diff, the mean over the rows of crps(a) - crps(b)
        (negative: a is better), and se_diff = sqrt(var(a_rows - b_rows, ddof=1) / rows), the paired standard error; each per output.
        Rows that are NaN in either result are left out.  Host only."""
        def rows(r):
            if not isinstance(r, dict) or "crps" not in r:
                raise ValueError("compareCrps takes the dicts crps returns")
            v = np.asarray(r["crps"], dtype=np.float64)
            return v.reshape(1, -1) if v.ndim < 2 else v
        ra, rb = rows(a), rows(b)
        if ra.shape != rb.shape:
            raise ValueError(f"the results cover {ra.shape[-1]} and {rb.shape[-1]} rows of {ra.shape[0]} and {rb.shape[0]} outputs: a "
                             "comparison needs the same rows")
        d = ra - rb
        diff, se = np.full(d.shape[0], np.nan), np.full(d.shape[0], np.nan)
        for k in range(d.shape[0]):
            v = d[k][~np.isnan(d[k])]
            if v.size:
                diff[k] = v.mean()
            if v.size > 1:
                se[k] = np.sqrt(np.var(v, ddof=1) / v.size)
        return {"crps_diff": diff, "se_diff": se}

    # ---- classification: entropy split, votes (tbnn_ensemble_uncertainty) and calibration of the posterior-mean classifier ----
    def _label_likelihood(self, likelihood):
        from .likelihood import BernoulliLikelihood, CategoricalLikelihood, GammaLikelihood, WeibullLikelihood
        lik = self.likelihood if likelihood is None else likelihood
        if isinstance(lik, WeibullLikelihood):
            raise ValueError("the entropy split and the votes are those of a label, not of a WeibullLikelihood's time to an event: "
                             "predictMoments(noiseVariance=True) separates the Weibull noise from the posterior spread of the scale, and "
                             "predictiveInterval / predictiveCDF / survival describe the time")
        if isinstance(lik, GammaLikelihood):
            raise ValueError("the entropy split and the votes are those of a label, not of a GammaLikelihood's positive target: "
                             "predictMoments(noiseVariance=True) separates the Gamma noise from the posterior spread of the mean, and "
                             "predictiveInterval / predictiveCDF check the intervals")
        if not isinstance(lik, (BernoulliLikelihood, CategoricalLikelihood)):
            raise ValueError("the entropy split, the votes and the calibration table are those of a label: a BernoulliLikelihood or a "
                             "CategoricalLikelihood; for a regression predictMoments(noiseVariance=True) separates the noise from the "
                             "posterior spread and predictiveInterval / predictiveCDF check the intervals")
        return lik

    def predictUncertainty(self, inputMatrix, n=1, weights=None, likelihood=None):
        """How sure is the ensemble of a label, and why?  Over every n-th network, reduced on the device (the definition is in
        include/tbnn.h, tbnn_ensemble_uncertainty), a dict of float64 arrays: probs [d_out, rows], the posterior-mean probability of each
        class (BernoulliLikelihood: of the label 1 of each output); votes [d_out, rows], the share of the posterior whose own arg-max is that
        class (Bernoulli: whose p >= 1/2); total, the entropy of probs; aleatoric, the posterior mean of each network's own entropy (noise
        in the data); epistemic = total - aleatoric >= 0, the mutual information between label and network ("BALD": what the networks
        disagree about); variation_ratio = 1 - max_k votes_k (Bernoulli: 1 - max(vote, 1 - vote)).  The entropies and the variation ratio
        are [rows] under a CategoricalLikelihood and [d_out, rows] under a BernoulliLikelihood, natural logarithms.  likelihood None: the
        predictor's own; a regression or count likelihood is refused.  weights: one per picked network, e.g. what reweight returns."""
        from .likelihood import CategoricalLikelihood
        lik = self._label_likelihood(likelihood)
        picked, w = self._picked(n, weights)
        ch = self._ensure_chain()
        out = ch.ensemble_uncertainty(picked, X=np.asarray(inputMatrix, dtype=np.float32), weights=w, likelihood=lik.kind)
        v = out["votes"]
        out["variation_ratio"] = 1.0 - (v.max(axis=0) if isinstance(lik, CategoricalLikelihood) else np.maximum(v, 1.0 - v))
        return out

    @staticmethod
    def _check_bins(bins):
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= int(bins) <= 1000:
            raise ValueError("bins must be an integer in 1 .. 1000")
        return int(bins)

    @staticmethod
    def _calibration_table(probs, Y, bins, kind):
        """The reliability table of a classifier that predicts the probabilities probs, float64 [d_out, rows], against the labels Y; kind
        "categorical" (the columns of probs are class probabilities; Y one-hot or probability rows [rows, K], label = the first arg-max, or
        an integer vector [rows]) or "bernoulli" (every output a label of its own, the entry the probability of 1, clipped to
        [1e-8, 1 - 1e-7] first; Y [rows, d_out] or [rows] of 0 / 1, label = y >= 1/2).  Host only, NumPy; see calibration for the result."""
        bins = predictor._check_bins(bins)
        if kind not in ("categorical", "bernoulli"):
            raise ValueError("kind must be 'categorical' or 'bernoulli'")
        p = np.asarray(probs, dtype=np.float64)
        if p.ndim != 2:
            raise ValueError("probs must be [d_out, rows]")
        K, rows = p.shape
        y = np.asarray(Y)
        if kind == "categorical":
            if y.ndim == 1:
                if y.size != rows:
                    raise ValueError(f"Y must hold {rows} labels")
                label = y.astype(np.int64)
                if np.any(label != y) or np.any(label < 0) or np.any(label >= K):
                    raise ValueError(f"integer labels must lie in 0 .. {K - 1}")
            else:
                if y.shape != (rows, K):
                    raise ValueError(f"Y must be [{rows}, {K}] or an integer vector [{rows}]")
                label = np.argmax(y, axis=1)
            predicted = np.argmax(p, axis=0)                                    # (the first of equal maxima: ties to the lowest class)
            confidence = p[predicted, np.arange(rows)]
            correct = predicted == label
            with np.errstate(divide="ignore"):
                nll = float(np.mean(-np.log(p[label, np.arange(rows)])))
            onehot = np.zeros((K, rows))
            onehot[label, np.arange(rows)] = 1.0
            brier = float(np.mean(np.sum((p - onehot) ** 2, axis=0)))
        else:
            y = y.reshape(rows, K) if y.size == rows * K else None
            if y is None:
                raise ValueError(f"Y must be [{rows}, {K}]")
            label = (y.T >= 0.5)
            p = np.clip(p, np.float64(np.float32(1e-8)), np.float64(np.float32(1.0) - np.float32(1e-7)))
            predicted = p >= 0.5
            confidence = np.maximum(p, 1.0 - p)
            correct = predicted == label
            nll = float(np.mean(-np.where(label, np.log(p), np.log1p(-p))))
            brier = float(np.mean((p - label) ** 2))
            predicted = predicted.astype(np.int64)
        edges = np.linspace(0.0, 1.0, bins + 1)
        # right-closed bins (e_{b-1}, e_b], 0 in the first
        idx = np.clip(np.searchsorted(edges, confidence, side="left") - 1, 0, bins - 1)
        count = np.bincount(idx.reshape(-1), minlength=bins)
        with np.errstate(invalid="ignore", divide="ignore"):
            conf_b = np.bincount(idx.reshape(-1), weights=confidence.reshape(-1), minlength=bins) / count
            acc_b = np.bincount(idx.reshape(-1), weights=correct.reshape(-1).astype(np.float64), minlength=bins) / count
        conf_b[count == 0] = np.nan
        acc_b[count == 0] = np.nan
        gap = np.abs(acc_b - conf_b)
        full = count > 0
        return {"accuracy": float(np.mean(correct)), "nll": nll, "brier": brier,
                "ece": float(np.sum(count[full] / confidence.size * gap[full])), "mce": float(np.max(gap[full])),
                "bins": {"edges": edges, "count": count, "confidence": conf_b, "accuracy": acc_b},
                "predicted": predicted, "confidence": confidence, "correct": correct}

    def calibration(self, inputMatrix, realVals, bins=10, n=1, weights=None, likelihood=None):
        """Is the ensemble's sureness honest?  The reliability table of the posterior-mean classifier (predictUncertainty's probs) against
        held-out labels -- the classification counterpart of predictiveCDF's PIT values.  The probabilities come from the device; the table
        is d_out x rows doubles of NumPy on the host.  Labels: CategoricalLikelihood one-hot or probability rows [rows, K] (label = the
        first arg-max) or an integer vector [rows]; BernoulliLikelihood [rows, d_out] or [rows] of 0 / 1 (label = y >= 1/2).  Returns a
        dict: accuracy; nll, the mean of -log pbar_label (Bernoulli: from pbar clipped to [1e-8, 1 - 1e-7]); brier, the mean over the rows
        of sum_k (pbar_k - y_k)^2 (Bernoulli: the mean over the elements of the square); ece = sum_b n_b / n |acc_b - conf_b| and
        mce = max_b |acc_b - conf_b| over the non-empty bins; bins: edges, count, confidence, accuracy -- `bins` (1 .. 1000) equal-width
        bins over [0, 1], right-closed, 0 in the first, an empty bin with count 0 and NaN means; and the row arrays predicted (arg-max,
        ties to the lowest class; Bernoulli pbar >= 1/2), confidence (max_k pbar_k; Bernoulli max(pbar, 1 - pbar)) and correct."""
        from .likelihood import CategoricalLikelihood
        lik = self._label_likelihood(likelihood)
        bins = self._check_bins(bins)                                                     # (before the device is asked for anything)
        picked, w = self._picked(n, weights)
        ch = self._ensure_chain()
        probs = ch.ensemble_uncertainty(picked, X=np.asarray(inputMatrix, dtype=np.float32), weights=w, likelihood=lik.kind)["probs"]
        return self._calibration_table(probs, realVals, bins, "categorical" if isinstance(lik, CategoricalLikelihood) else "bernoulli")

    def _ensure_chain(self):
        if self._chain is None:
            self._chain = nat.Chain(self._descriptor(), likelihood=nat.LIK_FIXED_GAUSSIAN, fixed_sd=1.0,
                                    device=self.device)
            print("tensorbnn_amd: forward kernel", self._chain.kernel_name)    # once; Chain warns when it is the generic one
        return self._chain

    def _hyper_probs(self, weights, n):
        """predictor.py:188-206 / :248-266: minus the data term, minus every layer's calculateHyperProbs.  With the built-in
        dense layers the sum over layers of calculateHyperProbs of EVERY picked network is one launch of the native library
        (tbnn_hyper_probs_many, one workgroup per network, the priors of the architecture loaded right now); layers from
        customLayerDict keep their own Python calculateHyperProbs."""
        picked = list(range(0, self.numNetworks, n))
        dense = [l for l in self.layers if l.numTensors > 0]
        if picked and len(self.hypers) and all(type(l) in (CauchyDenseLayer, GaussianDenseLayer) for l in dense) and \
                all(l.numHyperTensors == 0 for l in self.layers if l.numTensors == 0):
            ch = self._ensure_chain()
            thetas = np.stack([self.vectors[m] for m in picked])
            etas = np.stack([np.asarray(self.hypers[m], dtype=np.float32).reshape(-1)[:4 * len(dense)] for m in picked])
            hp = ch.hyper_probs_many(thetas, etas, priors=[l.prior_kind for l in dense])
            return np.array([np.float32(-np.float32(w) - np.float32(v)) for w, v in zip(weights, hp)])
        for m in picked:
            matrixIndex = hyperIndex = 0
            current = -weights[m // n]
            for layer in self.layers:
                tensors = [self.matrices[matrixIndex + x][m, :, :] for x in range(layer.numTensors)]
                hypers = [self.hypers[m][hyperIndex + x] for x in range(layer.numHyperTensors)]
                hyperIndex += layer.numHyperTensors
                matrixIndex += layer.numTensors
                if layer.numHyperTensors > 0:
                    current = current - np.float32(layer.calculateHyperProbs(hypers, tensors))
            weights[m // n] = current
        return np.array(weights)

    def trainProbs(self, trainX, trainY, n, likelihood):
        """predictor.py:157-207: negative log posterior weight of every n-th network under the training priors"""
        if likelihood is not None:
            weights = self._data_logprob(self.likelihood, trainX, trainY, n)
        else:
            weights = [np.float32(0) for _ in range(0, self.numNetworks, n)]
        self.weightsTrain = self._hyper_probs(weights, n)

    def reweight(self, architecture, trainX=None, trainY=None, n=1, likelihood=None):
        """predictor.py:209-273: importance weights p(theta | new priors) / p(theta | training priors), normalised"""
        if len(self.weightsTrain) == 0:
            self.trainProbs(trainX, trainY, n, likelihood)
        self.loadArchitecture(architecture=architecture)
        if likelihood is not None:
            weights = self._data_logprob(likelihood, trainX, trainY, n)
        else:
            weights = [np.float32(0) for _ in range(0, self.numNetworks, n)]
        self.weights = self._hyper_probs(weights, n)
        weighting = np.exp(self.weightsTrain - self.weights)
        weighting = weighting / np.sum(weighting)
        self.loadArchitecture()
        return weighting

    # ---- autocorrelation (predictor.py:275-312) ----
    def autocorrelation(self, inputData, nMax):
        output = np.squeeze(np.array(self.predict(inputData, n=1))).T
        valFunc, accepted = 0, 0
        for x in range(len(output)):
            temp = integrated_time(output[x], tol=5, quiet=True)
            if not np.isnan(temp).any():
                valFunc = valFunc + np.array(function_1d(output[x]))
                accepted += 1
        valFunc = valFunc / accepted
        return valFunc[:nMax] if nMax < len(valFunc) else valFunc

    def autoCorrelationLength(self, inputData, nMax):
        output = np.squeeze(np.array(self.predict(inputData, n=1))).T
        val, accepted = 0, 0
        for x in range(len(output)):
            temp = integrated_time(output[x], tol=5, quiet=True)
            if not np.isnan(temp).any():
                val = val + temp
                accepted += 1
        val = val / accepted
        if val[0] > nMax:
            print("Correlation time is greater than maximum accepted value.")
        return val[0]

    def extractParameters(self):
        """predictor.py:314-319: the parameter matrices, first axis = network"""
        return self.matrices

    def extractHyperParameters(self):
        """predictor.py:321-326: the hyper parameters, first axis = network"""
        return np.array(self.hypers)

    def parameterStatistics(self):
        """predictor.py:328-339: per parameter matrix, its mean and its standard deviation over the networks"""
        return [np.mean(m, axis=0) for m in self.matrices], [np.std(m, axis=0) for m in self.matrices]

    def hyperStatistics(self):
        """predictor.py:341-351: mean and standard deviation of every hyper parameter over the networks"""
        hypers = np.array(self.hypers)
        return np.mean(hypers, axis=0), np.std(hypers, axis=0)



def function_1d(x):
    """emcee.autocorr.function_1d: normalised autocorrelation function of a 1-D series (FFT, zero-padded)"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    if x.ndim != 1:
        raise ValueError("invalid dimensions for 1D autocorrelation function")
    n = 1
    while n < len(x):
        n <<= 1
    f = np.fft.fft(x - np.mean(x), n=2 * n)
    acf = np.fft.ifft(f * np.conjugate(f))[: len(x)].real
    acf /= acf[0]
    return acf


def integrated_time(x, c=5, tol=50, quiet=False):
    """emcee.autocorr.integrated_time for one chain: tau = 2 * cumsum(acf) - 1 at Sokal's window (first M >= c * tau);
    returns an array of one element, NaN-free unless the series is constant"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    f = function_1d(x)
    taus = 2.0 * np.cumsum(f) - 1.0
    m = np.arange(len(taus)) < c * taus
    window = int(np.argmin(m)) if np.any(m) else len(taus) - 1
    tau_est = np.array([taus[window]])
    if not quiet and np.any(tol * tau_est > len(x)):
        raise ValueError("The chain is shorter than {0} times the integrated autocorrelation time".format(tol))
    return tau_est
