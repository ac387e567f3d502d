"""tensorbnn_amd -- MI355X-native HMC sampler for dense Bayesian neural networks.

Drop-in for the HMC hot path of alpha-davidson/TensorBNN: the same
``network.add() / setupMCMC() / train()`` API and Layer / Likelihood plug-in
surface, with the transition running in hand-written gfx950 HIP kernels behind
the C ABI of ``include/tbnn.h`` (bound in ``_native.py``).  No CPU fallback.
"""
__version__ = "0.1.0"

# the reference's pre-training helpers (they load the native library on their first call, not here: `tensorbnn_amd.build` must import without it)
from .BNN_functions import trainBasicClassification, trainBasicRegression  # noqa: E402,F401


def __getattr__(name):
    # the likelihood plug-ins bind the native library when their module is imported: resolved on first use, for the same reason
    if name == "StudentTLikelihood":
        from .likelihood import StudentTLikelihood
        return StudentTLikelihood
    if name == "NegativeBinomialLikelihood":
        from .likelihood import NegativeBinomialLikelihood
        return NegativeBinomialLikelihood
    if name == "HeteroscedasticGaussianLikelihood":
        from .likelihood import HeteroscedasticGaussianLikelihood
        return HeteroscedasticGaussianLikelihood
    if name == "GammaLikelihood":
        from .likelihood import GammaLikelihood
        return GammaLikelihood
    if name == "WeibullLikelihood":
        from .likelihood import WeibullLikelihood
        return WeibullLikelihood
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
