"""The pre-training helpers of the reference (tensorBNN/BNN_functions.py:60-297) with their positional signatures, on the device.

``trainBasicRegression`` / ``trainBasicClassification`` build a plain network of ``hidden`` layers of ``width`` units, train it with
AMSGrad in ``cycles`` cycles of falling learning rate and early stopping on the validation loss, and return ``(weights, biases,
activation)`` for the ``weights=`` / ``biases=`` arguments of the BNN's layers.  Both are thin wrappers over ``network.pretrain`` with
``objective="likelihood"``; the optimiser is ``tbnn_optimize`` (include/tbnn.h) on the fused HIP kernels.  There is no CPU fallback.

Departures from the reference:
  * the hidden activation is Relu, i.e. ``alpha`` must be 0: the HIP path has no leaky-ReLU kernel family, and any other ``alpha`` raises
    NotImplementedError.  ``activation`` is returned as ``[]``, which is what the reference's LeakyReLU layers yield (they hold no weights);
  * one epoch is ONE FULL-BATCH Adam step, not Keras' pass over mini-batches of 32 rows (n / 32 updates): expect to ask for more epochs;
  * the losses are the project's likelihoods: mean squared error becomes a FixedGaussianLikelihood of sd 1 (the same minimiser; Adam's step
    does not depend on the scale of the loss beyond epsilon), binary cross-entropy a BernoulliLikelihood behind a sigmoid last layer (its
    probabilities clipped to [1e-8, 1 - 1e-7] as everywhere in the project);
  * Adam's epsilon is 1e-8 (Keras: 1e-7), beta1 0.9, beta2 0.999;
  * early stopping judges every 10 steps (``network.pretrain``'s checkEvery), and ``patience`` counts those checks;
  * ``callbackMetric``: "val_loss" (the validation rows) or "loss" (the training objective);
  * the initial weights are Glorot-uniform from NumPy's PCG64(1000 + layer), biases zero: the same distribution as Keras' initialiser, not
    TensorFlow's stream;
  * ``name`` is written as a NumPy archive ``<name>.npz`` (weights0, biases0, weights1, ...), not a Keras model.
"""
import numpy as np


def _leaky_check(alpha):
    if float(alpha) != 0.0:
        raise NotImplementedError(f"alpha = {alpha}: the HIP path has no leaky-ReLU kernel family; pre-training runs with alpha = 0 (Relu hidden layers)")


def _glorot(layer, fan_in, fan_out):
    lim = (6.0 / (fan_in + fan_out)) ** 0.5
    return np.random.Generator(np.random.PCG64(1000 + layer)).uniform(-lim, lim, (fan_out, fan_in)).astype(np.float32)


def _train_basic(hidden, inputDims, outputDims, width, cycles, epochs, trainIn, trainOut, valIn, valOut, name, callbacks, callbackMetric,
                 patience, classify, learningRate):
    from .activationFunctions import Relu, Sigmoid
    from .layer import GaussianDenseLayer
    from .likelihood import BernoulliLikelihood, FixedGaussianLikelihood
    from .network import network
    if callbackMetric not in ("val_loss", "loss"):
        raise NotImplementedError(f'callbackMetric {callbackMetric!r}: "val_loss" or "loss"')
    trainIn = np.asarray(trainIn, dtype=np.float32).reshape(-1, inputDims)
    trainOut = np.asarray(trainOut, dtype=np.float32).reshape(len(trainIn), outputDims)
    if callbackMetric == "val_loss":
        valIn = np.asarray(valIn, dtype=np.float32).reshape(-1, inputDims)
        valOut = np.asarray(valOut, dtype=np.float32).reshape(len(valIn), outputDims)
    else:
        valIn, valOut = np.zeros((0, inputDims), np.float32), np.zeros((0, outputDims), np.float32)
    net = network(np.float32, inputDims, trainIn, trainOut, valIn, valOut)
    dims = [inputDims] + [width] * hidden + [outputDims]
    for i in range(len(dims) - 1):
        net.add(GaussianDenseLayer(dims[i], dims[i + 1], weights=_glorot(i, dims[i], dims[i + 1]), biases=np.zeros((dims[i + 1], 1), np.float32)))
        if i < len(dims) - 2:
            net.add(Relu())
        elif classify:
            net.add(Sigmoid())
    lik = BernoulliLikelihood() if classify else FixedGaussianLikelihood(sd=1.0)
    try:
        total = int(cycles) * int(epochs)
        net.pretrain(lik, cycles=cycles, epochs=epochs, learningRate=learningRate, decay=10.0, objective="likelihood",
                     patience=patience if callbacks else total + 1, verbose=False)
    finally:
        if net._chain is not None:
            net._chain.close()
    weights = [np.asarray(net.states[2 * i], dtype=np.float32) for i in range(len(dims) - 1)]
    biases = [np.asarray(net.states[2 * i + 1], dtype=np.float32).reshape(-1, 1) for i in range(len(dims) - 1)]
    if name is not None:
        arrays = {}
        for i, (w, b) in enumerate(zip(weights, biases)):
            arrays[f"weights{i}"], arrays[f"biases{i}"] = w, b
        np.savez(name, **arrays)
    return (weights, biases, [])


def trainBasicRegression(hidden, inputDims, outputDims, width, cycles, epochs, alpha, trainIn, trainOut, valIn, valOut, name,
                         callbacks=True, callbackMetric="val_loss", patience=10):
    """BNN_functions.py:60-180 on the device: a regression network of `hidden` Relu layers of `width` units trained on the squared error with
    AMSGrad at 0.01 * 10**-cycle.  Returns (weights, biases, activation): weights[i] [out, in], biases[i] [out, 1], activation [].  See the
    module docstring for the departures from the reference (alpha must be 0; one epoch is one full-batch step; `name` is an .npz file)."""
    _leaky_check(alpha)
    return _train_basic(hidden, inputDims, outputDims, width, cycles, epochs, trainIn, trainOut, valIn, valOut, name, callbacks,
                        callbackMetric, patience, False, 0.01)


def trainBasicClassification(hidden, inputDims, outputDims, width, cycles, epochs, alpha, trainIn, trainOut, valIn, valOut, name,
                             callbacks=True, callbackMetric="val_loss", patience=10):
    """BNN_functions.py:183-298 on the device: a binary classifier of `hidden` Relu layers of `width` units and a sigmoid last layer trained on
    the cross-entropy with AMSGrad at 0.001 * 10**-cycle.  Returns (weights, biases, activation) as trainBasicRegression does; the same
    departures apply (alpha must be 0; one epoch is one full-batch step; `name` is an .npz file)."""
    _leaky_check(alpha)
    return _train_basic(hidden, inputDims, outputDims, width, cycles, epochs, trainIn, trainOut, valIn, valOut, name, callbacks,
                        callbackMetric, patience, True, 0.001)
