"""What the GPU test modules share when they put a spec of the oracle (oracle/tbnn_oracle.py) before the library and judge a gradient against it:
the layer tuples native.Chain takes, the slices of theta that hold one tensor (W_l or b_l) each, and the error of a gradient per tensor.  A
gradient is judged tensor by tensor because the early layers of a network have small gradients: against theta's inf-norm their errors would
vanish.  Every caller brings its own floor (1e-3 where a tensor's gradient may be all but zero, 1e-30 where it may not) and its own band."""
import numpy as np


def layers_of(spec):
    return [(l.in_dim, l.out_dim, l.act, l.prior) for l in spec.layers]


def tensors(spec):
    """(start, stop) of W_0, b_0, W_1, b_1, ... within theta"""
    for l, (ow, ob) in zip(spec.layers, spec.offsets()):
        yield ow, ob
        yield ob, ob + l.out_dim


def tensor_errs(spec, g, gref, floor):
    """per tensor: the largest error of g against gref, over max(that tensor's inf-norm in gref, floor)"""
    g = np.asarray(g, np.float64)
    return [float(np.abs(g[a:b] - gref[a:b]).max() / max(np.abs(gref[a:b]).max(), floor)) for a, b in tensors(spec)]


def tensor_err(spec, g, gref, floor):
    """the worst of tensor_errs"""
    return max(tensor_errs(spec, g, gref, floor))
