"""The fp64 restatement of tbnn_ensemble_uncertainty (include/tbnn.h) and of predictor.calibration in NumPy, written from the definitions
and independently of tensorbnn_amd/predictor.py: the reference of tests/test_gpu_uncertainty.py and tests/test_uncertainty_host.py.

Input: the fp32 forward outputs f [m, d_out, n] of the m networks (Chain.forward_many's).  Per-network quantities are formed in fp64 from
the fp32 values (the softmax in fp64 of the fp32 logits, the Bernoulli clip in fp32 as the device clips), the sums over the networks in
np.longdouble where that type is wider than fp64 (x86: a 64-bit significand), as the moments test sums.
"""
import numpy as np

LD = np.longdouble if np.finfo(np.longdouble).eps < 2.0 ** -60 else np.float64
B_LO, B_HI = np.float32(1e-8), np.float32(1) - np.float32(1e-7)               # the Bernoulli clip, fp32 constants


def softmax64(f):
    """fp64 softmax over axis 1 of the fp32 logits f [m, K, n]"""
    f = np.asarray(f, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(f - f.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)


def neg_xlogx(p):
    """-p log p elementwise, 0 at p = 0, in the dtype of p"""
    p = np.asarray(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p == 0, 0, -(p * np.log(np.where(p == 0, 1, p))))


def network_probs(f, kind):
    """every network's own label probabilities in fp64: categorical the softmax [m, K, n]; Bernoulli the clipped output [m, d_out, n]"""
    if kind == "categorical":
        return softmax64(f)
    return np.clip(np.asarray(f, dtype=np.float32), B_LO, B_HI).astype(np.float64)


def binary_entropy(p):
    p = np.asarray(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -(np.where(p == 0, 0, p * np.log(np.where(p == 0, 1, p))) + np.where(p == 1, 0, (1 - p) * np.log1p(-np.where(p == 1, 0, p))))


def uncertainty(f, w, kind):
    """dict of fp64 arrays: probs, votes [d_out, n]; total, aleatoric, epistemic ([n] categorical, [d_out, n] Bernoulli); and for the
    tests' error models p [m, d_out, n] (each network's probabilities), H [m, ...] (its entropies), arg [m, n] (categorical: its votes).
    A NaN among a row's (Bernoulli: an element's) values under any network makes every output of that row (element) NaN."""
    f = np.asarray(f, dtype=np.float32)
    m, K, n = f.shape
    ww = np.ones(m, dtype=LD) if w is None else np.asarray(w, dtype=np.float32).astype(LD)
    W = ww.sum()
    p = network_probs(f, kind)
    pl = p.astype(LD)
    if kind == "categorical":
        H = neg_xlogx(pl).sum(axis=1)                                            # [m, n]
        arg = np.argmax(np.where(np.isnan(p), -1.0, p), axis=1)                  # the first of equal maxima
        ind = (arg[:, None, :] == np.arange(K)[None, :, None]).astype(LD)
        bad = np.isnan(f).any(axis=(0, 1))                                       # [n]
        nan_p, nan_h = bad[None, :], bad
    else:
        H = binary_entropy(pl)                                                   # [m, d_out, n]
        arg = None
        ind = (p >= 0.5).astype(LD)
        bad = np.isnan(f).any(axis=0)                                            # [d_out, n]
        nan_p, nan_h = bad, bad
    wsum = lambda a: np.tensordot(ww, np.where(np.isnan(a), 0, a), axes=(0, 0)) / W
    probs, votes, aleatoric = wsum(pl), wsum(ind), wsum(H)
    total = neg_xlogx(probs).sum(axis=0) if kind == "categorical" else binary_entropy(probs)
    epistemic = np.maximum(total - aleatoric, 0)
    out = {"probs": np.where(nan_p, np.nan, probs), "votes": np.where(nan_p, np.nan, votes), "total": np.where(nan_h, np.nan, total),
           "aleatoric": np.where(nan_h, np.nan, aleatoric), "epistemic": np.where(nan_h, np.nan, epistemic)}
    out = {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}
    out.update(p=p, H=np.asarray(H, dtype=np.float64), arg=arg)
    return out


def variation_ratio(votes, kind):
    votes = np.asarray(votes, dtype=np.float64)
    return 1.0 - votes.max(axis=0) if kind == "categorical" else 1.0 - np.maximum(votes, 1.0 - votes)


def labels_of(Y, K, rows, kind):
    """the labels the calibration reads: categorical an integer vector [rows] as it is, else the first arg-max of each row of [rows, K];
    Bernoulli y >= 1/2 of [rows, d_out] (or [rows]), returned [d_out, rows]"""
    y = np.asarray(Y)
    if kind == "categorical":
        return y.astype(np.int64) if y.ndim == 1 else np.argmax(y.reshape(rows, K), axis=1)
    return y.reshape(rows, K).T >= 0.5


def calibration(probs, Y, bins, kind):
    """The calibration table of probs [d_out, rows] against the labels, by loops over the bins: (lo, hi] each, 0 in the first."""
    p = np.asarray(probs, dtype=np.float64)
    K, rows = p.shape
    label = labels_of(Y, K, rows, kind)
    if kind == "categorical":
        predicted = np.array([int(np.flatnonzero(p[:, r] == p[:, r].max())[0]) for r in range(rows)])
        confidence = p.max(axis=0)
        correct = predicted == label
        with np.errstate(divide="ignore"):
            nll = np.mean([-np.log(p[label[r], r]) for r in range(rows)])
        y1 = np.eye(K)[label].T
        brier = np.mean(((p - y1) ** 2).sum(axis=0))
    else:
        p = np.clip(p, float(B_LO), float(B_HI))
        predicted = (p >= 0.5).astype(np.int64)
        confidence = np.maximum(p, 1.0 - p)
        correct = predicted == label
        nll = np.mean(np.where(label, -np.log(p), -np.log1p(-p)))
        brier = np.mean((p - label.astype(np.float64)) ** 2)
    edges = np.linspace(0.0, 1.0, bins + 1)
    c, ok = confidence.reshape(-1), correct.reshape(-1)
    count, conf_b, acc_b = np.zeros(bins, dtype=np.int64), np.full(bins, np.nan), np.full(bins, np.nan)
    ece, mce = 0.0, 0.0
    for b in range(bins):
        inside = (c <= edges[b + 1]) & ((c > edges[b]) if b else (c >= 0.0))
        count[b] = inside.sum()
        if count[b]:
            conf_b[b], acc_b[b] = c[inside].mean(), ok[inside].mean()
            gap = abs(acc_b[b] - conf_b[b])
            ece += count[b] / c.size * gap
            mce = max(mce, gap)
    return {"accuracy": float(np.mean(correct)), "nll": float(nll), "brier": float(brier), "ece": float(ece), "mce": float(mce),
            "bins": {"edges": edges, "count": count, "confidence": conf_b, "accuracy": acc_b},
            "predicted": predicted, "confidence": confidence, "correct": correct}
