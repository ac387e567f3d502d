"""REF_FIG of tests/test_gpu_count_crps.py: the largest relative difference between tests/count_crps_ref.py (SciPy, fp64) and the same
three sums in 50-digit mpmath, over the first six rows (one per kind of target) of every case of test_against_reference and of the
large-rate case.  CPU only: the log-rates of those cases are the networks' last biases, so no forward pass is needed.

    python tools/count_crps_ref_fig.py

In mpmath a component's pmf starts at p(0) = exp(-mu) (q^r) and moves by its ratio recurrence; F is the running sum, S = 1 - F (exact
to 50 digits), over the reference's own k = 0 .. K."""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import count_crps_ref as cc                                             # noqa: E402

mp.mp.dps = 50


def mp_sums(f, w, ys, lik, r, n_k):
    om = np.asarray(w, np.float64) / np.sum(w, dtype=np.float64)
    mus = [mp.mpf(float(v)) for v in np.exp(np.asarray(f, np.float64))]
    F = [mp.mpf(0)] * n_k
    for o, mu in zip(om, mus):
        if not o > 0:
            continue
        o = mp.mpf(float(o))
        if lik == cc.POIS:
            p, step = mp.exp(-mu), lambda p, k: p * mu / (k + 1)
        else:
            rr = mp.mpf(r)
            q = rr / (rr + mu)
            p, step = q ** rr, lambda p, k: p * (k + rr) / (k + 1) * (1 - q)
        c = mp.mpf(0)
        for k in range(n_k):
            c += p
            F[k] += o * c
            p = step(p, k)
    out = []
    for y in ys:
        up = [float(y) <= k for k in range(n_k)]
        v = [1 - F[k] if up[k] else F[k] for k in range(n_k)]
        out.append((mp.fsum(x * x for x in v), mp.fsum(v), mp.fsum(F[k] * (1 - F[k]) for k in range(n_k))))
    return out


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    from test_gpu_count_crps import CASES, LARGE, weights
    jobs = [(lik, r, LARGE, None) if m == "large" else (lik, r, cc.log_rates(m, d_out), weights(m, wt)) for lik, r, m, d_out, _rows, wt in CASES]
    worst, seen = 0.0, set()
    for lik, r, f, w in jobs:
        w = np.ones(f.shape[0]) if w is None else w
        Y = cc.targets(f, 6)
        for j in range(f.shape[1]):
            key = (lik, r, f[:, j].tobytes(), np.asarray(w).tobytes())
            if key in seen:
                continue
            seen.add(key)
            ref = cc.count_crps_ref(f[:, j], w, Y[:, j], lik, r)
            big = mp_sums(f[:, j], w, Y[:, j], lik, r, ref[3])
            rel = max(float(abs(mp.mpf(float(ref[a][i])) - big[i][a]) / max(1, abs(big[i][a]))) for i in range(6) for a in range(3))
            worst = max(worst, rel)
            print(f"lik {lik} r {r} m {f.shape[0]} output {j}: n_k {ref[3]}, largest relative difference {rel:.3e}", flush=True)
    print(f"largest relative difference {worst:.3e}; REF_FIG = 4 x that = {4 * worst:.3e}")


if __name__ == "__main__":
    main()
