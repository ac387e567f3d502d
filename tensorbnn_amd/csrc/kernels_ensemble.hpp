// Reductions over the network axis of an ensemble's predictions (tbnn_ensemble_moments / tbnn_ensemble_loglik, include/tbnn.h).
//
// Input of both kernels: one chunk out[c][d_out][n] of the forward passes tbnn_forward_many runs (c networks, n the fast axis), still on
// the device.  Threads run along n (coalesced), the loop over the chunk's networks is inside the thread: one pass, no atomics, and every
// result is the same whatever the grid.  All sums are fp64; what crosses chunks lives in fp64 device buffers the host driver owns:
//
//   moments   acc[3][d_out n] = t_ref, S1 = sum_i w_i (t_i - t_ref), S2 = sum_i w_i (t_i - t_ref)^2.  t_ref is the FIRST network's value:
//             the shift keeps S2 - S1^2 / W free of the cancellation of raw second moments, and a later chunk shifts by the same amount
//             because it reads t_ref back.  W = sum_i w_i is one number for all elements: the host sums it (fp64, network order).
//             k_ens_moments_finish: mean = t_ref + S1 / W, var = S2 / W - (S1 / W)^2 (population form).
//   loglik    lse[2][n] = running maximum M and sum S of exp(log w_i + l_i - M) per row (l_i: the row's log-likelihood under network i,
//             summed over its outputs); k_ens_lppd_finish: M + log S - log W.  Per network, the rows of a workgroup are summed over the
//             wavefront (shuffles), then over the four waves through LDS in a fixed order, into part[workgroup][network]; the host adds
//             the workgroups in index order, so the per-network sums are the same from run to run.
//
//   quantiles the block [m][d_out][rb] of ALL m networks over a block of rows (a quantile needs every network's value of an element at once,
//             so the host cuts the rows, not the networks).  k_ens_transform writes t_i over f_i in place; k_ens_quantiles selects order
//             statistics exactly, without a sort: it fixes the bits of the order-preserving 32-bit key of the answer from the top, each
//             pass re-reading the element's m values (stride tot, coalesced) and counting those at or below the trial key.
//   diagnostics the same block, its network axis read as chains x draws: k_ens_diagnostics forms split-R-hat and the effective sample size
//             of every element (definition: include/tbnn.h, tbnn_ensemble_diagnostics) from centred fp64 sums, the autocovariances in
//             batches of ENS_LB lags that share one read of the chain.
//
// The transforms and the Bernoulli / categorical terms are evaluated in fp32 like the sampler's kernels (kernels_generic.hpp); the Gaussian
// term has no transcendental per element and is formed in fp64 from the fp32 prediction.  Streaming VALU kernels: no MFMA, no inline asm.
#pragma once
#include "common.hpp"

#define ENS_TB 256      // threads per workgroup
#define ENS_KT 8        // outputs of a row a softmax thread carries in registers at a time
#define ENS_NT 64       // networks per LDS tile of the per-network reduction
#define ENS_LB 8        // lags whose autocovariance sums a diagnostics thread carries in registers at a time (k_ens_diagnostics)
#define ENS_MAX_CHAINS 64   // chains of tbnn_ensemble_diagnostics / tbnn_series_diagnostics: 128 split-chain means per element in the scratch
#define ENS_QP 8        // probabilities whose bisection states a quantile thread carries in registers at a time (k_ens_quantiles' QP: this or half)

// t = xform(f) * scale + shift, the de-normalisation of tbnn_metrics (softmax: the caller passes the probability as f)
__device__ __forceinline__ float ens_xform(float f, int xform) {
    if (xform == TBNN_XFORM_EXP) return expf(f);
    if (xform == TBNN_XFORM_SIGMOID) return 1.f / (1.f + expf(-f));
    return f;
}

// exp(f - mx) for the softmax: the fp32 difference of two logits is rounded (half an ulp32 of up to 160 at saturated logits: 64 ulp32 of the
// exponential), so it is taken in fp64, where it is exact, and what its fp32 head leaves goes in to first order
__device__ __forceinline__ float ens_exp_diff(float f, float mx) {
    const double d = (double)f - (double)mx;
    const float dh = (float)d;
    return expf(dh) * (1.f + (float)(d - (double)dh));
}

// out: the chunk [c][tot], tot = d_out n; w: the chunk's c weights or null (equal); first: the chunk starts at network 0
__global__ __launch_bounds__(ENS_TB) void k_ens_moments(const float* __restrict__ out, int c, long tot, int xform, float scale, float shift,
                                                         const float* __restrict__ w, int first, double* __restrict__ acc) {
    for (long e = (long)blockIdx.x * ENS_TB + threadIdx.x; e < tot; e += (long)gridDim.x * ENS_TB) {
        double ref, s1 = 0.0, s2 = 0.0;
        int i = 0;
        if (first) { ref = (double)(ens_xform(out[e], xform) * scale + shift); i = 1; }        // network 0: t - t_ref = 0 adds nothing
        else { ref = acc[e]; s1 = acc[tot + e]; s2 = acc[2 * tot + e]; }
#pragma unroll 4
        for (; i < c; ++i) {
            const double d = (double)(ens_xform(out[(size_t)i * tot + e], xform) * scale + shift) - ref;
            const double wd = w ? (double)w[i] * d : d;
            s1 += wd;
            s2 = fma(wd, d, s2);
        }
        acc[e] = ref; acc[tot + e] = s1; acc[2 * tot + e] = s2;
    }
}

// TBNN_XFORM_SOFTMAX: a thread owns a row and walks the d_out logits of one network twice (maximum, then sum), as cat_delta4 and
// likelihood.log_softmax do; it carries ENS_KT outputs' accumulators in registers and repeats the walk for the next ENS_KT
__global__ __launch_bounds__(ENS_TB) void k_ens_moments_softmax(const float* __restrict__ out, int c, long n, int d_out, float scale, float shift,
                                                                 const float* __restrict__ w, int first, double* __restrict__ acc) {
    const long tot = n * d_out;
    for (long row = (long)blockIdx.x * ENS_TB + threadIdx.x; row < n; row += (long)gridDim.x * ENS_TB) {
        for (int k0 = 0; k0 < d_out; k0 += ENS_KT) {
            double ref[ENS_KT], s1[ENS_KT], s2[ENS_KT];
#pragma unroll
            for (int j = 0; j < ENS_KT; ++j) {
                const bool on = !first && k0 + j < d_out;
                const long e = (long)(k0 + j) * n + row;
                ref[j] = on ? acc[e] : 0.0; s1[j] = on ? acc[tot + e] : 0.0; s2[j] = on ? acc[2 * tot + e] : 0.0;
            }
            for (int i = 0; i < c; ++i) {
                const float* __restrict__ f = out + (size_t)i * tot + row;
                float mx = -INFINITY, s = 0.f;
                for (int k = 0; k < d_out; ++k) mx = fmaxf(mx, f[(size_t)k * n]);
                for (int k = 0; k < d_out; ++k) s += ens_exp_diff(f[(size_t)k * n], mx);
                const double wi = w ? (double)w[i] : 1.0;
#pragma unroll
                for (int j = 0; j < ENS_KT; ++j) {
                    if (k0 + j < d_out) {
                        const double t = (double)(ens_exp_diff(f[(size_t)(k0 + j) * n], mx) / s * scale + shift);
                        if (first && i == 0) ref[j] = t;
                        const double d = t - ref[j], wd = wi * d;
                        s1[j] += wd;
                        s2[j] = fma(wd, d, s2[j]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < ENS_KT; ++j) {
                if (k0 + j < d_out) {
                    const long e = (long)(k0 + j) * n + row;
                    acc[e] = ref[j]; acc[tot + e] = s1[j]; acc[2 * tot + e] = s2[j];
                }
            }
        }
    }
}

// in place: acc[0][e] <- mean, acc[1][e] <- variance (never below 0: the subtraction may round there)
__global__ __launch_bounds__(ENS_TB) void k_ens_moments_finish(double* __restrict__ acc, long tot, double W) {
    for (long e = (long)blockIdx.x * ENS_TB + threadIdx.x; e < tot; e += (long)gridDim.x * ENS_TB) {
        const double m1 = acc[tot + e] / W;
        acc[e] += m1;
        acc[tot + e] = fmax(fma(-m1, m1, acc[2 * tot + e] / W), 0.0);
    }
}

// log-likelihood of one row under one network, summed over the row's outputs.  f: the row's predictions, stride n; y: its d_out targets.
//   Gaussian kinds   -log sigma - 1/2 ((y - f) / sigma)^2 - 1/2 log 2 pi per output (layer.py _multivariate_log_prob; sigma clipped by the host,
//                    cst = -log sigma - 1/2 log 2 pi)
//   Bernoulli        xlogy(y, p) + xlog1py(1 - y, -p), p = clip(f, 1e-8, 1 - 1e-7) (likelihood.py:78-80; kernels_generic.hpp)
//   categorical      sum_k y_k (f_k - max - log sum_j exp(f_j - max)) (likelihood.py:86-107)
//   Poisson          y f - exp(f) - lgamma(y + 1) per output, f the log-rate, in fp64 (include/tbnn.h TBNN_LIK_POISSON)
__device__ __forceinline__ double ens_row_loglik(int lik, const float* __restrict__ f, long n, const float* __restrict__ y, int d_out, float sigma,
                                                 double cst) {
    double l = 0.0;
    if (lik == TBNN_LIK_CATEGORICAL) {
        float mx = -INFINITY, s = 0.f;
        for (int k = 0; k < d_out; ++k) mx = fmaxf(mx, f[(size_t)k * n]);
        double t = 0.0, sy = 0.0;
        for (int k = 0; k < d_out; ++k) {
            const float d = f[(size_t)k * n] - mx;
            s += expf(d);
            sy += (double)y[k];
            t = fma((double)y[k], (double)d, t);
        }
        l = t - sy * (double)logf(s);
    } else if (lik == TBNN_LIK_POISSON) {
        for (int k = 0; k < d_out; ++k) {
            const double fk = (double)f[(size_t)k * n], yk = (double)y[k];
            l += fma(yk, fk, -exp(fk)) - lgamma(yk + 1.0);
        }
    } else if (lik == TBNN_LIK_BERNOULLI) {
        for (int k = 0; k < d_out; ++k) {
            const float p = fminf(fmaxf(f[(size_t)k * n], 1e-8f), 1.f - 1e-7f), yk = y[k];
            const float t1 = (yk == 0.f) ? 0.f : yk * logf(p);
            const float t2 = (1.f - yk == 0.f) ? 0.f : (1.f - yk) * log1pf(-p);
            l += (double)t1 + (double)t2;
        }
    } else {
        for (int k = 0; k < d_out; ++k) {
            const double d = ((double)y[k] - (double)f[(size_t)k * n]) / (double)sigma;
            l += fma(-0.5 * d, d, cst);
        }
    }
    return l;
}

// One row per thread (the grid covers n).  sig / cst: the chunk's c sigmas and constants (Gaussian kinds; else unused); lw: the chunk's c
// log weights, -inf for a weight of 0, or null (equal: log 1); lse: [2][n] or null (no row-wise mixture wanted); part: [gridDim.x][c] or null
__global__ __launch_bounds__(ENS_TB) void k_ens_loglik(const float* __restrict__ out, int c, long n, int d_out, int lik, const float* __restrict__ Y,
                                                        const float* __restrict__ sig, const double* __restrict__ cst, const double* __restrict__ lw,
                                                        int first, double* __restrict__ lse, double* __restrict__ part) {
    __shared__ double red[ENS_NT][ENS_TB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row = (long)blockIdx.x * ENS_TB + tid;
    const bool valid = row < n;
    const long tot = n * d_out;
    double M = -INFINITY, S = 0.0;
    if (valid && lse && !first) { M = lse[row]; S = lse[n + row]; }
    for (int i0 = 0; i0 < c; i0 += ENS_NT) {
        const int ct = min(ENS_NT, c - i0);
        for (int ii = 0; ii < ct; ++ii) {
            const int i = i0 + ii;
            double l = 0.0;
            if (valid) {
                l = ens_row_loglik(lik, out + (size_t)i * tot + row, n, Y + (size_t)row * d_out, d_out, sig ? sig[i] : 1.f, cst ? cst[i] : 0.0);
                if (lse) {
                    const double a = (lw ? lw[i] : 0.0) + l;
                    if (a > M) { S = fma(S, exp(M - a), 1.0); M = a; }            // (M = -inf: S = 0, exp(-inf) = 0)
                    else if (a != -INFINITY) S += exp(a - M);                    // (a NaN prediction stays visible)
                }
            }
            if (part) {
                const double s = wave_sum(l);
                if (lane == 0) red[ii][wave] = s;
            }
        }
        if (part) {
            __syncthreads();
            if (tid < ct) part[(size_t)blockIdx.x * c + i0 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
            __syncthreads();
        }
    }
    if (valid && lse) { lse[row] = M; lse[n + row] = S; }
}

// in place: lse[0][row] <- log sum_i w_i p(y_row | theta_i) - log W
__global__ __launch_bounds__(ENS_TB) void k_ens_lppd_finish(double* __restrict__ lse, long n, double logW) {
    for (long row = (long)blockIdx.x * ENS_TB + threadIdx.x; row < n; row += (long)gridDim.x * ENS_TB)
        lse[row] = lse[row] + log(lse[n + row]) - logW;
}

// ---- quantiles ----
// t = xform(f) * scale + shift over f, in place, by the expressions of k_ens_moments.  items = m tot
__global__ __launch_bounds__(ENS_TB) void k_ens_transform(float* __restrict__ out, long items, int xform, float scale, float shift) {
    for (long e = (long)blockIdx.x * ENS_TB + threadIdx.x; e < items; e += (long)gridDim.x * ENS_TB)
        out[e] = ens_xform(out[e], xform) * scale + shift;
}

// TBNN_XFORM_SOFTMAX: a thread owns one network's row (item = network * n + row) and walks its d_out logits as k_ens_moments_softmax does;
// the third walk overwrites them, which nothing reads again
__global__ __launch_bounds__(ENS_TB) void k_ens_transform_softmax(float* __restrict__ out, int m, long n, int d_out, float scale, float shift) {
    const long items = (long)m * n;
    for (long it = (long)blockIdx.x * ENS_TB + threadIdx.x; it < items; it += (long)gridDim.x * ENS_TB) {
        float* __restrict__ f = out + (size_t)(it / n) * n * d_out + it % n;
        float mx = -INFINITY, s = 0.f;
        for (int k = 0; k < d_out; ++k) mx = fmaxf(mx, f[(size_t)k * n]);
        for (int k = 0; k < d_out; ++k) s += ens_exp_diff(f[(size_t)k * n], mx);
        for (int k = 0; k < d_out; ++k) f[(size_t)k * n] = ens_exp_diff(f[(size_t)k * n], mx) / s * scale + shift;
    }
}

// the order-preserving key of an fp32 value: a < b as numbers <=> key(a) < key(b) as unsigned (-0 below +0; NaNs at both ends, past the
// infinities: the caller counts them apart)
__device__ __forceinline__ unsigned ens_key(float v) {
    const unsigned b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ens_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// t: the block [m][tot] of transformed values; w: m weights or null; probs[2][np]: the probabilities p and LINEAR's h = (m - 1) p, the
// ROUNDED fp64 product NumPy forms (the host multiplies: here the compiler would fuse it with the subtraction of floor(h), and the fraction
// g would differ from NumPy's by up to half an ulp of h, m 2^-54); res[np][tot].  Per element and probability
// the smallest key K whose cumulative count (weights: fp64 sum in network order) reaches the target:
//   LINEAR        count(key_i <= K) >= lo + 1, lo = floor((m - 1) p): K is t_(lo).  One more pass gives count(<= K) and the smallest key
//                 above K: t_(lo+1) is t_(lo) itself when the count reaches lo + 2, else that key.  g = 0: t_(lo) as it is.
//   INVERTED_CDF  sum_{key_i <= K} w_i >= p W and > 0 (the second: p = 0 does not stop below the first network with a weight).  Without
//                 weights the count to reach is ceil(x), x the ROUNDED fp64 product p m -- NumPy's own index for any p, dyadic or not:
//                 it forms the same product, subtracts 1 (exact for x >= 1/2: x and 1 are multiples of ulp(x) and the difference is
//                 smaller than x) and takes floor(x - 1) + (x - 1 is no integer), which is ceil(x) - 1; below 1/2 both clamp to t_(0)
// K is built from the top: with the bits above `bit` fixed, the trial key sets `bit` to 0 and all below it to 1; the target is reached
// there <=> the bit is 0.  32 passes, whatever the values; a thread owns its element, so the result does not depend on the grid.
// QP: the probabilities that share a read, ENS_QP or, for the interval call's three, half of it -- every slot is compared against every
// value, live or not, and a slot's result does not depend on its neighbours.
template <bool WEIGHTED, int QP>
__global__ __launch_bounds__(ENS_TB) void k_ens_quantiles(const float* __restrict__ t, int m, long tot, const float* __restrict__ w, int method,
                                                           const double* __restrict__ probs, int np, double W, double* __restrict__ res) {
    for (long e = (long)blockIdx.x * ENS_TB + threadIdx.x; e < tot; e += (long)gridDim.x * ENS_TB) {
        const float* __restrict__ te = t + e;
        int nans = 0;
        for (int p0 = 0; p0 < np; p0 += QP) {
            unsigned K[QP];
            int need[QP];                          // the count to reach (no weights)
            double target[QP], g[QP];          // p W, the sum to reach (weights); LINEAR's fraction h - lo
#pragma unroll
            for (int j = 0; j < QP; ++j) {
                const double p = probs[min(p0 + j, np - 1)];       // (a slot past the last repeats it and is not written)
                K[j] = 0u; g[j] = 0.0; target[j] = p * W;
                if (method == TBNN_QUANT_LINEAR) {
                    const double hh = probs[np + min(p0 + j, np - 1)], lo = floor(hh);
                    g[j] = hh - lo; need[j] = (int)lo + 1;
                } else {
                    need[j] = max(1, (int)ceil(p * (double)m));     // unweighted: W = m
                }
            }
            for (int bit = 31; bit >= 0; --bit) {
                const unsigned low = (1u << bit) - 1u;
                int cnt[QP];
                double sum[QP];
#pragma unroll
                for (int j = 0; j < QP; ++j) { cnt[j] = 0; sum[j] = 0.0; }
#pragma unroll 8
                for (int i = 0; i < m; ++i) {
                    const float v = te[(size_t)i * tot];
                    const unsigned key = ens_key(v);
                    if (p0 == 0 && bit == 31) nans += (v != v);
                    if (WEIGHTED) {
                        const double wi = (double)w[i];
#pragma unroll
                        for (int j = 0; j < QP; ++j) sum[j] += key <= (K[j] | low) ? wi : 0.0;
                    } else {
#pragma unroll
                        for (int j = 0; j < QP; ++j) cnt[j] += key <= (K[j] | low);
                    }
                }
#pragma unroll
                for (int j = 0; j < QP; ++j) {
                    const bool reached = WEIGHTED ? (sum[j] >= target[j] && sum[j] > 0.0) : cnt[j] >= need[j];
                    if (!reached) K[j] |= 1u << bit;
                }
            }
            unsigned nxt[QP];
            int cle[QP];
#pragma unroll
            for (int j = 0; j < QP; ++j) { nxt[j] = 0xFFFFFFFFu; cle[j] = 0; }
            if (method == TBNN_QUANT_LINEAR) {
#pragma unroll 4
                for (int i = 0; i < m; ++i) {
                    const unsigned key = ens_key(te[(size_t)i * tot]);
#pragma unroll
                    for (int j = 0; j < QP; ++j) {
                        cle[j] += key <= K[j];
                        nxt[j] = key > K[j] ? min(nxt[j], key) : nxt[j];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < QP; ++j) {
                if (p0 + j < np) {
                    const double a = (double)ens_unkey(K[j]);
                    double r = a;
                    if (method == TBNN_QUANT_LINEAR && g[j] > 0.0) {
                        const double b = cle[j] >= need[j] + 1 ? a : (double)ens_unkey(nxt[j]);
                        r = a + g[j] * (b - a);
                    }
                    res[(size_t)(p0 + j) * tot + e] = nans ? (double)NAN : r;
                }
            }
        }
    }
}

// ---- split-R-hat and effective sample size ----
// t: the block [m][tot] of transformed values, m = C S, network i = c S + s (chain-major); mu: scratch [2 C][tot]; rhat, ess: [tot], either
// may be null.  A thread owns its element (the result does not depend on the grid) and walks, all in fp64:
//   means     split chain k = 2 c + h holds the N = S / 2 draws of chain c from s = 0 (h = 0) or from s = S - N (h = 1; an odd S drops the
//             middle draw); mu_k = sum_s x[k][s] / N in s order, kept in mu[k][e]; a NaN among the m values is counted here.
//   lags      ENS_LB at a time, l0 .. l0 + ENS_LB - 1: per split chain a window w[q] = d[s + l0 + q] (d = x - mu_k, 0 past the chain's end)
//             slides along the chain, so one load of d[s] and one of the value entering the window feed ENS_LB sums
//             acc[q] += d[s] w[q].  Every a_k(l) = acc / N is summed over s in order whatever ENS_LB is (a padded product adds 0 to a
//             finished sum); A(l) = sum_k a_k(l) / K in k order.
//   Geyer     the batch's pairs P = rho(2 j) + rho(2 j + 1) are consumed in order; the thread leaves the lag loop after the batch that
//             holds the first P <= 0 (lanes of a wave diverge there); lags of that batch past the stop are not used.
// Registers: acc, w and A are ENS_LB doubles each (48 VGPRs), indexed by unrolled constants only.
__device__ __forceinline__ double ens_centred(const float* __restrict__ x, long tot, int idx, int N, double mu) {
    return idx < N ? (double)x[(size_t)idx * tot] - mu : 0.0;
}

__global__ __launch_bounds__(ENS_TB) void k_ens_diagnostics(const float* __restrict__ t, int C, int S, long tot, double* __restrict__ mu,
                                                             double* __restrict__ rhat, double* __restrict__ ess) {
    const int N = S / 2, K = 2 * C;
    const double dN = (double)N, dK = (double)K;
    for (long e = (long)blockIdx.x * ENS_TB + threadIdx.x; e < tot; e += (long)gridDim.x * ENS_TB) {
        const float* __restrict__ te = t + e;
        double* __restrict__ mue = mu + e;
        int nans = 0;
        double msum = 0.0;
        for (int k = 0; k < K; ++k) {
            const float* __restrict__ x = te + (size_t)((k >> 1) * S + ((k & 1) ? S - N : 0)) * tot;
            double s1 = 0.0;
#pragma unroll 4
            for (int s = 0; s < N; ++s) {
                const float v = x[(size_t)s * tot];
                nans += (v != v);
                s1 += (double)v;
            }
            if ((S & 1) && (k & 1)) { const float v = te[(size_t)((k >> 1) * S + N) * tot]; nans += (v != v); }     // the dropped middle draw
            s1 /= dN;
            mue[(size_t)k * tot] = s1;
            msum += s1;
        }
        // Bn: the sample variance (ddof = 1) of the K means, two passes
        msum /= dK;
        double Bn = 0.0;
        for (int k = 0; k < K; ++k) {
            const double d = mue[(size_t)k * tot] - msum;
            Bn = fma(d, d, Bn);
        }
        Bn /= dK - 1.0;
        double Wv = 0.0, Vp = 0.0, Pprev = 0.0, Psum = 0.0;
        bool live = !nans;
        for (int l0 = 0; l0 < N && live; l0 += ENS_LB) {
            double A[ENS_LB];
#pragma unroll
            for (int q = 0; q < ENS_LB; ++q) A[q] = 0.0;
            for (int k = 0; k < K; ++k) {
                const float* __restrict__ x = te + (size_t)((k >> 1) * S + ((k & 1) ? S - N : 0)) * tot;
                const double m = mue[(size_t)k * tot];
                double acc[ENS_LB], w[ENS_LB];
#pragma unroll
                for (int q = 0; q < ENS_LB; ++q) { acc[q] = 0.0; w[q] = ens_centred(x, tot, l0 + q, N, m); }
                // ENS_LB steps at a time, the window a ring with constant indices: at step s0 + j slot (j + q) % ENS_LB holds d[s + l0 + q], and
                // slot j, used last as q = 0, takes the value that enters.  Steps past N - 1 - l0 multiply by the padding: they add 0.
                for (int s0 = 0; s0 < N - l0; s0 += ENS_LB) {
#pragma unroll
                    for (int j = 0; j < ENS_LB; ++j) {
                        const double ds = ens_centred(x, tot, s0 + j, N, m);
#pragma unroll
                        for (int q = 0; q < ENS_LB; ++q) acc[q] = fma(ds, w[(j + q) % ENS_LB], acc[q]);
                        w[j] = ens_centred(x, tot, s0 + j + l0 + ENS_LB, N, m);
                    }
                }
#pragma unroll
                for (int q = 0; q < ENS_LB; ++q) A[q] += acc[q] / dN;
            }
#pragma unroll
            for (int q = 0; q < ENS_LB; ++q) A[q] /= dK;
            if (l0 == 0) {
                Wv = A[0] * dN / (dN - 1.0);
                Vp = Wv * (dN - 1.0) / dN + Bn;
                live = Wv > 0.0;                    // (a NaN from an infinity among the values is not > 0 either)
                if (!live || !ess) break;
            }
            // pairs (l0 + 2 j, l0 + 2 j + 1), 2 k + 1 <= N - 1; the first is P_0 = 1 + rho(1)
#pragma unroll
            for (int j = 0; j < ENS_LB / 2; ++j) {
                if (live && l0 + 2 * j + 1 <= N - 1) {
                    const double r1 = 1.0 - (Wv - A[2 * j + 1]) / Vp;
                    if (l0 + j == 0) {
                        Pprev = 1.0 + r1;
                        Psum = Pprev;
                    } else {
                        const double P = (1.0 - (Wv - A[2 * j]) / Vp) + r1;
                        if (P > 0.0) { Pprev = fmin(Pprev, P); Psum += Pprev; }
                        else live = false;
                    }
                }
            }
        }
        const bool defined = !nans && Wv > 0.0;
        if (rhat) rhat[e] = defined ? sqrt(Vp / Wv) : (double)NAN;
        if (ess) {
            const double tau = fmax(2.0 * Psum - 1.0, 1.0 / log10(dK * dN));
            ess[e] = defined ? dK * dN / tau : (double)NAN;
        }
    }
}
