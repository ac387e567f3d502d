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
// The transforms and the Bernoulli / categorical terms are evaluated in fp32 like the sampler's kernels (kernels_generic.hpp); the Gaussian
// term has no transcendental per element and is formed in fp64 from the fp32 prediction.  Streaming VALU kernels: no MFMA, no inline asm.
#pragma once
#include "common.hpp"

#define ENS_TB 256      // threads per workgroup
#define ENS_KT 8        // outputs of a row a softmax thread carries in registers at a time
#define ENS_NT 64       // networks per LDS tile of the per-network reduction

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
