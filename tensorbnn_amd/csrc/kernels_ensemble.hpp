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
//   uncertainty acc = S[d_out n], V[d_out n], A[rt], then two result planes [rt] (rt = n categorical, d_out n Bernoulli): the plain sums
//             S_k = sum_i w_i p_ik of each network's own label probabilities, V_k = sum_i w_i [a_i == k] of its votes (Bernoulli:
//             [p_i >= 1/2]) and A = sum_i w_i H_i of its entropies H_i = -sum_k p_ik log p_ik -- the direct form, log and sum in fp64
//             from the fp32 p_ik, 0 log 0 = 0.  The values lie in [0, 1]: no shift.  A later chunk reads the three back and goes on in
//             network order.  k_ens_uncert_finish*: pbar = S / W, vote = V / W, total = H[pbar], aleatoric = A / W, epistemic =
//             total - aleatoric, not below 0 (Jensen: only rounding takes it there).  A NaN among a row's values under any network
//             makes every output of the row NaN, whatever that network's weight.  Contraction off.
//
//   quantiles the block [m][d_out][rb] of ALL m networks over a block of rows (a quantile needs every network's value of an element at once,
//             so the host cuts the rows, not the networks).  k_ens_transform writes t_i over f_i in place; k_ens_quantiles selects order
//             statistics exactly, without a sort: it fixes the bits of the order-preserving 32-bit key of the answer from the top, each
//             pass re-reading the element's m values (stride tot, coalesced) and counting those at or below the trial key.
//   diagnostics the same block, its network axis read as chains x draws: k_ens_diagnostics forms split-R-hat and the effective sample size
//             of every element (definition: include/tbnn.h, tbnn_ensemble_diagnostics) from centred fp64 sums, the autocovariances in
//             batches of ENS_LB lags that share one read of the chain.
//   predictive  the same block, untransformed: the posterior-predictive distribution of a NEW observation, the mixture over the networks of
//             the observation model around each prediction (definition: include/tbnn.h, tbnn_ensemble_predictive).  k_ens_pred_cdf
//             evaluates the mixture CDF at each element's target in one pass; k_ens_pred_quantiles inverts it per element and
//             probability -- Gaussian kinds: a verified bracket, then Newton steps safeguarded by bisection; Poisson: a search over the
//             integers -- every trial one pass over the element's m predictions.  All fp64, contraction off: a slot's result does not
//             depend on its neighbours or on the grid.
//   loo         the same block, untransformed: k_ens_pointwise writes the matrix l[m][rb] of row log-likelihoods (ens_row_loglik, the terms of
//             k_ens_loglik) with the rows' lppd and p_waic; k_ens_psis smooths each row's importance ratios (definition: include/tbnn.h,
//             tbnn_ensemble_loo): the cutoff by bisection on the order-preserving 64-bit key, the tail gathered into a scratch [M][rb] and
//             ranked there by counting, the generalised Pareto fit in one sweep over the G candidates.  All fp64, contraction off.
//   crps        the same block, untransformed: k_ens_crps forms the continuous ranked probability score of the predictive mixture (definition:
//             include/tbnn.h, tbnn_ensemble_crps) from its closed form, a sum over all PAIRS of networks.  The one kernel here that is not
//             one thread per element: ENS_CL lanes share an element, each holds one network of a tile in registers and walks the other
//             tile's networks from LDS (layout and summation order: at the kernel).  All fp64, contraction off, no atomics.
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
#define ENS_PQ 4        // probabilities whose root-search states a predictive-quantile thread carries in registers at a time (k_ens_pred_quantiles' QP)
#define ENS_PRED_PASSES 256   // trial points per probability at the most (Gaussian: the moves at least halve, a bisection at the worst; Poisson: <= 2 log2 of the count)
#define ENS_POIS_MAX_RATE 1073741824.0   // 2^30: a larger (or non-finite) rate makes the element NaN
#define ENS_NB_MAX 1048576.0             // 2^20: the negative binomial's ceiling on the rate AND on the count k; beyond either the element is NaN
#define ENS_CT 8        // networks per tile of the pair kernel (k_ens_crps): one per lane of an element
#define ENS_CE 32       // elements a workgroup of the pair kernel owns
#define ENS_CL (ENS_TB / ENS_CE)   // lanes that share an element there: one network of a tile each, so ENS_CL == ENS_CT
#define ENS_CRPS_MAX_M 4096   // networks of tbnn_ensemble_crps at the most: a launch is quadratic in m (a limit of the interface)

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

// ---- classification uncertainty: entropy split and votes (tbnn_ensemble_uncertainty) ----
// -x log x in fp64, 0 at x = 0 (a NaN stays NaN: the comparison is false)
__device__ __forceinline__ double ens_neg_xlogx(double x) {
#pragma clang fp contract(off)
    return x == 0.0 ? 0.0 : -(x * log(x));
}

// Bernoulli: an element is an (output, row) pair, as in k_ens_moments.  acc: S[tot], V[tot], A[tot] (then the finish kernel's two planes).
// p = clip(f, 1e-8, 1 - 1e-7) in fp32 (ens_row_loglik's clip, which swallows a NaN: it is carried beside the sums instead)
__global__ __launch_bounds__(ENS_TB) void k_ens_uncert(const float* __restrict__ out, int c, long tot, const float* __restrict__ w, int first,
                                                        double* __restrict__ acc) {
#pragma clang fp contract(off)
    for (long e = (long)blockIdx.x * ENS_TB + threadIdx.x; e < tot; e += (long)gridDim.x * ENS_TB) {
        double s = 0.0, v = 0.0, a = 0.0;
        if (!first) { s = acc[e]; v = acc[tot + e]; a = acc[2 * tot + e]; }
#pragma unroll 4
        for (int i = 0; i < c; ++i) {
            const float f = out[(size_t)i * tot + e];
            const float p = fminf(fmaxf(f, 1e-8f), 1.f - 1e-7f);
            const double pd = (double)p, wi = w ? (double)w[i] : 1.0;
            const double bad = f != f ? (double)NAN : 0.0;
            const double h = -(pd * log(pd) + (1.0 - pd) * log1p(-pd));
            s += wi * pd + bad;
            v += wi * (p >= 0.5f ? 1.0 : 0.0) + bad;
            a += wi * h + bad;
        }
        acc[e] = s; acc[tot + e] = v; acc[2 * tot + e] = a;
    }
}

// in place: S <- pbar, V <- vote, A <- aleatoric; the two planes behind them <- total, epistemic
__global__ __launch_bounds__(ENS_TB) void k_ens_uncert_finish(double* __restrict__ acc, long tot, double W) {
#pragma clang fp contract(off)
    for (long e = (long)blockIdx.x * ENS_TB + threadIdx.x; e < tot; e += (long)gridDim.x * ENS_TB) {
        const double pb = acc[e] / W, q = 1.0 - pb;
        const double t1 = pb == 0.0 ? 0.0 : pb * log(pb), t2 = q == 0.0 ? 0.0 : q * log1p(-pb);
        const double total = -(t1 + t2), al = acc[2 * tot + e] / W, d = total - al;
        acc[e] = pb;
        acc[tot + e] = acc[tot + e] / W;
        acc[2 * tot + e] = al;
        acc[3 * tot + e] = total;
        acc[4 * tot + e] = d < 0.0 ? 0.0 : d;                    // (a select, not fmax: a NaN stays NaN)
    }
}

// Categorical: a thread owns a row.  acc: S[d_out][n], V[d_out][n], A[n] (then the finish kernel's two planes [n]).  Per network the
// walks of k_ens_moments_softmax (maximum, sum) and a third over the probabilities p_k = ens_exp_diff(f_k, max) / s themselves: the vote
// a_i, the smallest k with p_k maximal, and -- in the first tile's pass only -- the entropy H_i.  ENS_KT classes' S and V sit in
// registers at a time and the walks are repeated for the next ENS_KT.  A NaN logit makes s, every p_k and H_i NaN; the votes get it from s.
__global__ __launch_bounds__(ENS_TB) void k_ens_uncert_softmax(const float* __restrict__ out, int c, long n, int d_out, const float* __restrict__ w,
                                                                int first, double* __restrict__ acc) {
    const long tot = n * d_out;
    for (long row = (long)blockIdx.x * ENS_TB + threadIdx.x; row < n; row += (long)gridDim.x * ENS_TB) {
        for (int k0 = 0; k0 < d_out; k0 += ENS_KT) {
            double s1[ENS_KT], v1[ENS_KT], a = 0.0;
#pragma unroll
            for (int j = 0; j < ENS_KT; ++j) {
                const bool on = !first && k0 + j < d_out;
                const long e = (long)(k0 + j) * n + row;
                s1[j] = on ? acc[e] : 0.0; v1[j] = on ? acc[tot + e] : 0.0;
            }
            if (k0 == 0 && !first) a = acc[2 * tot + row];
            for (int i = 0; i < c; ++i) {
                const float* __restrict__ f = out + (size_t)i * tot + row;
                float mx = -INFINITY, s = 0.f;
                for (int k = 0; k < d_out; ++k) mx = fmaxf(mx, f[(size_t)k * n]);
                for (int k = 0; k < d_out; ++k) s += ens_exp_diff(f[(size_t)k * n], mx);
                // (mx and s above: the statements of k_ens_moments_softmax, contracted as there -- the same p_k bit for bit; fp64 below)
                {
#pragma clang fp contract(off)
                    const double wi = w ? (double)w[i] : 1.0;
                    const double bad = s != s ? (double)NAN : 0.0;
                    float best = -1.f;
                    int arg = 0;
                    double hsum = 0.0;
                    for (int k = 0; k < d_out; ++k) {
                        const float p = ens_exp_diff(f[(size_t)k * n], mx) / s;
                        if (p > best) { best = p; arg = k; }
                        if (k0 == 0) hsum += ens_neg_xlogx((double)p);
                    }
                    if (k0 == 0) a += wi * hsum;
#pragma unroll
                    for (int j = 0; j < ENS_KT; ++j) {
                        if (k0 + j < d_out) {
                            const double p = (double)(ens_exp_diff(f[(size_t)(k0 + j) * n], mx) / s);
                            s1[j] += wi * p;
                            v1[j] += wi * (arg == k0 + j ? 1.0 : 0.0) + bad;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < ENS_KT; ++j) {
                if (k0 + j < d_out) {
                    const long e = (long)(k0 + j) * n + row;
                    acc[e] = s1[j]; acc[tot + e] = v1[j];
                }
            }
            if (k0 == 0) acc[2 * tot + row] = a;
        }
    }
}

// in place: S <- pbar, V <- vote, A <- aleatoric; the two planes [n] behind them <- total = H[pbar] (classes in index order), epistemic
__global__ __launch_bounds__(ENS_TB) void k_ens_uncert_finish_softmax(double* __restrict__ acc, long n, int d_out, double W) {
#pragma clang fp contract(off)
    const long tot = n * d_out;
    for (long row = (long)blockIdx.x * ENS_TB + threadIdx.x; row < n; row += (long)gridDim.x * ENS_TB) {
        double total = 0.0;
        for (int k = 0; k < d_out; ++k) {
            const long e = (long)k * n + row;
            const double pb = acc[e] / W;
            total += ens_neg_xlogx(pb);
            acc[e] = pb;
            acc[tot + e] = acc[tot + e] / W;
        }
        const double al = acc[2 * tot + row] / W, d = total - al;
        acc[2 * tot + row] = al;
        acc[2 * tot + n + row] = total;
        acc[2 * tot + 2 * n + row] = d < 0.0 ? 0.0 : d;            // (a select, not fmax: a NaN stays NaN)
    }
}

// log-likelihood of one row under one network, summed over the row's outputs.  f: the row's predictions, stride n; y: its d_out targets.
//   Gaussian kinds   -log sigma - 1/2 ((y - f) / sigma)^2 - 1/2 log 2 pi per output (layer.py _multivariate_log_prob; sigma clipped by the host,
//                    cst = -log sigma - 1/2 log 2 pi)
//   Bernoulli        xlogy(y, p) + xlog1py(1 - y, -p), p = clip(f, 1e-8, 1 - 1e-7) (likelihood.py:78-80; kernels_generic.hpp)
//   categorical      sum_k y_k (f_k - max - log sum_j exp(f_j - max)) (likelihood.py:86-107)
//   Poisson          y f - exp(f) - lgamma(y + 1) per output, f the log-rate, in fp64 (include/tbnn.h TBNN_LIK_POISSON)
//   neg. binomial    lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y log p + r log q per output in fp64, p = sigmoid(f - log r), the logs in
//                    the stable form of negbin_term (common.hpp); r arrives in `nu` (ensemble_api.hpp ens_lik_consts)
//   Gamma            a log a - lgamma(a) + (a - 1) log y - a f - a y exp(-f) per output in fp64, f the log of the mean (include/tbnn.h
//                    TBNN_LIK_GAMMA); the shape a arrives in `nu`, by the rule the dispersion follows
//   Weibull          per output in fp64, f the log of the scale, t = |y|, u = exp(k (log t - f)) (include/tbnn.h TBNN_LIK_WEIBULL): an event
//                    (y > 0) gives the log density log k + (k - 1) log t - k f - u, a right-censored row (y < 0) the log survival -u; the
//                    shape k arrives in `nu`, by the rule the dispersion follows
//   Student-t        cst - (nu + 1) / 2 log1p(((y - f) / sigma)^2 / nu) per output in fp64 (include/tbnn.h TBNN_LIK_STUDENT_T; sigma clipped by
//                    the host, cst = lgamma((nu+1)/2) - lgamma(nu/2) - 1/2 log(nu pi) - log sigma: ensemble_api.hpp ens_lik_consts)
__device__ __forceinline__ double ens_row_loglik(int lik, const float* __restrict__ f, long n, const float* __restrict__ y, int d_out, float sigma,
                                                 double cst, double nu) {
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
    } else if (lik == TBNN_LIK_HETERO_GAUSSIAN) {
        // ONE term per row (d_out == 2: the host refuses anything else): f the mean, g the log-sd clipped to +-log(1e8), target column 0;
        // the definition of include/tbnn.h in fp64.  (Two selects, not fmin / fmax: a NaN g stays NaN.)
        const double G = 18.420680743952367, g = (double)f[(size_t)n];
        const double gc = g < -G ? -G : (g > G ? G : g), r = (double)y[0] - (double)f[0];
        l = -0.9189385332046727 /* 1/2 log 2pi */ - gc - 0.5 * r * r * exp(-2.0 * gc);
    } else if (lik == TBNN_LIK_POISSON) {
        for (int k = 0; k < d_out; ++k) {
            const double fk = (double)f[(size_t)k * n], yk = (double)y[k];
            l += fma(yk, fk, -exp(fk)) - lgamma(yk + 1.0);
        }
    } else if (lik == TBNN_LIK_NEG_BINOMIAL) {
        const double lr = log(nu), lgr = lgamma(nu);
        for (int k = 0; k < d_out; ++k) {
            const double yk = (double)y[k], t = (double)f[(size_t)k * n] - lr;
            const double lp1 = log1p(exp(-fabs(t)));
            l += (lgamma(yk + nu) - lgr - lgamma(yk + 1.0)) - (yk * (fmax(-t, 0.0) + lp1) + nu * (fmax(t, 0.0) + lp1));
        }
    } else if (lik == TBNN_LIK_GAMMA) {
        const double c0 = nu * log(nu) - lgamma(nu);
        for (int k = 0; k < d_out; ++k) {
            const double yk = (double)y[k], fk = (double)f[(size_t)k * n];
            l += (c0 + (nu - 1.0) * log(yk)) - nu * (fk + yk * exp(-fk));
        }
    } else if (lik == TBNN_LIK_WEIBULL) {
        const double lk = log(nu);
        for (int k = 0; k < d_out; ++k) {
            const double yk = (double)y[k], fk = (double)f[(size_t)k * n], lt = log(fabs(yk));
            const double u = exp(nu * (lt - fk));
            l += yk > 0.0 ? ((lk + (nu - 1.0) * lt) - nu * fk) - u : -u;
        }
    } else if (lik == TBNN_LIK_STUDENT_T) {
        for (int k = 0; k < d_out; ++k) {
            const double d = ((double)y[k] - (double)f[(size_t)k * n]) / (double)sigma;
            l += cst - 0.5 * (nu + 1.0) * log1p(d * d / nu);
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

// one more term a of a running log-sum-exp: M the maximum so far, S = sum exp(a_i - M)
__device__ __forceinline__ void ens_lse_step(double a, double& M, double& S) {
    if (a > M) { S = fma(S, exp(M - a), 1.0); M = a; }            // (M = -inf: S = 0, exp(-inf) = 0)
    else if (a != -INFINITY) S += exp(a - M);                    // (a NaN prediction stays visible)
}

// One row per thread (the grid covers n).  sig / cst: the chunk's c sigmas and constants (Gaussian kinds, Student-t with its nu; else unused); lw: the chunk's c
// log weights, -inf for a weight of 0, or null (equal: log 1); lse: [2][n] or null (no row-wise mixture wanted); part: [gridDim.x][c] or null
__global__ __launch_bounds__(ENS_TB) void k_ens_loglik(const float* __restrict__ out, int c, long n, int d_out, int lik, const float* __restrict__ Y,
                                                        const float* __restrict__ sig, const double* __restrict__ cst, const double* __restrict__ lw,
                                                        int first, double* __restrict__ lse, double* __restrict__ part, double nu) {
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
                l = ens_row_loglik(lik, out + (size_t)i * tot + row, n, Y + (size_t)row * d_out, d_out, sig ? sig[i] : 1.f, cst ? cst[i] : 0.0, nu);
                if (lse) {
                    ens_lse_step((lw ? lw[i] : 0.0) + l, M, S);
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

// ---- posterior-predictive CDF and quantiles with observation noise ----
// Phi((y - f) / s) as erfc(-(y - f) c) / 2, c = 1 / (s sqrt 2) staged by the host
__device__ __forceinline__ double ens_phi(double y, double f, double c) {
#pragma clang fp contract(off)
    return 0.5 * erfc(-((y - f) * c));
}

// log1p(mu) - mu.  Below |mu| < 1/32 the difference of the two would lose |mu| 2^-53 / (mu^2 / 2) of itself, so the series
// -mu^2/2 + mu^3/3 - ... is summed there (14 terms: the first left out is below 2^-57 of the result)
__host__ __device__ __forceinline__ double ens_log1pmx(double mu) {
#pragma clang fp contract(off)
    if (fabs(mu) >= 0.03125) return log1p(mu) - mu;
    double t = 0.0;
#pragma unroll
    for (int k = 15; k >= 2; --k) t = ((k & 1) ? 1.0 : -1.0) / (double)k + mu * t;
    return mu * mu * t;
}

// log of x^a e^-x / Gamma(a + 1), a > 0, x > 0.  Written out, a log x - x - lgamma(a + 1) cancels terms of size a log a, so from a = 32 on
// it is formed around the peak instead: with mu = (x - a) / a and Stirling's series for lgamma,
//   a (log1p(mu) - mu) - 1/2 log(2 pi a) - (1/(12 a) - 1/(360 a^3) + 1/(1260 a^5))        (next term 1/(1680 a^7) < 3e-14)
__host__ __device__ __forceinline__ double ens_pois_logpref(double a, double x) {
#pragma clang fp contract(off)
    if (a < 32.0) return a * log(x) - x - lgamma(a + 1.0);
    const double r = 1.0 / a, r2 = r * r;
    const double stirling = r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0)));
    return a * ens_log1pmx((x - a) / a) - 0.5 * log(6.283185307179586477 * a) - stirling;
}

#define ENS_Q_TEMME_A 65536.0    // from this a on Q(a, x) is Temme's expansion: no loop.  Below it a series or fraction of at most 10 sqrt(a) + 100 terms

// Q(a, x), the regularised upper incomplete gamma function, for a >= 1 (here an integer, k + 1) and finite x >= 0: Pr[Poisson(x) <= a - 1].
// Where x^a e^-x / Gamma(a + 1) is below e^-80 the answer is 1 or 0 to more than 1e-25 and nothing is summed.  Else, a < 2^16: below
// x < a + 1 the series P = pref sum_n x^n / ((a + 1) .. (a + n)), Q = 1 - P; from there on the continued fraction
// Q = pref a / (x + 1 - a - 1 (1 - a) / (x + 3 - a - 2 (2 - a) / (x + 5 - a - ...))) by the modified Lentz recurrence (Numerical Recipes
// section 6.2; for an integer a it ends by itself at term a); either needs a few sqrt(a) terms near x = a, fewer away from it, 2,660 at
// the most.  a >= 2^16: Temme's uniform expansion (N. M. Temme, SIAM J. Math. Anal. 10 (1979) 757; the coefficients' series in eta are those of
// DiDonato and Morris, ACM TOMS 12 (1986) 377): with eta^2 / 2 = mu - log1p(mu), eta of the sign of mu = (x - a) / a,
//   Q = erfc(eta sqrt(a / 2)) / 2 + exp(-a eta^2 / 2) / sqrt(2 pi a) (c0 + c1 / a + c2 / a^2),   c0 = 1 / mu - 1 / eta, ...
// Past the e^-80 exit |eta| < 0.05 there, where the c_k are summed from their Taylor series (the closed forms cancel); what is left out is
// below 1e-16 of Q.  So the cost of one evaluation does not grow with the rate beyond 2^16.
// The series and the fraction hold for every a > 0, an integer or not (the fraction of a non-integer a does not end by itself: it
// converges, and the cap of 10 sqrt(max(a, x)) + 100 terms holds): ens_gamma_p and the Gamma likelihood's CDF call it with any shape.
// (__host__ too: the host stages the standard Gamma quantiles that seed k_ens_pred_quantiles' bracket with the same function.)
__host__ __device__ __forceinline__ double ens_gamma_q(double a, double x) {
#pragma clang fp contract(off)
    if (x <= 0.0) return 1.0;
    const double lp = ens_pois_logpref(a, x);
    const bool series = x < a + 1.0;
    if (lp < -80.0) return series ? 1.0 : 0.0;
    if (a >= ENS_Q_TEMME_A) {
        const double mu = (x - a) / a, h = -ens_log1pmx(mu);                // eta^2 / 2
        const double eta = copysign(sqrt(2.0 * h), mu), r = 1.0 / a;
        const double c0 = -1.0 / 3.0 + eta * (1.0 / 12.0 + eta * (-2.0 / 135.0 + eta * (1.0 / 864.0 + eta * (1.0 / 2835.0 + eta * (-139.0 / 777600.0)))));
        const double c1 = -1.0 / 540.0 + eta * (-1.0 / 288.0 + eta * (1.0 / 378.0 + eta * (-77.0 / 77760.0)));
        const double c2 = 25.0 / 6048.0 + eta * (-139.0 / 51840.0);
        const double q = 0.5 * erfc(eta * sqrt(0.5 * a)) + exp(-a * h) / sqrt(6.283185307179586477 * a) * (c0 + r * (c1 + r * c2));
        return fmin(fmax(q, 0.0), 1.0);
    }
    const double pref = exp(lp);
    const int itmax = (int)(10.0 * sqrt(fmax(a, x))) + 100;
    if (series) {
        double ap = a, del = 1.0, sum = 1.0;
        for (int it = 0; it < itmax; ++it) {
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (del < sum * 1e-17) break;
        }
        return fmax(1.0 - pref * sum, 0.0);
    }
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int it = 1; it <= itmax; ++it) {
        const double an = -(double)it * ((double)it - a);
        b += 2.0;
        d = an * d + b;
        if (fabs(d) < tiny) d = tiny;
        c = b + an / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 2.3e-16) break;
    }
    return fmin(pref * a * h, 1.0);
}

// P(a, x) = 1 - Q(a, x), the regularised LOWER incomplete gamma function, for any a > 0 and x >= 0 (+inf: 1): the CDF at y of a Gamma
// distribution of shape a and mean mu is P(a, a y / mu).  On the series' side (x < a + 1, a < 2^16) it is returned as the series gives
// it, pref sum_n x^n / ((a + 1) .. (a + n)) in ens_gamma_q's own order -- a small lower tail is not formed as 1 - (1 - P); elsewhere
// 1 - Q from the fraction or Temme's expansion, where Q is the small side or both are of order 1.
__host__ __device__ __forceinline__ double ens_gamma_p(double a, double x) {
#pragma clang fp contract(off)
    if (!(x > 0.0)) return 0.0;
    if (x == (double)INFINITY) return 1.0;
    if (!(x < a + 1.0) || a >= ENS_Q_TEMME_A) return 1.0 - ens_gamma_q(a, x);
    const double lp = ens_pois_logpref(a, x);
    if (lp < -80.0) return 0.0;
    const double pref = exp(lp);
    const int itmax = (int)(10.0 * sqrt(fmax(a, x))) + 100;
    double ap = a, del = 1.0, sum = 1.0;
    for (int it = 0; it < itmax; ++it) {
        ap += 1.0;
        del *= x / ap;
        sum += del;
        if (del < sum * 1e-17) break;
    }
    return fmin(pref * sum, 1.0);
}

// ---- the regularised incomplete beta function I_x(a, b), fp64 (the negative-binomial CDF: Pr[Y <= k] = I_q(r, k + 1), q = r / (r + mu)) ----
// Stirling's correction: lgamma(z) = (z - 1/2) log z - z + 1/2 log 2 pi + ens_stirling(z); from z = 16 on the next term, 1 / (1680 z^7), is < 3e-12
__device__ __forceinline__ double ens_stirling(double z) {
#pragma clang fp contract(off)
    const double r = 1.0 / z, r2 = r * r;
    return r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0)));
}

// log of x^a y^b / B(a, b), y = 1 - x given by the caller (formed on its own, not as 1 - x).  Written out, lgamma(a + b) - lgamma(a) - lgamma(b)
// + a log x + b log y differences terms of size n log n, n = a + b: 1.4e7 at a count of 2^20, 3e-9 of the result.  So, as ens_pois_logpref
// forms its prefactor around the peak: every argument >= 16 takes Stirling's series, whose leading parts cancel in closed form --
//   a, b >= 16   1/2 log(a b / (2 pi n)) + a log1pmx(u) + b log1pmx(v) + S(n) - S(a) - S(b),  u = (x - a/n) / (a/n), v = (y - b/n) / (b/n)
//                (a u + b v = 0: the first-order parts are gone, both log1pmx terms are <= 0; x - a/n as (x b - y a) / n)
//   one < 16     with s the small and L the large one: lgamma(n) - lgamma(L) = L log1pmx(s/L) - 1/2 log1p(s/L) + s log n + S(n) - S(L),
//                then - lgamma(s) + a log x + b log y: where the result is not negligible every term is of modest size
//   both < 16    written out: no term exceeds ~50
// log x and log y through log1p of the other where they are near 1
__device__ __forceinline__ double ens_beta_logpref(double a, double b, double x, double y) {
#pragma clang fp contract(off)
    const double n = a + b;
    if (a >= 16.0 && b >= 16.0) {
        const double d = (x * b - y * a) / n;
        return 0.5 * log(a * b / (6.283185307179586477 * n)) + a * ens_log1pmx(d * n / a) + b * ens_log1pmx(-d * n / b) +
               (ens_stirling(n) - ens_stirling(a) - ens_stirling(b));
    }
    const double lx = x < 0.5 ? log(x) : log1p(-y), ly = y < 0.5 ? log(y) : log1p(-x);
    if (a < 16.0 && b < 16.0) return lgamma(n) - lgamma(a) - lgamma(b) + a * lx + b * ly;
    const double sm = fmin(a, b), lg = fmax(a, b), z = sm / lg;
    const double gr = lg * ens_log1pmx(z) - 0.5 * log1p(z) + sm * log(n) + (ens_stirling(n) - ens_stirling(lg)) - lgamma(sm);
    return gr + a * lx + b * ly;
}

// the continued fraction of I_x(a, b) a B(a, b) / (x^a y^b) by the modified Lentz recurrence (Numerical Recipes section 6.4, betacf): it
// converges in O(sqrt(max(a, b))) double steps for x < (a + 1) / (a + b + 2); never more than 10 sqrt(max(a, b)) + 100 are taken (10,340 at
// the ceiling; the grid of tests/test_gpu_negbin_predictive.py needs 129 at the most)
__device__ __forceinline__ double ens_beta_cf(double a, double b, double x) {
#pragma clang fp contract(off)
    const double tiny = 1e-300;
    const int itmax = (int)(10.0 * sqrt(fmax(a, b))) + 100;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int it = 1; it <= itmax; ++it) {
        const double m = (double)it, m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 2.3e-16) break;
    }
    return h;
}

// I_x(a, b) for a, b > 0 and x, y = 1 - x in [0, 1], both given.  The side by the usual rule: x < (a + 1) / (a + b + 2) the fraction of
// (a, b, x), else 1 minus the fraction of (b, a, y).  Where the prefactor is below e^-80 the answer is 0 or 1 to more than 1e-25 (the
// fraction over its first argument stays below ~1e7 here) and nothing is summed.  A NaN among the arguments gives NaN.
__device__ __forceinline__ double ens_betainc(double a, double b, double x, double y) {
#pragma clang fp contract(off)
    if (x != x || y != y) return (double)NAN;
    if (!(x > 0.0)) return 0.0;
    if (!(y > 0.0)) return 1.0;
    const double lp = ens_beta_logpref(a, b, x, y);
    const bool left = x < (a + 1.0) / (a + b + 2.0);
    if (lp < -80.0) return left ? 0.0 : 1.0;
    const double pref = exp(lp);
    if (left) return fmin(pref * ens_beta_cf(a, b, x) / a, 1.0);
    return fmax(1.0 - pref * ens_beta_cf(b, a, y) / b, 0.0);
}

// the negative binomial's q = r / (r + mu) = sigmoid(log r - f) and p = 1 - q = sigmoid(f - log r), each formed directly from
// e = exp(-|log r - f|): neither is a difference from 1
__device__ __forceinline__ void ens_nb_qp(double lr, double f, double& q, double& p) {
#pragma clang fp contract(off)
    const double s = lr - f, e = exp(-fabs(s)), big = 1.0 / (1.0 + e), small = e / (1.0 + e);
    q = s >= 0.0 ? big : small;
    p = s >= 0.0 ? small : big;
}

// the spacing of fp64 at |v| (v finite)
__device__ __forceinline__ double ens_ulp64(double v) {
    const double av = fabs(v);
    return __longlong_as_double(__double_as_longlong(av) + 1) - av;
}

// the heteroscedastic Gaussian's log-sd as the likelihood reads it: g clipped to +-log(1e8) (two selects: a NaN stays NaN)
__device__ __forceinline__ double ens_het_gc(float g) {
    const double G = 18.420680743952367, gd = (double)g;
    return gd < -G ? -G : (gd > G ? G : gd);
}

// (TBNN_LIK_HETERO_GAUSSIAN: an element is a ROW -- tot = r, the block is [m][2][r], network i's mean f_i at t[2 i tot + e] and its
// log-sd g_i one plane further; s_i = exp(gc_i) and c_i = exp(-gc_i) / sqrt 2 are formed per (network, row) where the Gaussian kinds read
// cst[2 m + i] and cst[m + i]; a NaN f_i or g_i of a network that counts gives NaN, one of a network of weight 0 is not looked at.)
// t: the block [m][tot] of untransformed predictions, tot = d_out r; Y: the block's targets [r][d_out]; cst[2][m]: w_i / W and, Gaussian
// kinds, 1 / (s_i sqrt 2).  cdf[tot] = F(y); below[tot] (Poisson, or null) = F(y - 1).  Networks of weight 0 add nothing; a NaN among an
// element's f_i or a NaN target (Poisson: any target that is not finite) gives NaN.  Poisson: the target is read at k = floor(y), F = 0 for k < 0, and a non-finite rate or one
// above 2^30 among the networks that count gives NaN.  Negative binomial (disp = r, the dispersion; not read otherwise): as Poisson with
// F(k) = sum_i w_i / W I_{q_i}(r, k + 1), q_i = sigmoid(log r - f_i); its ceilings are 2^20 on the rate AND on k = floor(y): beyond either
// the element is NaN (ENS_NB_MAX).  Gamma (TBNN_LIK_GAMMA; disp = the shape a): F(y) = sum_i w_i / W P(a, a y exp(-f_i)) by ens_gamma_p,
// F = 0 for y <= 0; NaN for a NaN target and, among the networks that count, a NaN f_i or a mean exp(f_i) that is 0 or not finite (a
// network of weight 0 is not looked at, whatever it holds).  Weibull (TBNN_LIK_WEIBULL; disp = the shape k): the target is read at
// t = |y| (its sign is the censoring flag, which the caller knows: on a censored row the PIT lies in [F, 1]),
// F(t) = sum_i w_i / W (-expm1(-u_i)), u_i = exp(k (log t - f_i)), F = 0 for t = 0; Gamma's NaN rules, the scale exp(f_i) for the mean.
template <int LIK>
__global__ __launch_bounds__(ENS_TB) void k_ens_pred_cdf(const float* __restrict__ t, int m, long tot, long r, int d_out, const float* __restrict__ Y,
                                                          const double* __restrict__ cst, double* __restrict__ cdf, double* __restrict__ below,
                                                          double disp) {
#pragma clang fp contract(off)
    constexpr bool COUNTS = LIK == TBNN_LIK_POISSON || LIK == TBNN_LIK_NEG_BINOMIAL;
    constexpr bool HET = LIK == TBNN_LIK_HETERO_GAUSSIAN;
    const long ns = HET ? 2 * tot : tot;                  // floats between two networks' predictions of an element
    const double lr = LIK == TBNN_LIK_NEG_BINOMIAL ? log(disp) : 0.0;
    for (long e = (long)blockIdx.x * ENS_TB + threadIdx.x; e < tot; e += (long)gridDim.x * ENS_TB) {
        const float* __restrict__ te = t + e;
        const float yf = Y[(size_t)(e % r) * d_out + e / r];
        const double y = (double)yf, k = floor(y);
        int bad = COUNTS ? !(fabsf(yf) < INFINITY) : yf != yf;
        if (LIK == TBNN_LIK_NEG_BINOMIAL) bad += k > ENS_NB_MAX;
        double F = 0.0, Fb = 0.0;
        for (int i = 0; i < m; ++i) {
            const float fv = te[(size_t)i * ns];
            const double wn = cst[i];
            if (HET) {
                if (!(wn > 0.0)) continue;                  // (a network of weight 0 adds nothing, whatever it holds)
                const float gv = te[(size_t)i * ns + tot];
                bad += (fv != fv) + (gv != gv);
                F += wn * ens_phi(y, (double)fv, exp(-ens_het_gc(gv)) * 0.70710678118654752440);
                continue;
            }
            if (LIK != TBNN_LIK_GAMMA && LIK != TBNN_LIK_WEIBULL) bad += fv != fv;        // (Gamma, Weibull: a network of weight 0 is not looked at; a NaN that counts: below)
            if (!(wn > 0.0)) continue;
            if (LIK == TBNN_LIK_POISSON) {
                const double lam = exp((double)fv);
                if (!(lam <= ENS_POIS_MAX_RATE)) { bad += 1; continue; }
                if (k >= 0.0) F += wn * ens_gamma_q(k + 1.0, lam);
                if (below && k >= 1.0) Fb += wn * ens_gamma_q(k, lam);
            } else if (LIK == TBNN_LIK_GAMMA) {
                const double mu = exp((double)fv);
                if (!(mu > 0.0 && mu < (double)INFINITY)) { bad += 1; continue; }       // (the mean 0 or not finite; a NaN f_i too)
                if (y > 0.0) F += wn * ens_gamma_p(disp, (disp * y) * exp(-(double)fv));
            } else if (LIK == TBNN_LIK_WEIBULL) {
                const double lam = exp((double)fv);
                if (!(lam > 0.0 && lam < (double)INFINITY)) { bad += 1; continue; }     // (the scale 0 or not finite; a NaN f_i too)
                if (fabs(y) > 0.0) F += wn * -expm1(-exp(disp * (log(fabs(y)) - (double)fv)));
            } else if (LIK == TBNN_LIK_NEG_BINOMIAL) {
                const double lam = exp((double)fv);
                if (!(lam <= ENS_NB_MAX)) { bad += 1; continue; }
                if (bad) continue;                                                      // (a count past the ceiling: nothing is summed)
                double q, p;
                ens_nb_qp(lr, (double)fv, q, p);
                if (k >= 0.0) F += wn * ens_betainc(disp, k + 1.0, q, p);
                if (below && k >= 1.0) Fb += wn * ens_betainc(disp, k, q, p);
            } else {
                F += wn * ens_phi(y, (double)fv, cst[m + i]);
            }
        }
        cdf[e] = bad ? (double)NAN : F;
        if (below) below[e] = bad ? (double)NAN : Fb;
    }
}

// Quantiles of the same mixtures.  cst[3][m]: w_i / W, 1 / (s_i sqrt 2), s_i (Gaussian kinds; Poisson reads the first row only);
// probs[2][np]: p and, Gaussian kinds, z_p = Phi^-1(p) from the host; smax: the largest s_i that counts; res[np][tot].  A thread owns its
// element and carries QP probabilities' search states; every trial is one pass over the element's m predictions (stride tot, coalesced;
// the constants are uniform), shared by the slots still searching, and the thread leaves when all are done.
//   Gaussian  bracket [min_i, max_i] of f_i + s_i z_p (each component's own p-quantile: F <= p at the lower end and >= p at the upper),
//             widened by 2^-44 (max(|a|, |b|) + smax), then VERIFIED: an end whose F is on the wrong side becomes the other end and is pushed
//             out by twice the width, up to 16 times.  From there F(a) < p <= F(b) as evaluated.  Trial: the Newton step from the last
//             point (F' = sum_i w_i / W c_i exp(-z_i^2) / sqrt pi), carried 2^-20 of its length and 2 ulp further so that converged steps land
//             across the root and the OTHER end closes in too; the midpoint instead when that leaves the bracket or is more than half
//             as long as the last move (the moves then shrink at least as a bisection's: Numerical Recipes' rtsafe).  Ends at F(x) == p or a bracket of at most 2 ulp64; the result is the upper end b.
//   Poisson   the smallest integer k >= 0 with F(k) >= p, F(k) = sum_i w_i / W Q(k + 1, exp(f_i)): from k = floor(mean rate) outward in steps
//             that double, starting at floor(sqrt(mean rate)) + 1 (F(-1) = 0 < p is known), until bracketed; then bisection.
// An element with a NaN among its f_i gives NaN at every probability; so does, among the networks that count, an infinite f_i (Gaussian: the
// bracket is unbounded) or a rate that is not finite or above 2^30 (Poisson).
//   neg. binomial (disp = r; not read otherwise) Poisson's slots with F(k) = sum_i w_i / W I_{q_i}(r, k + 1): from k = floor(mean rate), the first
//             step floor(sqrt(mean + mean^2 / r)) + 1.  No trial goes past k = 2^20 (ENS_NB_MAX): a probability whose F(2^20) is still below it
//             gives NaN, and so does a rate that is not finite or above 2^20 among the networks that count.
//   Gamma     (disp = the shape a) the Gaussian scheme on the positive axis: probs[np + j] holds g_p / a, g_p the p-quantile of the standard
//             Gamma(a, 1) from the host, so exp(f_i) g_p / a is component i's own p-quantile and [min_i, max_i] of those the bracket; it is
//             widened by the FACTOR 1 + 2^-44 at each end and verified with multiplicative pushes (an end on the wrong side becomes the other
//             end and moves out by the square of the ends' ratio, up to 16 times), so no end reaches 0.  Then the same safeguarded Newton
//             search in y, its slope the mixture density sum_i w_i / W (a / mu_i) x_i^(a - 1) e^-x_i / Gamma(a), x_i = a y / mu_i, formed in
//             logs (infinite at 0 for a < 1: the step is then refused for the midpoint); the same stopping rule, the result the upper end.
//             NaN: a NaN f_i, or a mean exp(f_i) that is 0 or not finite among the networks that count.
//   Weibull   (disp = the shape k) Gamma's scheme: probs[np + j] holds g_p = (-log1p(-p))^(1/k) from the host, so exp(f_i) g_p is component
//             i's own p-quantile; the same multiplicative bracket, verification and safeguarded Newton search, with the closed forms
//             F_i(y) = -expm1(-u_i) and F_i'(y) = (k / y) exp(z_i - u_i), z_i = k (log y - f_i), u_i = exp(z_i); the same stopping rule, the upper end.
template <int LIK, int QP>
__global__ __launch_bounds__(ENS_TB) void k_ens_pred_quantiles(const float* __restrict__ t, int m, long tot, const double* __restrict__ cst,
                                                                const double* __restrict__ probs, int np, double smax, double* __restrict__ res,
                                                                double disp) {
#pragma clang fp contract(off)
    constexpr bool NEGB = LIK == TBNN_LIK_NEG_BINOMIAL;
    constexpr bool HET = LIK == TBNN_LIK_HETERO_GAUSSIAN;          // (a Gaussian kind below: the same bracket, search and stopping rule)
    constexpr bool WEI = LIK == TBNN_LIK_WEIBULL;
    constexpr bool GAM = LIK == TBNN_LIK_GAMMA || WEI;          // (the kinds on the positive axis: multiplicative bracket and pushes)
    const bool gauss = LIK != TBNN_LIK_POISSON && !NEGB;      // (the continuous kinds: the Gaussian ones, Gamma and Weibull)
    const double lga = GAM && !WEI ? lgamma(disp) : 0.0;
    const long ns = HET ? 2 * tot : tot;                  // floats between two networks' predictions of an element
    const double lr = NEGB ? log(disp) : 0.0;
    for (long e = (long)blockIdx.x * ENS_TB + threadIdx.x; e < tot; e += (long)gridDim.x * ENS_TB) {
        const float* __restrict__ te = t + e;
        for (int p0 = 0; p0 < np; p0 += QP) {
            // a, b: Gaussian the bracket's ends; Poisson the largest k known with F < p and the smallest with F >= p (or +inf: none yet).
            // x: the trial; wd: Gaussian the bracket's width while it is verified, then the length of the last move; Poisson the next step outward
            double pj[QP], a[QP], b[QP], x[QP], wd[QP];
            int ph[QP];                                // Gaussian: 0 verifying a, 1 verifying b, 2 searching; + 8 per push outward.  -1: done
            int bad = 0;
            double mean = 0.0;
            double smx = HET ? 0.0 : smax;                 // the widening's scale: HET the element's own largest s_i that counts
#pragma unroll
            for (int j = 0; j < QP; ++j) {
                pj[j] = probs[min(p0 + j, np - 1)];
                a[j] = gauss ? (double)INFINITY : -1.0; b[j] = gauss ? -(double)INFINITY : (double)INFINITY;
                ph[j] = p0 + j < np ? 0 : -1;              // (a slot past the last is never evaluated)
            }
            for (int i = 0; i < m; ++i) {
                const float fv = te[(size_t)i * ns];
                const double wn = cst[i];
                if (!HET && !GAM) bad += fv != fv;
                float gv = 0.f;
                if (HET && wn > 0.0) { gv = te[(size_t)i * ns + tot]; bad += (fv != fv) + (gv != gv); }      // (weight 0: not looked at)
                if (!(wn > 0.0)) continue;
                if (GAM) {
                    const double mu = exp((double)fv);
                    bad += !(mu > 0.0 && mu < (double)INFINITY);           // (a NaN f_i too; a network of weight 0 is not looked at)
#pragma unroll
                    for (int j = 0; j < QP; ++j) {
                        const double v = mu * probs[np + min(p0 + j, np - 1)];
                        a[j] = fmin(a[j], v); b[j] = fmax(b[j], v);
                    }
                } else if (gauss) {
                    bad += fabsf(fv) == INFINITY;
                    const double s = HET ? exp(ens_het_gc(gv)) : cst[2 * m + i];
                    if (HET) smx = fmax(smx, s);
#pragma unroll
                    for (int j = 0; j < QP; ++j) {
                        const double v = fma(s, probs[np + min(p0 + j, np - 1)], (double)fv);
                        a[j] = fmin(a[j], v); b[j] = fmax(b[j], v);
                    }
                } else {
                    const double lam = exp((double)fv);
                    if (!(lam <= (NEGB ? ENS_NB_MAX : ENS_POIS_MAX_RATE))) bad += 1;
                    mean += wn * lam;
                }
            }
#pragma unroll
            for (int j = 0; j < QP; ++j) {
                if (GAM) {
                    a[j] *= 1.0 - 0x1p-44; b[j] *= 1.0 + 0x1p-44;
                    x[j] = a[j]; wd[j] = b[j] / a[j];                                   // (while verifying: the ends' ratio)
                } else if (gauss) {
                    const double d = 0x1p-44 * (fmax(fabs(a[j]), fabs(b[j])) + smx);
                    a[j] -= d; b[j] += d;
                    x[j] = a[j]; wd[j] = b[j] - a[j];
                } else {
                    x[j] = floor(mean); wd[j] = floor(sqrt(NEGB ? mean + mean * mean / disp : mean)) + 1.0;
                }
            }
            for (int pass = 0; pass < ENS_PRED_PASSES && !bad; ++pass) {
                bool live = false;
#pragma unroll
                for (int j = 0; j < QP; ++j) live = live || ph[j] >= 0;
                if (!live) break;
                double F[QP], D[QP];
#pragma unroll
                for (int j = 0; j < QP; ++j) { F[j] = 0.0; D[j] = 0.0; }
                for (int i = 0; i < m; ++i) {
                    const double wn = cst[i];
                    if (!(wn > 0.0)) continue;
                    const double f = (double)te[(size_t)i * ns];
                    if (WEI) {
#pragma unroll
                        for (int j = 0; j < QP; ++j) {
                            if (ph[j] >= 0) {
                                // (the density's u e^-u as exp(z - u), z = log u: a far-off network, u = inf, adds 0 -- not inf * 0 -- and
                                // the Newton step of the others stays alive)
                                const double z = disp * (log(x[j]) - f), u = exp(z);
                                F[j] += wn * -expm1(-u);
                                D[j] += wn * ((disp / x[j]) * exp(z - u));
                            }
                        }
                    } else if (GAM) {
                        const double am = disp * exp(-f);                                   // a / mu_i
#pragma unroll
                        for (int j = 0; j < QP; ++j) {
                            if (ph[j] >= 0) {
                                const double xi = x[j] * am;
                                F[j] += wn * ens_gamma_p(disp, xi);
                                D[j] += wn * (am * exp((disp - 1.0) * log(xi) - xi - lga));
                            }
                        }
                    } else if (gauss) {
                        const double c = HET ? exp(-ens_het_gc(te[(size_t)i * ns + tot])) * 0.70710678118654752440 : cst[m + i], wc = wn * c;
#pragma unroll
                        for (int j = 0; j < QP; ++j) {
                            if (ph[j] >= 0) {
                                const double z = (x[j] - f) * c;
                                F[j] += wn * (0.5 * erfc(-z));
                                D[j] += wc * exp(-(z * z));
                            }
                        }
                    } else if (NEGB) {
                        double q, p;
                        ens_nb_qp(lr, f, q, p);
#pragma unroll
                        for (int j = 0; j < QP; ++j)
                            if (ph[j] >= 0) F[j] += wn * ens_betainc(disp, x[j] + 1.0, q, p);
                    } else {
                        const double lam = exp(f);
#pragma unroll
                        for (int j = 0; j < QP; ++j)
                            if (ph[j] >= 0) F[j] += wn * ens_gamma_q(x[j] + 1.0, lam);
                    }
                }
#pragma unroll
                for (int j = 0; j < QP; ++j) {
                    if (ph[j] < 0) continue;
                    const double p = pj[j];
                    if (!gauss) {
                        if (F[j] >= p) b[j] = x[j]; else a[j] = x[j];
                        if (b[j] == (double)INFINITY) {                                       // still below: outward, unless the count is absurd
                            if (NEGB && a[j] >= ENS_NB_MAX) { b[j] = (double)NAN; ph[j] = -1; continue; }      // (F at the ceiling is below p)
                            if (a[j] > 0x1p40) { b[j] = a[j]; ph[j] = -1; continue; }
                            x[j] = a[j] + wd[j]; wd[j] *= 2.0;
                            if (NEGB) x[j] = fmin(x[j], ENS_NB_MAX);
                        } else if (ph[j] == 0 && a[j] < 0.0 && b[j] - wd[j] > 0.0) {           // above, and nothing below it tried yet: outward and down
                            x[j] = b[j] - wd[j]; wd[j] *= 2.0;
                        } else {
                            ph[j] = 1;
                            if (b[j] - a[j] <= 1.0) { ph[j] = -1; continue; }
                            x[j] = a[j] + floor(0.5 * (b[j] - a[j]));
                        }
                        continue;
                    }
                    const int stage = ph[j] & 7, pushes = ph[j] >> 3;
                    if (stage == 0) {                                                       // x == a: F(a) < p wanted
                        if (F[j] < p || pushes >= 16) { ph[j] = 1; x[j] = b[j]; }
                        else if (GAM) { b[j] = a[j]; a[j] /= wd[j] * wd[j]; wd[j] = b[j] / a[j]; x[j] = a[j]; ph[j] += 8; }
                        else { b[j] = a[j]; a[j] -= 2.0 * wd[j]; wd[j] = b[j] - a[j]; x[j] = a[j]; ph[j] += 8; }
                        continue;
                    }
                    if (stage == 1) {                                                       // x == b: F(b) >= p wanted
                        if (GAM && !(F[j] >= p) && pushes < 16) { a[j] = b[j]; b[j] *= wd[j] * wd[j]; wd[j] = b[j] / a[j]; x[j] = b[j]; ph[j] += 8; continue; }
                        if (!(F[j] >= p) && pushes < 16) { a[j] = b[j]; b[j] += 2.0 * wd[j]; wd[j] = b[j] - a[j]; x[j] = b[j]; ph[j] += 8; continue; }
                        ph[j] = 2;
                        wd[j] = 4.0 * (b[j] - a[j]);                                        // (the first trial may be a Newton step)
                    } else if (F[j] >= p) b[j] = x[j];
                    else a[j] = x[j];
                    const double w = b[j] - a[j];
                    if (F[j] == p || !(w > 2.0 * ens_ulp64(b[j]))) { ph[j] = -1; continue; }
                    // F' = D / sqrt pi (Gamma, Weibull: D itself)
                    const double step = (p - F[j]) * (GAM ? 1.0 : 1.7724538509055160273) / D[j];
                    const double xn = x[j] + step + (0x1p-20 * step + copysign(2.0 * ens_ulp64(x[j]), step));
                    const bool newton = xn > a[j] && xn < b[j] && fabs(xn - x[j]) <= 0.5 * wd[j];
                    const double xt = newton ? xn : a[j] + 0.5 * w;
                    wd[j] = fabs(xt - x[j]);
                    x[j] = xt;
                }
            }
#pragma unroll
            for (int j = 0; j < QP; ++j)
                if (p0 + j < np) res[(size_t)(p0 + j) * tot + e] = bad ? (double)NAN : b[j];
        }
    }
}

// ---- Pareto-smoothed leave-one-out cross-validation and WAIC ----
// out: the block [m][d_out][r] of untransformed predictions; Y: the block's targets [r][d_out]; sig / cst: the m sigmas and constants of
// k_ens_loglik (Gaussian kinds; else null).  L[m][r] = l_i of every row, by ens_row_loglik: the bits k_ens_loglik sums.  lppd[r] (or null) =
// logsumexp_i l_i - log m, by the steps and in the order of k_ens_loglik / k_ens_lppd_finish: the same bits; pwaic[r] (or null) = the
// centred sum of squares of the row's l_i over m - 1, the l_i read back from L.  A row with an l_i that is not finite gives NaN in both.
__global__ __launch_bounds__(ENS_TB) void k_ens_pointwise(const float* __restrict__ out, int m, long r, int d_out, int lik, const float* __restrict__ Y,
                                                           const float* __restrict__ sig, const double* __restrict__ cst, double logm,
                                                           double* L, double* __restrict__ lppd, double* __restrict__ pwaic, double nu) {
#pragma clang fp contract(off)
    const long tot = r * d_out;
    for (long row = (long)blockIdx.x * ENS_TB + threadIdx.x; row < r; row += (long)gridDim.x * ENS_TB) {
        double Mx = -INFINITY, S = 0.0, sum = 0.0;
        int bad = 0;
        for (int i = 0; i < m; ++i) {
            const double l = ens_row_loglik(lik, out + (size_t)i * tot + row, r, Y + (size_t)row * d_out, d_out, sig ? sig[i] : 1.f, cst ? cst[i] : 0.0, nu);
            L[(size_t)i * r + row] = l;
            bad += !(fabs(l) < INFINITY);
            ens_lse_step(l, Mx, S);
            sum += l;
        }
        if (lppd) lppd[row] = bad ? (double)NAN : Mx + log(S) - logm;
        if (pwaic) {
            const double mean = sum / (double)m;
            double ss = 0.0;
#pragma unroll 4
            for (int i = 0; i < m; ++i) {
                const double d = L[(size_t)i * r + row] - mean;
                ss += d * d;
            }
            pwaic[row] = bad ? (double)NAN : ss / (double)(m - 1);
        }
    }
}

// the order-preserving key of an fp64 value (ens_key's rule)
__device__ __forceinline__ unsigned long long ens_key64(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b ^ ((b >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}
__device__ __forceinline__ double ens_unkey64(unsigned long long k) {
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : 0xFFFFFFFFFFFFFFFFull)));
}

// the raw log ratio x_i = -l_i - max_j(-l_j); adding 0 turns a -0 into +0, so that equal values have equal keys
__device__ __forceinline__ double ens_psis_x(double l, double mx) {
#pragma clang fp contract(off)
    return (-l - mx) + 0.0;
}

// L: the block's matrix [m][r]; M, G, q: the tail length, the number of candidates and the quartile index of tbnn_ensemble_loo, from the
// host; ta, tb: scratch [M][r] each; elpd, pk: [r].  A thread owns its row (the result does not depend on the grid) and walks, all in fp64:
//   maximum   mx = max_i(-l_i), and the check that every l_i is finite (else NaN, NaN)
//   cutoff    c = v_(m-M), the smallest key K with count(key(x_i) <= K) >= m - M, its 64 bits fixed from the top as k_ens_quantiles fixes 32
//   tail      the x_i > c and, of those equal to c, the last M - count(x_i > c) in network order (the members a stable sort puts last; the
//             values are what counts), written to ta in network order; their rank among the M -- the count of smaller values, and of equal
//             ones earlier in ta -- goes to tb, then y_j = exp(x_j) - exp(c) over x_j in ta.  M^2 comparisons: below the fit's M G log1p up
//             to M of a few thousand
//   fit       one sweep over g = 1 .. G: the weights exp(L_g - logsumexp L) and b = sum_g b_g w_g are carried as a running maximum of L_g
//             and the two sums S = sum exp(L_g - max), B = sum b_g exp(L_g - max), rescaled when the maximum moves; b = B / S.  No L_g is
//             kept and none recomputed
//   closing   a second walk over the networks finds the tail's members by the same rule and gives each the quantile of its rank; the two
//             log-sum-exps run in network order
// No per-thread array: ta and tb are read at stride r (coalesced: the lanes of a wave ask for the same j).
__global__ __launch_bounds__(ENS_TB) void k_ens_psis(const double* __restrict__ L, int m, long r, int M, int G, int q, double* ta, double* tb,
                                                      double* __restrict__ elpd, double* __restrict__ pk) {
#pragma clang fp contract(off)
    const double dM = (double)M, dG = (double)G;
    for (long row = (long)blockIdx.x * ENS_TB + threadIdx.x; row < r; row += (long)gridDim.x * ENS_TB) {
        const double* __restrict__ Lr = L + row;
        double* A = ta + row;
        double* B = tb + row;
        double mx = -INFINITY;
        int bad = 0;
#pragma unroll 4
        for (int i = 0; i < m; ++i) {
            const double l = Lr[(size_t)i * r];
            bad += !(fabs(l) < INFINITY);
            mx = fmax(mx, -l);
        }
        if (bad) {
            if (elpd) elpd[row] = (double)NAN;
            if (pk) pk[row] = (double)NAN;
            continue;
        }
        const int need = m - M;
        unsigned long long K = 0ull;
        for (int bit = 63; bit >= 0; --bit) {
            const unsigned long long trial = K | ((1ull << bit) - 1ull);
            int cnt = 0;
#pragma unroll 8
            for (int i = 0; i < m; ++i) cnt += ens_key64(ens_psis_x(Lr[(size_t)i * r], mx)) <= trial;
            if (cnt < need) K |= 1ull << bit;
        }
        const double c = ens_unkey64(K);
        int above = 0, ties = 0;
#pragma unroll 4
        for (int i = 0; i < m; ++i) {
            const double x = ens_psis_x(Lr[(size_t)i * r], mx);
            above += x > c;
            ties += x == c;
        }
        const int first_tie = ties - (M - above);          // ties before this one (network order) stay below the tail
        int pos = 0, seen = 0;
        double tmin = 0.0;
        for (int i = 0; i < m; ++i) {
            const double x = ens_psis_x(Lr[(size_t)i * r], mx);
            bool in = x > c;
            if (x == c) { in = seen >= first_tie; ++seen; }
            if (in && pos < M) { A[(size_t)pos * r] = x; tmin = fmin(tmin, x); ++pos; }
        }
        double kk = (double)INFINITY, sigma = 0.0, ec = 0.0;
        bool smooth = M >= 5 && pos == M && tmin < 0.0;         // (the largest x is 0 and is in the tail: the range is -tmin)
        if (smooth) {
            for (int j = 0; j < M; ++j) {
                const double xj = A[(size_t)j * r];
                int cnt = 0;
#pragma unroll 8
                for (int jj = 0; jj < M; ++jj) {
                    const double v = A[(size_t)jj * r];
                    cnt += (v < xj) || (v == xj && jj < j);
                }
                B[(size_t)j * r] = (double)cnt;
            }
            ec = exp(c);
            double yq = 0.0, yM = 0.0;
            for (int j = 0; j < M; ++j) {
                const double y = exp(A[(size_t)j * r]) - ec;
                if ((int)B[(size_t)j * r] == q - 1) yq = y;
                yM = fmax(yM, y);
                A[(size_t)j * r] = y;
            }
            smooth = yq > 0.0;
            if (smooth) {
                double Lmax = -INFINITY, S = 0.0, Bs = 0.0;
                for (int g = 1; g <= G; ++g) {
                    const double b = 1.0 / yM + (1.0 - sqrt(dG / ((double)g - 0.5))) / (3.0 * yq);
                    double ks = 0.0;
#pragma unroll 4
                    for (int j = 0; j < M; ++j) ks += log1p(-b * A[(size_t)j * r]);
                    const double kap = ks / dM;
                    const double Lg = dM * (log(-b / kap) - kap - 1.0);
                    if (Lg > Lmax) {
                        const double e = exp(Lmax - Lg);
                        S = S * e + 1.0; Bs = Bs * e + b; Lmax = Lg;
                    } else {
                        const double e = exp(Lg - Lmax);            // (a NaN L_g reaches b, and k with it)
                        S += e; Bs += b * e;
                    }
                }
                const double b = Bs / S;
                double ks = 0.0;
#pragma unroll 4
                for (int j = 0; j < M; ++j) ks += log1p(-b * A[(size_t)j * r]);
                const double kap = ks / dM;
                sigma = -kap / b;
                kk = (dM * kap + 5.0) / (dM + 10.0);
                smooth = fabs(kk) < INFINITY && fabs(sigma) < INFINITY;      // else the raw ratios, and the k obtained
            }
        }
        if (pk) pk[row] = kk;
        if (!elpd) continue;
        double M1 = -INFINITY, S1 = 0.0, M2 = -INFINITY, S2 = 0.0;
        pos = 0; seen = 0;
        for (int i = 0; i < m; ++i) {
            const double l = Lr[(size_t)i * r];
            const double x = ens_psis_x(l, mx);
            bool in = x > c;
            if (x == c) { in = seen >= first_tie; ++seen; }
            double lw = x;
            if (in && pos < M) {
                if (smooth) {
                    const double z = log1p(-((B[(size_t)pos * r] + 0.5) / dM));
                    const double qv = fabs(kk) < 0x1p-52 ? -sigma * z : sigma * expm1(-kk * z) / kk;
                    lw = fmin(log(ec + qv), 0.0);
                }
                ++pos;
            }
            ens_lse_step(lw + l, M1, S1);
            ens_lse_step(lw, M2, S2);
        }
        elpd[row] = (M1 + log(S1)) - (M2 + log(S2));
    }
}

// ---- the continuous ranked probability score of the predictive mixture (tbnn_ensemble_crps) ----
// compensated (Kahan) accumulation: s + the running sum of what the additions lost; the sums below are of terms >= 0
__device__ __forceinline__ void ens_kahan(double a, double& s, double& c) {
#pragma clang fp contract(off)
    const double y = a - c;
    const double t = s + y;
    c = (t - s) - y;
    s = t;
}

// A(mu, sigma) = E|N(mu, sigma^2)| = sigma [2 phi(z) + z erf(z / sqrt 2)], z = |mu| / sigma, sigma > 0: both terms >= 0
__device__ __forceinline__ double ens_abs_normal(double mu, double sigma) {
#pragma clang fp contract(off)
    const double z = fabs(mu) / sigma;
    return sigma * (0.79788456080286535588 * exp(-0.5 * (z * z)) + z * erf(z * 0.70710678118654752440));
}

// t: the block [m][tot] of untransformed predictions (TBNN_LIK_HETERO_GAUSSIAN: [m][2][tot], tot = r, as k_ens_pred_cdf reads it); Y: the
// block's targets [r][d_out]; cst[2][m]: w_i / W and, Gaussian kinds with NOISE, s_i.  res[3][rbk]: crps, error, spread of the block's
// tot elements.  NOISE false: A(mu, 0) = |mu|, no scale is read (heteroscedastic kind: the mean plane alone).
//
// Layout.  A workgroup owns ENS_CE = 32 consecutive elements at a time, thread tid the element el = tid % 32 as lane g = tid / 32 of its
// ENS_CL = 8.  The networks are cut into tiles of ENS_CT = 8.  For tile I, lane g keeps network i = 8 I + g of its element in REGISTERS
// (f_i, s_i, w_i / W) and adds the element's error term of that network; then the tiles J = 0 .. I pass through LDS one after the other,
// [8][32] doubles of f_j (heteroscedastic kind: and of s_j = exp(gc_j)), every thread staging the one value (network 8 J + g, element el)
// -- its 32 neighbours read 128 contiguous bytes -- so a prediction comes from memory once per tile pass and is read eight times from LDS.
// The tile is double-buffered: the value of tile J + 1 is loaded before tile J is walked and written after, one barrier per tile pair.
// A wave reads f_j of ONE j for its 32 elements: 32 consecutive doubles, one bank row, the two half-waves (two values of g) the same
// addresses -- no bank conflict.  Lane g walks j = 8 J .. 8 J + 7 (J < I), j = 8 I .. i on the diagonal tile (NOISE false: .. i - 1, the
// diagonal term is 0), skipping networks of weight 0, which are never looked at in the pair walk.  w_j / W and the Gaussian kinds' s_j
// are read from cst at an index the whole wave shares.
// Sums, all compensated (ens_kahan), in this order: a lane's error sum over its networks i = g, g + 8, ... ascending; a lane's spread sum
// over I ascending, J ascending, j ascending, of (w_i / W)(w_j / W) A(f_i - f_j, sqrt(s_i^2 + s_j^2)), the diagonal term (j = i) at half
// weight; then, through LDS, the element's eight lanes g = 0 .. 7 in order.  crps = error - spread.  Nothing depends on the element's
// place in its workgroup, the grid or the block: the same bits from run to run and whatever the row blocks.
// NaN (all three results): a NaN target; Gaussian kinds: a NaN f_i under any network; heteroscedastic kind: a NaN f_i or (NOISE) g_i of a
// network that counts; an infinite f_i of a network that counts.
template <int LIK, bool NOISE>
__global__ __launch_bounds__(ENS_TB) void k_ens_crps(const float* __restrict__ t, int m, long tot, long r, int d_out, const float* __restrict__ Y,
                                                      const double* __restrict__ cst, double* __restrict__ res, long rbk) {
#pragma clang fp contract(off)
    static_assert(ENS_CL == ENS_CT && ENS_CT * ENS_CE == ENS_TB, "one staged value per thread and tile, one network of a tile per lane");
    constexpr bool HET = LIK == TBNN_LIK_HETERO_GAUSSIAN;
    __shared__ double fJ[2][ENS_CT][ENS_CE];
    __shared__ double sJ[HET && NOISE ? 2 : 1][ENS_CT][ENS_CE];
    __shared__ double red[2][ENS_CL][ENS_CE];
    __shared__ int redbad[ENS_CL][ENS_CE];
    const int el = threadIdx.x % ENS_CE, g = threadIdx.x / ENS_CE;
    const long ns = HET ? 2 * tot : tot;                  // floats between two networks' predictions of an element
    const int nt = (m + ENS_CT - 1) / ENS_CT;
    int b = 0;
    for (long e0 = (long)blockIdx.x * ENS_CE; e0 < tot; e0 += (long)gridDim.x * ENS_CE) {
        const long e = e0 + el;
        const bool live = e < tot;
        const float yf = live ? Y[(size_t)(e % r) * d_out + e / r] : 0.f;
        const double y = (double)yf;
        int bad = yf != yf;
        double es = 0.0, ec = 0.0, ss = 0.0, sc = 0.0;
        for (int I = 0; I < nt; ++I) {
            // this lane's network of tile I; it is also the value this thread stages when J reaches I
            const int i = I * ENS_CT + g;
            const bool have = live && i < m;
            const double wi = have ? cst[i] : 0.0;
            double fi = 0.0, si = 1.0;
            if (have) {
                const float fv = t[(size_t)i * ns + e];
                fi = (double)fv;
                if (!HET) bad += fv != fv;
                if (NOISE && !HET) si = cst[(size_t)m + i];
                if (wi > 0.0) {
                    if (HET && NOISE) {
                        const float gv = t[(size_t)i * ns + tot + e];
                        si = exp(ens_het_gc(gv));
                        bad += gv != gv;
                    }
                    bad += (fv != fv) + (fabsf(fv) == INFINITY);
                    ens_kahan(wi * (NOISE ? ens_abs_normal(y - fi, si) : fabs(y - fi)), es, ec);
                }
            }
            // the staged value of tile J = 0: network g
            double pf = 0.0, ps = 1.0;
            if (live && g < m) {
                pf = (double)t[(size_t)g * ns + e];
                if (HET && NOISE) ps = exp(ens_het_gc(t[(size_t)g * ns + tot + e]));
            }
            for (int J = 0; J <= I; ++J) {
                fJ[b][g][el] = pf;
                if (HET && NOISE) sJ[b][g][el] = ps;
                __syncthreads();
                const int jn = J + 1 <= I ? (J + 1) * ENS_CT + g : m;         // the next tile's network of this thread, loaded under the walk
                float nf = 0.f, ng = 0.f;
                if (live && jn < m) {
                    nf = t[(size_t)jn * ns + e];
                    if (HET && NOISE) ng = t[(size_t)jn * ns + tot + e];
                }
                if (have && wi > 0.0) {
                    const int j0 = J * ENS_CT;
                    const int last = J < I ? min(ENS_CT, m - j0) - 1 : (NOISE ? g : g - 1);
                    const double vi = si * si;
                    for (int jl = 0; jl <= last; ++jl) {
                        const double wj = cst[j0 + jl];
                        if (!(wj > 0.0)) continue;
                        const double mu = fi - fJ[b][jl][el];
                        double a;
                        if (NOISE) {
                            const double sj = HET ? sJ[b][jl][el] : cst[(size_t)m + j0 + jl];
                            a = ens_abs_normal(mu, sqrt(vi + sj * sj));
                        } else {
                            a = fabs(mu);
                        }
                        const double wij = wi * wj;
                        ens_kahan((J == I && jl == g ? 0.5 * wij : wij) * a, ss, sc);
                    }
                }
                pf = (double)nf;
                if (HET && NOISE) ps = exp(ens_het_gc(ng));
                b ^= 1;
            }
        }
        red[0][g][el] = es; red[1][g][el] = ss; redbad[g][el] = bad;
        __syncthreads();
        if (g == 0 && live) {
            double E = 0.0, Ec = 0.0, S = 0.0, Sc = 0.0;
            int anybad = 0;
#pragma unroll
            for (int l = 0; l < ENS_CL; ++l) {
                ens_kahan(red[0][l][el], E, Ec);
                ens_kahan(red[1][l][el], S, Sc);
                anybad += redbad[l][el];
            }
            res[e] = anybad ? (double)NAN : E - S;
            res[rbk + e] = anybad ? (double)NAN : E;
            res[2 * rbk + e] = anybad ? (double)NAN : S;
        }
    }
}
