// Shared device/host definitions for libtbnn (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tbnn.h"

// a fused kernel's hidden activations as ONE int: a TBNN_ACT_* value (every hidden layer the same), or this flag + 3 bits per hidden layer
// (kernels_fast.hpp: Shape::act; fused_ops.hpp)
#define TBNN_ACT_PACKED 0x40000000

// the likelihood a fused kernel was instantiated for (kernels_fast.hpp: Shape::LIK; fused_ops.hpp: FusedOps::lik)
enum { SHAPE_LIK_GAUSS = 0, SHAPE_LIK_BERN = 1, SHAPE_LIK_CAT = 2, SHAPE_LIK_POIS = 3 };
// flag bit of the code: the kernel scales each row's data term by its weight (tbnn_set_row_weights; kernels_fast.hpp: row_weight)
enum { SHAPE_LIK_WEIGHTED = 4 };
// flag bit on the Gaussian family (the low two bits are full): the Student-t data term of TBNN_LIK_STUDENT_T, the residual y - f of the
// Gaussian kinds under another loss (kernels_fast.hpp: lik_delta); weighted: SHAPE_LIK_STUDENT | SHAPE_LIK_WEIGHTED
enum { SHAPE_LIK_STUDENT = 8 };
// the same bit on the Poisson code: the negative-binomial data term of TBNN_LIK_NEG_BINOMIAL, the log-rate f of the Poisson kind under
// another loss; weighted: SHAPE_LIK_POIS | SHAPE_LIK_NEGBIN | SHAPE_LIK_WEIGHTED.  (The bit is not defined on the other two codes.)
enum { SHAPE_LIK_NEGBIN = 8 };
// a further flag bit on the Gaussian code: the heteroscedastic Gaussian of TBNN_LIK_HETERO_GAUSSIAN -- exactly two outputs per row, the mean
// f and the log-sd g, ONE term per row (kernels_fast.hpp: lik_pair); weighted: SHAPE_LIK_HETERO | SHAPE_LIK_WEIGHTED.  (Not defined on the
// other codes, nor together with SHAPE_LIK_STUDENT.)
enum { SHAPE_LIK_HETERO = 16 };
// the same bit on the Poisson code: the Gamma data term of TBNN_LIK_GAMMA, the log-mean f of the Poisson kind under another loss;
// weighted: SHAPE_LIK_POIS | SHAPE_LIK_GAMMA | SHAPE_LIK_WEIGHTED.  (Not defined on the other two codes, nor together with SHAPE_LIK_NEGBIN.)
enum { SHAPE_LIK_GAMMA = 16 };
// bits 8 and 16 TOGETHER on the Poisson code: the Weibull data term of TBNN_LIK_WEIBULL with right-censored targets, the log-scale f under
// a third element-wise loss; weighted: SHAPE_LIK_POIS | SHAPE_LIK_WEIBULL | SHAPE_LIK_WEIGHTED.  (Not defined on the other codes.)
enum { SHAPE_LIK_WEIBULL = 8 | 16 };
// ... of a TBNN_LIK_* value (Gaussian and fixed-sd Gaussian share their kernels: the sd is a run-time argument)
__host__ __device__ constexpr int shape_lik(int lik) {
    return lik == TBNN_LIK_BERNOULLI ? SHAPE_LIK_BERN : lik == TBNN_LIK_CATEGORICAL ? SHAPE_LIK_CAT : lik == TBNN_LIK_POISSON ? SHAPE_LIK_POIS :
           lik == TBNN_LIK_STUDENT_T ? (SHAPE_LIK_STUDENT | SHAPE_LIK_GAUSS) :
           lik == TBNN_LIK_NEG_BINOMIAL ? (SHAPE_LIK_NEGBIN | SHAPE_LIK_POIS) :
           lik == TBNN_LIK_HETERO_GAUSSIAN ? (SHAPE_LIK_HETERO | SHAPE_LIK_GAUSS) :
           lik == TBNN_LIK_GAMMA ? (SHAPE_LIK_GAMMA | SHAPE_LIK_POIS) :
           lik == TBNN_LIK_WEIBULL ? (SHAPE_LIK_WEIBULL | SHAPE_LIK_POIS) : SHAPE_LIK_GAUSS;
}

#define TBNN_WAVE 64
#define PSTAT_CAP 512                     // entries of the per-workgroup statistic buffer (tbnn_api.hip): >= the grid of every fused pass

// Network descriptor passed BY VALUE as a kernel argument (lives in SGPRs /
// the kernarg segment: every lookup is wave-uniform).
struct NetDev {
    int nl;                       // dense layers
    int in[TBNN_MAX_LAYERS];      // inputDims   (layer.py:110)
    int out[TBNN_MAX_LAYERS];     // outputDims  (layer.py:111)
    int act[TBNN_MAX_LAYERS];     // activation following the layer
    int prior[TBNN_MAX_LAYERS];   // TBNN_PRIOR_*
    int offW[TBNN_MAX_LAYERS];    // offset of W_l in theta
    int offB[TBNN_MAX_LAYERS];    // offset of b_l in theta
    int actOff[TBNN_MAX_LAYERS];  // offset (in floats per row) of a_{l+1} in the per-row activation record
    int P, H;
    int lik;                      // TBNN_LIK_*
    int d_in, d_out;
    int sumOut;                   // sum of out dims = floats per row in the activation record
    int maxW;                     // widest layer (in or out)
    float fixed_sd;
    int reserved_flags;           // bit 0: fast kernel processes one tile at a time (diagnostic)
    float lik_df;                 // TBNN_LIK_STUDENT_T: the degrees of freedom nu; TBNN_LIK_NEG_BINOMIAL: the dispersion r; TBNN_LIK_GAMMA: the shape a; TBNN_LIK_WEIBULL: the shape k (0 otherwise)
};

// Gradient-slab stores of the narrow family: WRITE-THROUGH (global_store ... sc1: a relaxed agent-scope atomic store) when the slabs
// are big next to the launch (P >= 2048 parameters x 256 workgroups: configs[1] writes 5.6 MB in a 47-us launch).  A slab is written
// once per launch and read once by the next kernel (k_update).  Left dirty in the L2s it waits for the end of the launch: between two
// kernels this 8-XCD part writes every dirty line back, and that write-back sat on the critical path of every leapfrog step.
// configs[1], bench.py --workload c2: plain stores 18.81 k leapfrog steps/s (fused pass 49.6 us by hipEvent), non-temporal stores
// 19.31 k (47.9 us), write-through 19.72 k (47.1 us).  Small next to long launches (configs[4], the mid-width kernel: 2,788 -> 2,797 steps/s), neutral for small networks (P < 2048:
// plain stores), negative for the layered family's many small dW launches (8 -> 300 -> 300 -> 1: 493 -> 511 us): plain stores there.
template <bool NT>
__device__ __forceinline__ void slab_store(float* ptr, float val) {
    if constexpr (NT) __hip_atomic_store(ptr, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *ptr = val;
}

// 16 bytes of a slab / stored block at once, write-through: one `global_store_dwordx4 ... sc1` (a 4-byte sc1 store is one fabric
// write per lane: ~6x the time per byte of the 16-byte form, MI355X_MICROARCH.md).  The compiler's hazard recognizer does not see
// an inline-asm store as a VMEM store and would not keep a following VALU write off the store-data VGPRs (2 wait states on a
// > 64-bit store): the s_nop inside the statement provides them whatever the register allocation.
typedef float tb_f32x4 __attribute__((ext_vector_type(4)));
template <bool WT>
__device__ __forceinline__ void store16(float* ptr, const tb_f32x4& v) {
    if constexpr (WT) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(ptr), "v"(v) : "memory");
    else *reinterpret_cast<tb_f32x4*>(ptr) = v;
}

// Several chains in one launch (round 4): a handle created with tbnn_create_multi keeps its C chains' buffers as [C][...]
// arrays and launches the per-chain kernels with gridDim.y = C; blockIdx.y picks the chain.  Strides the kernels cannot derive
// from NetDev travel in this struct (all zero for one chain: blockIdx.y is 0 then anyway).
// Per-chain step control of a multi-chain handle whose chains run at their own (eps, L) (tbnn_hmc_step_each; the reference runs one
// adapter per chain, network.py:221-235, :603-607): the chains advance in lockstep for max_c L_c leapfrog steps; chain c takes its
// closing half kick at step L_c and is skipped afterwards -- k_update returns for it and the blocks of the fused pass exit at once, so
// its gradient slab and statistic stay those of ITS last step.
struct StepCtl { float eps; int L; };
__device__ __forceinline__ bool chain_done(const StepCtl* __restrict__ ctl, int t, int chain) { return ctl && t > ctl[chain].L; }
struct ChainStride { long img, eta, slab; const StepCtl* ctl; int t; };

// Per-chain scalar record kept on the device (doubles: energies are summed
// and differenced in fp64 -- strictly more accurate than the reference's fp32).
struct Scal {
    double stat_cur, prior_cur, logp_cur;   // at the current (accepted) state
    double stat_new, prior_new, logp_new;   // at the proposal
    double k0, k1;                          // kinetic energies
    double lar;                             // log accept ratio
    double logu;                            // log U(0,1)
    double d2;                              // |q_prop - q_cur|^2
    double sjd;                             // d2 if accepted else 0
    int accepted;
    int pad;
};

// Likelihood standard deviation used on the hot path.
// Gaussian: clip(eta_last^2, 1e-8, 1e8) (likelihood.py:88 + BNN_functions.py:23-24);
// FixedGaussian: sd as given (likelihood.py:162), same clip inside multivariateLogProb.
// The clip is written once (lik_sigma_clip); lik_sigma_from is lik_sigma for a caller that has loaded the hyper already
// (k_fwd_bwd_fast3 requests it with its first batch of loads; eta_last is not used unless the likelihood has its own noise hyper).
__device__ __forceinline__ float lik_sigma_clip(float s) {
    s = fmaxf(s, 1e-8f);
    s = fminf(s, 1e8f);
    return s;
}
__device__ __forceinline__ float lik_sigma(const NetDev& nd, const float* __restrict__ eta) {
    const float s = (nd.lik == TBNN_LIK_GAUSSIAN) ? eta[nd.H - 1] * eta[nd.H - 1] : nd.fixed_sd;
    return lik_sigma_clip(s);
}
__device__ __forceinline__ float lik_sigma_from(const NetDev& nd, float eta_last) {
    return lik_sigma_clip((nd.lik == TBNN_LIK_GAUSSIAN) ? eta_last * eta_last : nd.fixed_sd);
}

// Student-t (TBNN_LIK_STUDENT_T).  A kernel derives two constants once in its prologue: k = 1 / (nu s^2), which scales the squared residual
// (the fused kernels: in the place of the Gaussian 1 / s^2, lik_inv_var of kernels_fast.hpp), and nu + 1, the factor of the delta.
// log1p(u) for u >= 0 accurate RELATIVE TO ITSELF: the term is multiplied by (nu + 1) / 2 afterwards, and a bare __logf(1 + u) carries
// the rounding of 1 + u, ~6e-8 ABSOLUTE, into a term that may itself be 1e-6 (nu = 1e4: 3e-4 per element after scaling).  Below 1/4 the
// series 2 atanh(z) = 2 z (1 + z^2/3 + z^4/5 + z^6/7), z = u / (2 + u) <= 1/9 (the next term is 3e-9 of the sum); from 1/4 on the hardware
// log2 of 1 + u, whose value is then >= 0.22 and takes the sum's rounding as ~3e-7 of itself.  Both are computed and one selected: no
// branch in the tile body.  u = inf (a residual past the fp32 range) gives inf, NaN gives NaN: the statistic is not finite and k_energy
// rejects the proposal.  No contraction beyond the fmaf written out (here, in student_elem and in lik_delta's branch): which product the
// compiler fuses into which sum (2 + u, z + z, 1 + u of u = r r k) is its choice per instantiation, and a weighted kernel at weight 1 must
// give the unweighted kernel's bits
__device__ __forceinline__ float log1p_fast(float u) {
#pragma clang fp contract(off)
    const float z = u * __builtin_amdgcn_rcpf(2.f + u), z2 = z * z;
    const float ser = (2.f * z) * fmaf(z2, fmaf(z2, fmaf(z2, 1.f / 7.f, 0.2f), 1.f / 3.f), 1.f);
    return u < 0.25f ? ser : __logf(1.f + u);
}
// one (row, output) element of the Student-t data term for the kernels that branch at run time (layered, generic): adds
// wt log1p(r^2 k) to stat and returns dL/df = wt (nu + 1) r k / (1 + r^2 k), k = 1 / (nu s^2) -- the arithmetic of lik_delta's branch
__device__ __forceinline__ float student_elem(float fi, float y, double& stat, float wt, float k, float np1) {
#pragma clang fp contract(off)
    const float r = y - fi, u = r * r * k;
    stat += (double)(wt * log1p_fast(u));
    return wt * (np1 * (r * k) * __builtin_amdgcn_rcpf(1.f + u));
}

// Negative binomial with log link (TBNN_LIK_NEG_BINOMIAL), fi the log of the mean, r the dispersion, lr = log r derived once in the
// kernel's prologue.  With t = f - log r, p = sigmoid(t) = mu / (r + mu), q = 1 - p: the term y log p + r log q and dL/df = y q - r p.
// Neither e^f nor r + e^f is formed: a = |t|, e = e^-a in (0, 1] by the hardware exp2, l = log1p(e) (log1p_fast: accurate relative to
// itself, which the small side needs -- r log q ~ -mu when r is large), -log p = max(-t, 0) + l, -log q = max(t, 0) + l; p and q from e
// and ONE hardware reciprocal of 1 + e, picked by the sign of t.  y (-log p) and r (-log q) are both >= 0: nothing cancels in the term,
// and y q - r p is the difference of two bounded products.  Every finite f gives a finite term (f past the fp32 range of exp: e = 0,
// the term ~ -y |t| or -r t, finite while that product is: |f| to 1e30 at counts to 1e8); NaN gives NaN and k_energy rejects the proposal.  Not contracted, for the reason given at log1p_fast.
// *term: the element's part of the statistic (the constant lgamma(y + r) - lgamma(r) - lgamma(y + 1) is the handle's: data_logp,
// kernels_hmc.hpp); returns dL/df.  One function for lik_delta's compile-time branch and the kernels that branch at run time.
__device__ __forceinline__ float negbin_term(float fi, float y, float r, float lr, float* term) {
#pragma clang fp contract(off)
    const float t = fi - lr, a = fabsf(t);
    const float e = __expf(-a), l = log1p_fast(e);
    const float nlp = fmaxf(-t, 0.f) + l, nlq = fmaxf(t, 0.f) + l;
    const float rc = __builtin_amdgcn_rcpf(1.f + e), s = e * rc;
    const bool pos = t >= 0.f;
    const float p = pos ? rc : s, q = pos ? s : rc;
    *term = -(y * nlp + r * nlq);
    return y * q - r * p;
}
// ... for the kernels that branch at run time (layered, generic): adds wt term to stat, returns wt dL/df
__device__ __forceinline__ float negbin_elem(float fi, float y, double& stat, float wt, float r, float lr) {
#pragma clang fp contract(off)
    float term;
    const float d = negbin_term(fi, y, r, lr, &term);
    stat += (double)(wt * term);
    return wt * d;
}

// Gamma with log link (TBNN_LIK_GAMMA, defined in include/tbnn.h), fi the log of the mean.  ONE hardware exp2: e = e^-f, the element's
// part of the statistic f + y e^-f (its factor -a and the constant: data_logp, kernels_hmc.hpp) and, returned, y e^-f - 1: dL/df over the
// shape a, which the caller multiplies in.  A log-mean below the fp32 range of e^-f gives inf: the statistic is not finite and k_energy
// rejects the proposal (Poisson's rule, on the other side); NaN gives NaN.  On the other side, a log-mean above 87.3 puts e^-f below
// fp32's normal range and the hardware exp2 returns 0: the element becomes the term f and the delta -a, short of y e^-f < y 2^-126.  Staging
// admits targets up to 2^100 only (k_pois_const, GAMMA_Y_MAX), so what is lost stays below 2^-26 next to the 1 it is subtracted from.  Not contracted, for the reason given at log1p_fast.  One
// function for lik_delta's compile-time branch and the kernels that branch at run time.
__device__ __forceinline__ float gamma_term(float fi, float y, float* term) {
#pragma clang fp contract(off)
    const float ye = y * __expf(-fi);
    *term = fi + ye;
    return ye - 1.f;
}
// ... for the kernels that branch at run time (layered, generic): adds wt term to stat, returns wt dL/df = wt (a (y e^-f - 1))
__device__ __forceinline__ float gamma_elem(float fi, float y, double& stat, float wt, float a) {
#pragma clang fp contract(off)
    float term;
    const float d = gamma_term(fi, y, &term);
    stat += (double)(wt * term);
    return wt * (a * d);
}

// Weibull with right-censored targets (TBNN_LIK_WEIBULL, defined in include/tbnn.h), fi the log of the scale, k the shape.  The SIGN of
// the target is the censoring flag: y > 0 an event at time y (d = 1), y < 0 a row still running at time |y| (d = 0); the sign test and
// t = |y| read the same register.  ONE hardware log2 and ONE hardware exp2: u = (t e^-f)^k = exp(k (log t - f)), the element's part of
// the statistic k d f + u (its sign and the constant: data_logp, kernels_hmc.hpp) and, returned, u - d: dL/df over the shape k, which the
// caller multiplies in.  The term is picked by a select, not formed as d (k f): a NaN stays a NaN (y, f or u), and u past the fp32 range
// gives inf -- the statistic is not finite and k_energy rejects the proposal (Poisson's and Gamma's rule).  Staging admits 2^-100 <= |y|
// <= 2^100 only (k_pois_const), so the hardware log sees a normal number.  Not contracted, for the reason given at log1p_fast.  One
// function for lik_delta's compile-time branch and the kernels that branch at run time.
__device__ __forceinline__ float weibull_term(float fi, float y, float k, float* term) {
#pragma clang fp contract(off)
    const bool event = y > 0.f;
    const float u = __expf(k * (__logf(fabsf(y)) - fi));
    *term = event ? k * fi + u : u;
    return event ? u - 1.f : u;
}
// ... for the kernels that branch at run time (layered, generic): adds wt term to stat, returns wt dL/df = wt (k (u - d))
__device__ __forceinline__ float weibull_elem(float fi, float y, double& stat, float wt, float k) {
#pragma clang fp contract(off)
    float term;
    const float d = weibull_term(fi, y, k, &term);
    stat += (double)(wt * term);
    return wt * (k * d);
}

// Heteroscedastic Gaussian (TBNN_LIK_HETERO_GAUSSIAN): one ROW of a 2-output network, f the mean and g the log of the sd.  With
// G = log(1e8) (the clip of lik_sigma, on the log scale), gc = g clipped to [-G, G], u = e^(-2 gc) by the hardware exp2 (within
// [1e-16, 1e16]: never 0 or inf) and r = y - f: the row's term -gc - 1/2 r^2 u (the constant -1/2 log(2 pi) per row: data_logp,
// kernels_hmc.hpp), dL/df = r u and dL/dg = r^2 u - 1 inside the clip, 0 outside it (the derivative of the clipped function, as the
// Bernoulli clip's).  The clip is two selects, not fminf / fmaxf: a NaN g stays NaN, the statistic is not finite and k_energy rejects the
// proposal; so does r^2 u past the fp32 range.  Adds wt term to stat when `count`, returns wt dL/df and wt dL/dg in *df, *dg.  A
// multiplication by the weight 1 is exact and nothing here is contracted (the reason given at log1p_fast: which of r u, r (r u),
// 1/2 q + gc the compiler fuses is its choice per instantiation): a weighted kernel at weight 1 gives the unweighted kernel's bits.  One
// function for the fused families (kernels_fast.hpp: lik_pair) and the kernels that branch at run time.
#define HETERO_LOG_CLIP 18.420680743952367f          // log(1e8)
__device__ __forceinline__ void hetero_pair(float f, float g, float y, float wt, bool count, double& stat, float* df, float* dg) {
#pragma clang fp contract(off)
    float gc = g < -HETERO_LOG_CLIP ? -HETERO_LOG_CLIP : g;
    gc = g > HETERO_LOG_CLIP ? HETERO_LOG_CLIP : gc;
    const bool inside = g >= -HETERO_LOG_CLIP && g <= HETERO_LOG_CLIP;
    const float u = __expf(-2.f * gc);
    const float r = y - f, ru = r * u, q = r * ru;
    const float term = -gc - 0.5f * q;
    if (count) stat += (double)(wt * term);
    *df = wt * ru;
    *dg = inside ? wt * (q - 1.f) : 0.f;
}

__device__ __forceinline__ float act_fwd(float z, int act) {
    switch (act) {
        case TBNN_ACT_RELU: return fmaxf(z, 0.f);                  // activationFunctions.py:36
        case TBNN_ACT_TANH: return tanhf(z);                       // :62
        case TBNN_ACT_SIGMOID: return 1.f / (1.f + expf(-z));      // :49
        case TBNN_ACT_EXP: return expf(z);                         // :23
        case TBNN_ACT_ELU: return z > 0.f ? z : expm1f(z);         // :75
        default: return z;
    }
}
// derivative expressed through the activation OUTPUT a
__device__ __forceinline__ float act_bwd(float a, int act) {
    switch (act) {
        case TBNN_ACT_RELU: return a > 0.f ? 1.f : 0.f;
        case TBNN_ACT_TANH: return 1.f - a * a;
        case TBNN_ACT_SIGMOID: return a * (1.f - a);
        case TBNN_ACT_EXP: return a;
        case TBNN_ACT_ELU: return a > 0.f ? 1.f : a + 1.f;
        default: return 1.f;
    }
}

// diagnostic build only (-DTBNN_TILE_STAMPS): shader-clock stamps (per translation unit; tbnn_debug_tile_stamps reads
// the copy of tbnn_api.hip)
#ifdef TBNN_TILE_STAMPS
static __device__ unsigned long long g_tile_stamps[64];
#endif

// wave (64-lane) and block reductions
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// wave_sum's value in LANE 0 ONLY, bit for bit (the same tree: lane i += lane i + o for o = 32 .. 1), without the six dependent
// LDS-crossbar round trips of __shfl_down on a double (~650 cycles with one wave per SIMD): v_permlane32_swap / v_permlane16_swap
// (gfx950) bring the upper half / the odd rows down, row_shl DPP moves do the steps inside a row.  tools/ubench/wsum.hip checks the
// bits against wave_sum on the device.
template <int CTRL>
__device__ __forceinline__ double dpp_shl_add(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    const int hi2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return v + __hiloint2double(hi2, lo2);
}
__device__ __forceinline__ double wave_sum_lane0(double v) {
    {
        const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);      // [1]: lanes 0..31 <- lanes 32..63
        const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        v += __hiloint2double((int)b[1], (int)a[1]);
    }
    {
        const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);      // [1]: rows 0, 2 <- rows 1, 3
        const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v += __hiloint2double((int)b[1], (int)a[1]);
    }
    v = dpp_shl_add<0x108>(v);       // row_shl:8: lane i <- lane i + 8 of its row
    v = dpp_shl_add<0x104>(v);
    v = dpp_shl_add<0x102>(v);
    v = dpp_shl_add<0x101>(v);
    return v;
}
// max / sum over the four lane groups of a wave (lanes i16, i16 + 16, i16 + 32, i16 + 48: one data row of an MFMA D-layout tile), the result
// in all four, bit for bit the same value: v_permlane32_swap pairs lane i with lane i ^ 32, then v_permlane16_swap lane i with i ^ 16.
// Every lane of the wave must execute it (no divergent branch around the call).  The compiler's hazard recognizer keeps the two wait
// states between a VALU write of an operand and the swap reading it (builtins, not inline asm).
__device__ __forceinline__ float lanegroup_max(float v) {
    const unsigned u = __float_as_uint(v);
    const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);      // [0]: lane i <- lane i & 31, [1]: lane i <- 32 + (i & 31)
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const unsigned w = __float_as_uint(v);
    const auto b = __builtin_amdgcn_permlane16_swap(w, w, false, false);      // [0]: even row of the pair, [1]: odd row
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float lanegroup_sum(float v) {
    const unsigned u = __float_as_uint(v);
    const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const unsigned w = __float_as_uint(v);
    const auto b = __builtin_amdgcn_permlane16_swap(w, w, false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
__device__ __forceinline__ float wave_sumf(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// sum over the whole block; result valid in thread 0.  red: >= blockDim/64 doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    double t = 0.0;
    if (w == 0) {
        t = lane < nw ? red[lane] : 0.0;
        t = wave_sum(t);
    }
    return t;
}

// Philox4x32-10 chain RNG (replaces tf.random.set_seed(50), network.py:562).
// key = (seed, chain_id); counter = (block, epoch, purpose, 0).
struct Philox4 { uint32_t v[4]; };
__host__ __device__ __forceinline__ uint32_t tb_mulhi(uint32_t a, uint32_t b) {
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
}
__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                           uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint32_t p0h = tb_mulhi(0xD2511F53u, c0), p0l = 0xD2511F53u * c0;
        const uint32_t p1h = tb_mulhi(0xCD9E8D57u, c2), p1l = 0xCD9E8D57u * c2;
        const uint32_t n0 = p1h ^ c1 ^ k0, n1 = p1l, n2 = p0h ^ c3 ^ k1, n3 = p0l;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Philox4 o; o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}
__host__ __device__ __forceinline__ float u01(uint32_t x) {   // (0,1)
    return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f);
}
// j-th standard normal of (epoch, purpose): block j/4, Box-Muller pair (j%4)/2
__device__ __forceinline__ float philox_normal(uint32_t j, uint32_t epoch, uint32_t purpose, uint32_t k0, uint32_t k1) {
    const Philox4 r = philox4x32_10(j >> 2, epoch, purpose, 0u, k0, k1);
    const int h = (j >> 1) & 1;
    const float u1 = u01(r.v[2 * h]), u2 = u01(r.v[2 * h + 1]);
    const float rad = sqrtf(-2.f * logf(u1));
    const float ang = 6.28318530717958647692f * u2;
    return (j & 1) ? rad * sinf(ang) : rad * cosf(ang);
}
// the four normals of Philox block b = j / 4 at once (the same arithmetic as philox_normal, one block cipher instead of four)
__device__ __forceinline__ void philox_normal4(uint32_t b, uint32_t epoch, uint32_t purpose, uint32_t k0, uint32_t k1, float (&out)[4]) {
    const Philox4 r = philox4x32_10(b, epoch, purpose, 0u, k0, k1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = u01(r.v[2 * h]), u2 = u01(r.v[2 * h + 1]);
        const float rad = sqrtf(-2.f * logf(u1));
        const float ang = 6.28318530717958647692f * u2;
        out[2 * h] = rad * cosf(ang);
        out[2 * h + 1] = rad * sinf(ang);
    }
}
__device__ __forceinline__ float philox_logu(uint32_t epoch, uint32_t purpose, uint32_t k0, uint32_t k1) {
    const Philox4 r = philox4x32_10(0u, epoch, purpose, 0u, k0, k1);
    return logf(u01(r.v[0]));
}

#define PURPOSE_MOMENTUM 0u
#define PURPOSE_LOGU 1u
#define PURPOSE_HYPER_MOMENTUM 2u
#define PURPOSE_HYPER_LOGU 3u
