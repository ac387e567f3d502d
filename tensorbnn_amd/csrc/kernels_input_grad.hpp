// Input sensitivities of an ensemble (tbnn_ensemble_input_grad, include/tbnn.h): every network's Jacobian d xform(f_o) / d x_k per row, and
// its moments over the networks, in one kernel -- k_ens_input_grad.  Nothing else in the library propagates a gradient to the inputs.
//
//   split     Row tile stationary, networks streamed.  A workgroup owns RT rows (64: four waves; 16: one wave), a wave 16 of them, and walks
//             the c networks of the chunk in order.  It is the only writer of its rows' elements of the four fp64 planes and adds network
//             after network by plain read-modify-write (the same thread every time): no atomics, the same bits whatever the chunks.
//   passes    Both on v_mfma_f32_16x16x4_f32.  Forward, layer l: Z = A_{l-1} W_l^T, M = the wave's 16 rows, N = 16 outputs of the layer,
//             K = its inputs; bias and activation in the epilogue, a_l into the record.  Reverse: G_{l-1} = (G_l W_l) o act'(a_{l-1}) seeded
//             with G_L = s g'(f_o) act'(a_L) e_o; M = the stacked (output, row) pairs -- a wave keeps one accumulator tile per output of
//             the group for its 16 rows, so og outputs cost one walk over W_l --, N = 16 inputs of the layer, K = its outputs.  The last
//             step G_1 W_1 is not stored in LDS: its accumulator tiles go straight to jac_out and into the planes (a lane holds 4
//             consecutive rows of one input column: 16 lanes x 4 groups fill whole lines of a plane).
//   LDS map   rec  [d_in + sumOut][RT + 1]   x and a_1 .. a_L, feature-major, the row the fast axis (the A operand reads 16 consecutive
//                                            rows of one feature; the odd stride spreads the epilogue's stores over the banks)
//             G    2 x [maxOut][og RT + 1]   G_l and G_{l-1} in turn, feature-major, (output of the group, row) the fast axis
//             Wp   2 x [IG_KC][IG_PS]        two weight panels: 16 columns of N by IG_KC values of K, zero-padded at both fringes
//             (d_in + sumOut)(RT + 1) + 2 maxOut (og RT + 1) + 2 IG_KC IG_PS floats; og = the most outputs (<= 16) that fit IG_LDS_MAX
//             floats with RT = 64, else with RT = 16, else the call is refused.  More than og outputs: the reverse pass runs per group.
//   panels    Every W_l goes through LDS in panels of IG_KC x 16 floats, so no width is limited by the panels.  One sequence of panels
//             runs through the layers, both passes, the groups and the networks (ig_next); the loads of the next panel are issued into
//             registers before the MFMAs of the current one and stored into the other buffer after them, one barrier per panel.
//   fringes   No width need be a multiple of 16 or 4: the panels are padded with zeros, the A operand is masked beyond K, columns beyond N
//             are not stored.  (The 4x4x1 form is not used: the kernel is untuned.)
// fp32 throughout the passes -- act_fwd / act_bwd of common.hpp, act' from the fp32 activation outputs as the training kernels take it --,
// fp64 in the planes: ref = the first network's value, S1 = sum w (J - ref), S2 = sum w (J - ref)^2 (the shifted form of k_ens_moments) and
// SA = sum w |J|.  A value that is not finite enters as NaN.  k_ens_input_grad_finish: mean, variance (population form), mean |J|.
#pragma once
#include "kernels_ensemble.hpp"

#define IG_KC 64                         // values of K per weight panel
#define IG_PS 17                         // floats per K-row of a panel in LDS: 16 columns and one of padding
#define IG_PANEL (IG_KC * IG_PS)
#define IG_OG 16                         // outputs per group of the reverse pass at the most: accumulator tiles a wave carries
#define IG_LDS_MAX 40944                 // floats of LDS a workgroup may take (160 KiB less 64 bytes)
#define IG_LDS_MID 20480                 // ... and the two smaller instantiations: two and four workgroups per CU
#define IG_LDS_MIN 10240

__host__ __device__ inline long ig_lds_floats(int d_in, int sumOut, int maxOut, int rt, int og) {
    return (long)(d_in + sumOut) * (rt + 1) + 2L * maxOut * (og * rt + 1) + 2L * IG_PANEL;
}

// one weight panel of the sequence: network i, outputs from g0 (reverse pass), the pass, the layer, the first column of N and value of K
struct IgPanel { int i, g0, rev, l, n0, k0; };
// the panel after p; false: p was the last panel of the chunk's last network
__device__ __forceinline__ bool ig_next(IgPanel& p, const NetDev& nd, int c, int og) {
    const int K = p.rev ? nd.out[p.l] : nd.in[p.l], N = p.rev ? nd.in[p.l] : nd.out[p.l];
    p.k0 += IG_KC;
    if (p.k0 < K) return true;
    p.k0 = 0; p.n0 += 16;
    if (p.n0 < N) return true;
    p.n0 = 0;
    if (!p.rev) {
        if (++p.l < nd.nl) return true;
        p.rev = 1; p.l = nd.nl - 1; p.g0 = 0;
        return true;
    }
    if (--p.l >= 0) return true;
    p.g0 += og;
    if (p.g0 < nd.d_out) { p.l = nd.nl - 1; return true; }
    p.rev = 0; p.l = 0; p.g0 = 0;
    return ++p.i < c;
}
// panel element (k, n): forward W_l[n0 + n][k0 + k] (B = W^T), reverse W_l[k0 + k][n0 + n]; 0 beyond the layer.  Forward a thread walks
// k (the fast axis of W there), reverse n.
template <int NT>
__device__ __forceinline__ void ig_load(float (&st)[IG_KC * 16 / NT], const float* __restrict__ thetas, const NetDev& nd, const IgPanel& p, int tid) {
    const int in = nd.in[p.l], out = nd.out[p.l];
    const float* __restrict__ W = thetas + (size_t)p.i * nd.P + nd.offW[p.l];
#pragma unroll
    for (int q = 0; q < IG_KC * 16 / NT; ++q) {
        const int e = q * NT + tid;
        const int k = p.rev ? e >> 4 : e % IG_KC, n = p.rev ? e & 15 : e / IG_KC;
        const int ro = p.rev ? p.k0 + k : p.n0 + n, ci = p.rev ? p.n0 + n : p.k0 + k;      // row (output) and column (input) of W_l
        st[q] = (ro < out && ci < in) ? W[(size_t)ro * in + ci] : 0.f;
    }
}
template <int NT>
__device__ __forceinline__ void ig_store(float* __restrict__ P, const float (&st)[IG_KC * 16 / NT], const IgPanel& p, int tid) {
#pragma unroll
    for (int q = 0; q < IG_KC * 16 / NT; ++q) {
        const int e = q * NT + tid;
        const int k = p.rev ? e >> 4 : e % IG_KC, n = p.rev ? e & 15 : e / IG_KC;
        P[k * IG_PS + n] = st[q];
    }
}
// g'(f) of the element-wise transforms, by the expressions of ens_xform
__device__ __forceinline__ float ig_gprime(float f, int xform) {
    if (xform == TBNN_XFORM_EXP) return expf(f);
    if (xform == TBNN_XFORM_SIGMOID) { const float g = 1.f / (1.f + expf(-f)); return g * (1.f - g); }
    return 1.f;
}
// one network's value v of element e into the planes acc[4][tot]; fst: network 0 of the call, whose value is the shift
__device__ __forceinline__ void ig_accum(double* __restrict__ acc, long tot, long e, float v, double w, bool fst) {
    const double x = isfinite(v) ? (double)v : (double)NAN;
    if (fst) { acc[e] = x; acc[tot + e] = 0.0; acc[2 * tot + e] = 0.0; acc[3 * tot + e] = w * fabs(x); return; }
    const double d = x - acc[e], wd = w * d;
    acc[tot + e] += wd;
    acc[2 * tot + e] = fma(wd, d, acc[2 * tot + e]);
    acc[3 * tot + e] += w * fabs(x);
}

// thetas: the chunk [c][P]; X: the block's rows [nr][d_in]; w: the chunk's c weights or null (equal); first: the chunk starts at network 0;
// acc: [4][d_out d_in nr]; jac: [c][d_out][d_in][nr] or null.  grid: one workgroup per RT rows.  LDSF: the floats of LDS of the instantiation,
// at least ig_lds_floats(.., RT, og)
template <int RT, int LDSF>
__global__ __launch_bounds__(RT * 4) void k_ens_input_grad(NetDev nd, const float* __restrict__ thetas, int c, const float* __restrict__ X, long nr,
                                                            int og, int maxOut, int xform, float scale, const float* __restrict__ w, int first,
                                                            double* __restrict__ acc, float* __restrict__ jac) {
    constexpr int NT = RT * 4, RS = RT + 1;
    __shared__ float lds[LDSF];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int MS = og * RT + 1;
    float* const rec = lds;
    float* const G = rec + (nd.d_in + nd.sumOut) * RS;
    float* const Wp = G + 2 * maxOut * MS;
    const long row0 = (long)blockIdx.x * RT;
    const long tot = (long)nd.d_out * nd.d_in * nr;
    const int wrow = 16 * wv + 4 * lg;                      // the first of the 4 rows of the tile this lane holds in an accumulator

    for (int e = tid; e < RT * nd.d_in; e += NT) {
        const int r = e / nd.d_in, k = e - r * nd.d_in;
        rec[k * RS + r] = row0 + r < nr ? X[(row0 + r) * nd.d_in + k] : 0.f;
    }
    IgPanel cur{0, 0, 0, 0, 0, 0};
    float st[IG_KC * 16 / NT];
    ig_load<NT>(st, thetas, nd, cur, tid);
    ig_store<NT>(Wp, st, cur, tid);
    __syncthreads();

    tb_f32x4 a4[IG_OG];
    int buf = 0;
    for (bool more = true; more;) {
        IgPanel nxt = cur;
        more = ig_next(nxt, nd, c, og);
        if (more) ig_load<NT>(st, thetas, nd, nxt, tid);

        const int l = cur.l, in = nd.in[l], out = nd.out[l];
        const float* __restrict__ P = Wp + buf * IG_PANEL + lg * IG_PS + lr;
        const int K = cur.rev ? out : in, N = cur.rev ? in : out;
        const int kend = min(IG_KC, (K - cur.k0 + 3) & ~3);
        const bool last = cur.k0 + IG_KC >= K;
        const int col = cur.n0 + lr;
        if (!cur.rev) {
            const float* __restrict__ ain = rec + (l ? nd.d_in + nd.actOff[l - 1] : 0) * RS + 16 * wv + lr;
            if (cur.k0 == 0) a4[0] = tb_f32x4{0.f, 0.f, 0.f, 0.f};
            for (int kk = 0; kk < kend; kk += 4) {
                const int k = cur.k0 + kk + lg;
                const float a = ain[(k < K ? k : 0) * RS];
                a4[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(k < K ? a : 0.f, P[kk * IG_PS], a4[0], 0, 0, 0);
            }
            if (last && col < N) {
                const float b = thetas[(size_t)cur.i * nd.P + nd.offB[l] + col];
                float* __restrict__ ao = rec + (nd.d_in + nd.actOff[l] + col) * RS + wrow;
#pragma unroll
                for (int j = 0; j < 4; ++j) ao[j] = act_fwd(a4[0][j] + b, nd.act[l]);
            }
        } else {
            const int ogc = min(og, nd.d_out - cur.g0);
            const int par = (nd.nl - 1 - l) & 1;
            float* const Gin = G + par * maxOut * MS;
            float* const Gout = G + (par ^ 1) * maxOut * MS;
            if (l == nd.nl - 1 && cur.n0 == 0 && cur.k0 == 0) {
                // the seed of this group: G_L[k][t][r] = s g'(f) act'(f) at k = g0 + t, 0 elsewhere
                const float* __restrict__ aL = rec + (nd.d_in + nd.actOff[l]) * RS;
                for (int e = tid; e < K * ogc * RT; e += NT) {
                    const int r = e % RT, t = (e / RT) % ogc, k = e / (RT * ogc);
                    float v = 0.f;
                    if (k == cur.g0 + t) { const float f = aL[k * RS + r]; v = scale * ig_gprime(f, xform) * act_bwd(f, nd.act[l]); }
                    Gin[k * MS + t * RT + r] = v;
                }
                __syncthreads();
            }
            if (cur.k0 == 0) {
#pragma unroll
                for (int t = 0; t < IG_OG; ++t) a4[t] = tb_f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const float* __restrict__ gi = Gin + 16 * wv + lr;
            for (int kk = 0; kk < kend; kk += 4) {
                const int k = cur.k0 + kk + lg;
                const float b = P[kk * IG_PS];
                const float* __restrict__ gk = gi + (k < K ? k : 0) * MS;
#pragma unroll
                for (int t = 0; t < IG_OG; ++t)
                    if (t < ogc) {
                        const float a = gk[t * RT];
                        a4[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(k < K ? a : 0.f, b, a4[t], 0, 0, 0);
                    }
            }
            if (last && col < N) {
                if (l > 0) {
                    const float* __restrict__ ap = rec + (nd.d_in + nd.actOff[l - 1] + col) * RS + wrow;
                    float d[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) d[j] = act_bwd(ap[j], nd.act[l - 1]);
                    float* __restrict__ go = Gout + col * MS + wrow;
#pragma unroll
                    for (int t = 0; t < IG_OG; ++t)
                        if (t < ogc) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) go[t * RT + j] = a4[t][j] * d[j];
                        }
                } else {
                    const double wi = w ? (double)w[cur.i] : 1.0;
                    const bool fst = first && cur.i == 0;
#pragma unroll
                    for (int t = 0; t < IG_OG; ++t)
                        if (t < ogc) {
                            const long e0 = ((long)(cur.g0 + t) * nd.d_in + col) * nr + row0 + wrow;
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (row0 + wrow + j < nr) {
                                    const float v = a4[t][j];
                                    if (jac) jac[(size_t)cur.i * tot + e0 + j] = v;
                                    ig_accum(acc, tot, e0 + j, v, wi, fst);
                                }
                        }
                }
            }
        }
        if (more) ig_store<NT>(Wp + (buf ^ 1) * IG_PANEL, st, nxt, tid);
        __syncthreads();
        cur = nxt; buf ^= 1;
    }
}

// in place: acc[0] <- mean, acc[1] <- variance (never below 0: the subtraction may round there), acc[3] <- mean |J|; a NaN stays one
__global__ __launch_bounds__(ENS_TB) void k_ens_input_grad_finish(double* __restrict__ acc, long tot, double W) {
    for (long e = (long)blockIdx.x * ENS_TB + threadIdx.x; e < tot; e += (long)gridDim.x * ENS_TB) {
        const double m1 = acc[tot + e] / W;
        const double v = fma(-m1, m1, acc[2 * tot + e] / W);
        acc[e] += m1;
        acc[tot + e] = v != v ? v : fmax(v, 0.0);
        acc[3 * tot + e] /= W;
    }
}
