// Integrated-gradients attributions of an ensemble (tbnn_ensemble_integrated_grad, include/tbnn.h): for every network, row, output and input
// A = (x_k - x0_k) sum_s q_s J[o][k](x_s) over P points x_s of the straight path from the baseline x0 to x, with its moments over the
// networks, in one kernel -- k_ens_path_grad.  J is the Jacobian of k_ens_input_grad (kernels_input_grad.hpp), whose panel streaming
// (ig_next, ig_load, ig_store), planes (ig_accum, k_ens_input_grad_finish) and LDS map this kernel shares; what is its own:
//
//   path      The path is the M axis.  A tile of RT MFMA rows holds DR = RT / P data rows times P path points, tile row = rd P + s, so a
//             wave's 16 rows are 16 consecutive points of one data row (RT = 64: 4, 2 or 1 data rows; RT = 16: one, at P = 16).  The
//             prologue builds x_s = fmaf(s / (P - 1), x - x0, x0) (s = P - 1: x itself) into the record from X and the baseline: nothing of
//             size P n exists outside LDS.  The forward pass and the reverse pass down to G_1 are those of the Jacobian kernel.
//   reduce    sum_s q_s (G_1(x_s) W_1) = (sum_s q_s G_1(x_s)) W_1: the quadrature sum is taken BEFORE the product with W_1, the largest of
//             the reverse pass where d_in is.  The epilogue of the step that forms G_1 does not store it: a lane weights its 4 accumulator
//             rows (4 consecutive s) by q_s act'(a_1) and sums them, two row swaps (xor 16, 32) sum the 4 lane groups -- one wave, 16 path
//             points, one value per (unit j, output t) --, and lane group 0 writes it to part[j][t (RT / 16) + wave] in the G buffer G_1
//             would have taken.  P = 16: that is Gbar_1[j][t DR + rd] already.  P = 32, 64: the P / 16 partials of a pair are neighbours
//             there and are summed in wave order into the other G buffer, which is free by then.  No hidden layer: G_1 is the seed, and
//             Gbar_1 is summed from its expression directly, s ascending.
//   last      Gbar_1 W_1 with M = the (output of the group, data row) pairs of the tile, t DR + rd < og DR <= RT: wave v takes pairs
//             16 v .. 16 v + 15 where there are any (M padded to 16), one accumulator tile, the same panels of W_1 as the Jacobian's last
//             step.  Times d_k = x_k - x0_k (the record's rows s = P - 1 and s = 0 of input k, which are x and x0 themselves), then to
//             attr_out and into the planes; the workgroup is the only writer of its rows: no atomics, the same bits whatever the chunks.
//   diff      scale (g(f(x)) - g(f(x0))) from the record's last layer at s = P - 1 and s = 0, by ens_xform.
//   LDS       ig_lds_floats(d_in, sumOut, maxOut, RT, og): the Jacobian's map, nothing added -- the partials and Gbar_1 take at most
//             maxOut og (RT / 16) floats of a G buffer of maxOut (og RT + 1).
// The first layer's pre-activation is linear in s; it is NOT interpolated from the end points here: every x_s goes through the MFMAs.
#pragma once
#include "kernels_input_grad.hpp"

// trapezoid weight of path point s of P
__device__ __forceinline__ float pg_weight(int s, int P) {
    return (s == 0 || s == P - 1 ? 0.5f : 1.f) / (float)(P - 1);
}

// thetas, w, first, acc as k_ens_input_grad's; X: the block's rows [nr][d_in]; base: the baseline [d_in]; P: path points, 16, 32 or 64, at
// most RT; attr: [c][d_out][d_in][nr] or null; diff: [c][d_out][nr] or null.  grid: one workgroup per RT / P rows
template <int RT, int LDSF>
__global__ __launch_bounds__(RT * 4) void k_ens_path_grad(NetDev nd, const float* __restrict__ thetas, int c, const float* __restrict__ X,
                                                           const float* __restrict__ base, long nr, int P, int og, int maxOut, int xform,
                                                           float scale, const float* __restrict__ w, int first, double* __restrict__ acc,
                                                           float* __restrict__ attr, float* __restrict__ diff) {
    constexpr int NT = RT * 4, RS = RT + 1, NWV = RT / 16;
    __shared__ float lds[LDSF];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int MS = og * RT + 1;
    const int DR = RT / P, NW = P / 16;                     // data rows of the tile; waves (partials) per data row
    float* const rec = lds;
    float* const G = rec + (nd.d_in + nd.sumOut) * RS;
    float* const Wp = G + 2 * maxOut * MS;
    const long row0 = (long)blockIdx.x * DR;                // the first data row of the tile
    const long tot = (long)nd.d_out * nd.d_in * nr;
    const int wrow = 16 * wv + 4 * lg;                      // the first of the 4 tile rows (or pairs) this lane holds in an accumulator
    // G_1 is the input of the reverse step of layer 0, which reads buffer (nl - 1) & 1
    float* const Gpart = G + ((nd.nl - 1) & 1) * maxOut * MS;
    float* const Gbar = nd.nl > 1 && NW > 1 ? G + (((nd.nl - 1) & 1) ^ 1) * maxOut * MS : Gpart;

    for (int e = tid; e < RT * nd.d_in; e += NT) {
        const int r = e / nd.d_in, k = e - r * nd.d_in, rd = r / P, s = r - rd * P;
        const float x = row0 + rd < nr ? X[(row0 + rd) * nd.d_in + k] : 0.f, x0 = base[k];
        rec[k * RS + r] = s == P - 1 ? x : fmaf((float)s / (float)(P - 1), x - x0, x0);
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
        const float* __restrict__ Pn = Wp + buf * IG_PANEL + lg * IG_PS + lr;
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
                a4[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(k < K ? a : 0.f, Pn[kk * IG_PS], a4[0], 0, 0, 0);
            }
            if (last && col < N) {
                const float b = thetas[(size_t)cur.i * nd.P + nd.offB[l] + col];
                float* __restrict__ ao = rec + (nd.d_in + nd.actOff[l] + col) * RS + wrow;
#pragma unroll
                for (int j = 0; j < 4; ++j) ao[j] = act_fwd(a4[0][j] + b, nd.act[l]);
            }
        } else {
            const int ogc = min(og, nd.d_out - cur.g0);
            const int npair = ogc * DR;
            const int par = (nd.nl - 1 - l) & 1;
            float* const Gin = G + par * maxOut * MS;
            float* const Gout = G + (par ^ 1) * maxOut * MS;
            if (l == nd.nl - 1 && cur.n0 == 0 && cur.k0 == 0) {
                const float* __restrict__ aL = rec + (nd.d_in + nd.actOff[l]) * RS;
                if (diff && cur.g0 == 0)
                    for (int e = tid; e < nd.d_out * DR; e += NT) {
                        const int rd = e % DR, o = e / DR;
                        if (row0 + rd < nr)
                            diff[((size_t)cur.i * nd.d_out + o) * nr + row0 + rd] =
                                scale * (ens_xform(aL[o * RS + rd * P + P - 1], xform) - ens_xform(aL[o * RS + rd * P], xform));
                    }
                if (l > 0) {
                    // the seed of this group: G_L[k][t][r] = s g'(f) act'(f) at k = g0 + t, 0 elsewhere
                    for (int e = tid; e < K * ogc * RT; e += NT) {
                        const int r = e % RT, t = (e / RT) % ogc, k = e / (RT * ogc);
                        float v = 0.f;
                        if (k == cur.g0 + t) { const float f = aL[k * RS + r]; v = scale * ig_gprime(f, xform) * act_bwd(f, nd.act[l]); }
                        Gin[k * MS + t * RT + r] = v;
                    }
                } else {
                    // no hidden layer: the seed is G_1, summed over the path as it is formed
                    for (int e = tid; e < K * npair; e += NT) {
                        const int p = e % npair, k = e / npair, t = p / DR, rd = p - t * DR;
                        float v = 0.f;
                        if (k == cur.g0 + t)
                            for (int s = 0; s < P; ++s) {
                                const float f = aL[k * RS + rd * P + s];
                                v += pg_weight(s, P) * (scale * ig_gprime(f, xform) * act_bwd(f, nd.act[l]));
                            }
                        Gbar[k * MS + p] = v;
                    }
                }
                __syncthreads();
            }
            if (l == 0 && nd.nl > 1 && NW > 1 && cur.n0 == 0 && cur.k0 == 0) {
                // the partials of the waves of a data row, in wave order
                for (int e = tid; e < K * npair; e += NT) {
                    const int p = e % npair, k = e / npair;
                    float v = Gpart[k * MS + p * NW];
                    for (int u = 1; u < NW; ++u) v += Gpart[k * MS + p * NW + u];
                    Gbar[k * MS + p] = v;
                }
                __syncthreads();
            }
            if (l > 0) {
                if (cur.k0 == 0) {
#pragma unroll
                    for (int t = 0; t < IG_OG; ++t) a4[t] = tb_f32x4{0.f, 0.f, 0.f, 0.f};
                }
                const float* __restrict__ gi = Gin + 16 * wv + lr;
                for (int kk = 0; kk < kend; kk += 4) {
                    const int k = cur.k0 + kk + lg;
                    const float b = Pn[kk * IG_PS];
                    const float* __restrict__ gk = gi + (k < K ? k : 0) * MS;
#pragma unroll
                    for (int t = 0; t < IG_OG; ++t)
                        if (t < ogc) {
                            const float a = gk[t * RT];
                            a4[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(k < K ? a : 0.f, b, a4[t], 0, 0, 0);
                        }
                }
                if (last) {
                    // every lane takes the row swaps; columns beyond N read column 0 and store nothing
                    const float* __restrict__ ap = rec + (nd.d_in + nd.actOff[l - 1] + (col < N ? col : 0)) * RS + wrow;
                    float d[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) d[j] = act_bwd(ap[j], nd.act[l - 1]);
                    if (l > 1) {
                        if (col < N) {
                            float* __restrict__ go = Gout + col * MS + wrow;
#pragma unroll
                            for (int t = 0; t < IG_OG; ++t)
                                if (t < ogc) {
#pragma unroll
                                    for (int j = 0; j < 4; ++j) go[t * RT + j] = a4[t][j] * d[j];
                                }
                        }
                    } else {
                        const int s0 = wrow & (P - 1);
#pragma unroll
                        for (int j = 0; j < 4; ++j) d[j] *= pg_weight(s0 + j, P);
#pragma unroll
                        for (int t = 0; t < IG_OG; ++t)
                            if (t < ogc) {
                                float v = a4[t][0] * d[0];
#pragma unroll
                                for (int j = 1; j < 4; ++j) v += a4[t][j] * d[j];
                                v += __shfl_xor(v, 16, 64);
                                v += __shfl_xor(v, 32, 64);
                                if (lg == 0 && col < N) Gpart[col * MS + t * NWV + wv] = v;
                            }
                    }
                }
            } else if (16 * wv < npair) {
                if (cur.k0 == 0) a4[0] = tb_f32x4{0.f, 0.f, 0.f, 0.f};
                const int pa = 16 * wv + lr;
                for (int kk = 0; kk < kend; kk += 4) {
                    const int k = cur.k0 + kk + lg;
                    const float a = Gbar[(k < K ? k : 0) * MS + pa];
                    a4[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(k < K && pa < npair ? a : 0.f, Pn[kk * IG_PS], a4[0], 0, 0, 0);
                }
                if (last && col < N) {
                    const double wi = w ? (double)w[cur.i] : 1.0;
                    const bool fst = first && cur.i == 0;
                    const float* __restrict__ xk = rec + col * RS;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int p = wrow + j, t = p / DR, rd = p - t * DR;
                        if (p < npair && row0 + rd < nr) {
                            const float v = a4[0][j] * (xk[rd * P + P - 1] - xk[rd * P]);
                            const long e = ((long)(cur.g0 + t) * nd.d_in + col) * nr + row0 + rd;
                            if (attr) attr[(size_t)cur.i * tot + e] = v;
                            ig_accum(acc, tot, e, v, wi, fst);
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
