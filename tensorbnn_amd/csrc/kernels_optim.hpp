// Pre-training on the device (tbnn_optimize): Adam / AMSGrad ascent of the target log-probability -- the optimiser's siblings of
// k_update and k_energy.  One step = the fused forward+backward pass every family already has (unchanged), then k_optim: slab reduction,
// prior gradient, one Adam step in fp32, image scatter.  On the steps that are checked k_optim_logp runs between the two: it forms the
// objective at theta_t and sets the chain's flags, which k_optim reads.
// Restates BNN_functions.trainBasicRegression / trainBasicClassification's optimiser (BNN_functions.py:137-138, :256-257: Adam with
// amsgrad=True), as torch.optim.Adam(amsgrad=..., maximize=True) defines the step:
//   m = b1 m + (1 - b1) g ; v = b2 v + (1 - b2) g^2 ; vhat = amsgrad ? max(vhat, v) : v
//   theta += a_t m / (sqrt(vhat) r_t + epsilon),   a_t = lr / (1 - b1^t),  r_t = 1 / sqrt(1 - b2^t)   (formed on the host in fp64)
#pragma once
#include "common.hpp"
#include "update_ops.hpp"
#include "kernels_hmc.hpp"

// per-chain record of a run: what k_optim_logp writes and k_optim reads
struct OptChain {
    double best;          // the largest finite objective seen since the last reset (-inf: none)
    int best_step;        // the optimiser step t it was seen at
    int better;           // the LAST checked objective became `best`: theta_t is the new q_best
    int frozen;           // a checked objective was not finite: the chain makes no update from then on
    int pad;
};
// the Adam step's scalars (by value: wave-uniform)
struct OptStep { float a_t, r_t, b1, b2, omb1, omb2, epsilon; int amsgrad; };

// Single-workgroup kernel per chain (gridDim.y = chain): the objective at theta_t = q from the statistic partials of the pass that has
// just run -- the target log-probability, or (likelihood_only) its data term alone -- into trace[c][k], and the chain's flags.
__global__ __launch_bounds__(1024) void k_optim_logp(
    NetDev nd, int likelihood_only, const float* __restrict__ eta, const float* __restrict__ q,
    const double* __restrict__ partial_stat, int nslab, double n, double lik_c,
    OptChain* __restrict__ oc, int step, double* __restrict__ trace, int n_checks, int k)
{
    __shared__ double red[16];
    if (blockIdx.y) {
        const size_t c = blockIdx.y;
        eta += c * nd.H; q += c * (size_t)nd.P; partial_stat += c * PSTAT_CAP; oc += c;
        trace += c * (size_t)n_checks;
    }
    double st = 0.0;
    for (int w = threadIdx.x; w < nslab; w += blockDim.x) st += partial_stat[w];
    st = block_sum(st, red);
    double pr = 0.0;
    if (!likelihood_only) {
        pr = prior_logp_partial(nd, eta, q);
        pr = block_sum(pr, red);
    }
    if (threadIdx.x != 0) return;
    const double lp = pr + data_logp(nd, eta, st, n, lik_c);
    trace[k] = lp;
    const bool fin = isfinite(lp);
    const bool better = fin && lp > oc->best;
    oc->better = better ? 1 : 0;
    if (better) { oc->best = lp; oc->best_step = step; }
    if (!fin) oc->frozen = 1;
}

// k_update's geometry (UC float4 columns x UG slab groups per block, gridDim.y = chain).  checked: k_optim_logp has judged theta_t in
// this step, so the chain's flags are this step's.
template <int UC = UPD_COLS, int UG = UPD_GROUPS>
__global__ __launch_bounds__(UC * UG) void k_optim(
    NetDev nd, int likelihood_only, OptStep s, int checked, const float* __restrict__ eta,
    const float* __restrict__ slabs, int nslab, int pitch,
    float* __restrict__ q, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, float* __restrict__ vhat,
    float* __restrict__ q_best, const OptChain* __restrict__ oc,
    const int* __restrict__ imgmap, float* __restrict__ qimg, int img_floats)
{
    if (blockIdx.y) {
        const size_t c = blockIdx.y, cp = c * (size_t)nd.P;
        eta += c * nd.H; slabs += c * (size_t)nslab * pitch;
        q += cp; g += cp; m += cp; v += cp; vhat += cp; q_best += cp; oc += c;
        if (qimg) qimg += c * (size_t)img_floats;
    }
    const int better = checked ? oc->better : 0, frozen = oc->frozen;      // (block-uniform)
    __shared__ float4 part[UG][UC];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int c4 = blockIdx.x * UC + tx;                // float4 column
    const int jf = c4 * 4 + ty;                         // ty < 4 selects which of the column's 4 parameters this thread finishes
    const bool fin = ty < 4 && jf < nd.P;
    // what the finishing thread needs, fetched before the slab loads (upd_prefetch's reason)
    float th = 0.f, mj = 0.f, vj = 0.f, vh = 0.f, loc = 0.f, scale = 1.f;
    int prior = 0, m0 = -1, m1 = -1;
    if (fin) {
        th = q[jf];
        if (better) q_best[jf] = th;                    // theta_t, the value this thread already holds
        if (!frozen) {
            if (!likelihood_only) prior_params(nd, eta, jf, prior, loc, scale);
            mj = m[jf]; vj = v[jf]; vh = vhat[jf];
            if (imgmap) { m0 = imgmap[jf]; m1 = imgmap[nd.P + jf]; }
        }
    }
    if (frozen) return;                                 // (the whole block: no barrier is left waiting)
    part[ty][tx] = upd_column_partial<UG>(slabs, nslab, pitch, c4, ty);
    __syncthreads();
    if (!fin) return;
    float gj = upd_block_sum<UC, UG>(part, tx, ty);     // (k_update's reduction: one barrier, the tree's additions in registers)
    if (!likelihood_only) gj += prior_grad(prior, loc, scale, th);
    g[jf] = gj;
    mj = s.b1 * mj + s.omb1 * gj;
    vj = s.b2 * vj + s.omb2 * (gj * gj);
    vh = s.amsgrad ? fmaxf(vh, vj) : vj;
    th += s.a_t * mj / (sqrtf(vh) * s.r_t + s.epsilon);
    m[jf] = mj; v[jf] = vj; vhat[jf] = vh; q[jf] = th;
    if (imgmap) { qimg[m0] = th; if (m1 >= 0) qimg[m1] = th; }
}

// After the last evaluation (at theta_T = q): q_best takes theta_T when that evaluation was the best, and the chain's state q_cur
// becomes q_best (keep_best, or the chain froze) or theta_T.  gridDim.y = chain.
__global__ __launch_bounds__(256) void k_optim_finish(int P, int keep_best, const OptChain* __restrict__ oc, const float* __restrict__ q,
                                                      float* __restrict__ q_best, float* __restrict__ q_cur) {
    const size_t c = blockIdx.y, cp = c * (size_t)P;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P) return;
    const OptChain me = oc[c];
    const float th = q[cp + j];
    float qb = q_best[cp + j];
    if (me.better) { qb = th; q_best[cp + j] = th; }
    q_cur[cp + j] = (keep_best || me.frozen) ? qb : th;
}

// reset: no moments, no best record (q_best = the start state: what a chain that freezes at its first check goes back to)
__global__ __launch_bounds__(256) void k_optim_reset(int P, int chains, const float* __restrict__ q_cur, float* __restrict__ m, float* __restrict__ v,
                                                     float* __restrict__ vhat, float* __restrict__ g, float* __restrict__ q_best, OptChain* __restrict__ oc) {
    const size_t c = blockIdx.y, cp = c * (size_t)P;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < P) { m[cp + j] = 0.f; v[cp + j] = 0.f; vhat[cp + j] = 0.f; g[cp + j] = 0.f; q_best[cp + j] = q_cur[cp + j]; }
    if (j == 0) { OptChain z; z.best = -INFINITY; z.best_step = 0; z.better = 0; z.frozen = 0; z.pad = 0; oc[c] = z; }
}
