// The kernel families behind one host-side interface.  A handle (tbnn_api.hip: tbnn_ctx) owns ONE Backend -- chosen and constructed by
// select_kernels -- and the host layer never asks which family it got: it prepares the backend for a data set, asks it for gradients,
// forward passes and (where it has one) whole trajectories.  Each backend owns its plan and its private device buffers.
// Host only, included by tbnn_api.hip alone, after the kernel headers and its owners and error helpers (Buf, fail, HIPCHK): nothing here
// crosses the dlopen boundary -- a kernel library still registers a FusedOps table (fused_ops.hpp), which FusedBackend / WideBackend wrap.
// tbnn_api.hip's include order: kernel headers, owners and error helpers, this file, tbnn_ctx and the launch helpers, ensemble_api.hpp.
#pragma once

// one gradient (forward + backward pass over the rows) for all chains of a handle
struct PassArgs {
    const float* img; long img_stride;        // the padded weight images [C][img_stride] (null: the backend has none)
    const float* q;                           // the weights themselves [C][P]
    const float* eta; long eta_stride;
    const float* X; const float* Y; const float* w; long n;   // Y: the targets the pass reads ([Y | w] while row weights are set); w: the weights or null
    float* slabs; long slab_stride; int pitch;                // gradient slabs [C][nslab][pitch]
    double* pstat;                            // statistic partials [C][PSTAT_CAP]
    int C; const StepCtl* ctl; int t; const StepCtl* ctl_host;   // ctl != null: chain c takes no part past its own L (ctl_host mirrors ctl)
};
// (the chain-by-chain backends skip a chain past its own L on the host)
static inline bool chain_past_L(const PassArgs& a, int c) { return a.ctl != nullptr && a.t > a.ctl_host[c].L; }

class Backend {
  protected:
    const NetDev& nd;                         // the handle's descriptor (it outlives the backend)
    std::string name_;
    explicit Backend(const NetDev& nd_) : nd(nd_) {}
  public:
    virtual ~Backend() = default;
    const char* name() const { return name_.c_str(); }          // tbnn_kernel_name
    virtual int img_floats() const { return 0; }                // floats of one padded weight image (0: the kernels read theta itself)
    virtual void image_map(int* /* 2P */) const {}
    // plan n rows, (re)allocate the private buffers -- what they held is released first -- and run what the family runs once per data set.
    // *grid: entries of the statistic buffer in use; *nslab: gradient slabs per chain
    virtual int prepare(hipStream_t st, const float* dX, long n, int* grid, int* nslab) = 0;
    virtual int fwd_bwd(hipStream_t st, const PassArgs& a) = 0;
    // `nets` networks, weights P floats apart at q (device), over dX[n][d_in] -> dOut[net][d_out][n].  img: zero-padded image scratch built
    // through imgmap -- one image, or (forward_batched) one per network, img_floats apart
    virtual bool forward_batched() const { return false; }
    virtual int forward(hipStream_t st, int nets, const float* q, const float* dX, long n, float* dOut, const int* imgmap, float* img) = 0;
    // a chain's one slab IS its dense gradient row (the row-shard block then reduces nothing)
    virtual bool slab_is_grad_row() const { return false; }
    // the L leapfrog steps of a transition in ONE launch, for data sets of at most traj_max_rows rows (0: no such kernel)
    virtual long traj_max_rows() const { return 0; }
    virtual int trajectory(hipStream_t, int, const float*, long, const float*, const float*, const float*, long, float*, float*, float*, float*, const int*, double*,
                           int, float, int, const StepCtl*) { return -1; }     // (FusedOps::traj's arguments)
    virtual const FusedOps* ops() const { return nullptr; }     // the FusedOps table behind a one-kernel fused backend (tbnn_debug_stamps), else null
};

// the thread-per-row forward kernel: what a backend without a forward kernel of its own predicts with (scratch per call, synchronised
// before it goes)
static int generic_forward(const NetDev& nd, hipStream_t st, int nets, const float* q, const float* dX, long n, float* dOut) {
    const long nblk = (n + GEN_RB - 1) / GEN_RB;
    const int grid = (int)std::min<long>(nblk, 512);
    const size_t per = generic_scratch_floats(nd);
    Buf<float> scr;
    HIPCHK(scr.alloc(per * grid));
    for (int i = 0; i < nets; ++i)
        hipLaunchKernelGGL(k_forward_generic, dim3(grid), dim3(GEN_RB), 0, st, nd, q + (size_t)i * nd.P, dX, n, scr, per, dOut + (size_t)i * n * nd.d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// A one-kernel fused table (TBNN_FAMILY_NARROW: the narrow, mid and tall instantiations, ahead-of-time or registered): one gradient slab
// per workgroup, all chains of a multi-chain handle in ONE launch (gridDim.y = chain).  No private workspace.
class FusedBackend final : public Backend {
    const FusedOps* o;
    int grid_ = 0;
  public:
    FusedBackend(const NetDev& nd_, const FusedOps* ops_) : Backend(nd_), o(ops_) { name_ = o->name; }
    int img_floats() const override { return o->img_floats; }
    void image_map(int* map) const override { o->image_map(map); }
    const FusedOps* ops() const override { return o; }
    int prepare(hipStream_t, const float*, long n, int* grid, int* nslab) override {
        grid_ = o->grid(n);
        // test hook: a smaller grid puts small row counts into the many-rounds + cooperative-tail regime of the big ones
        if (const char* ge = getenv("TBNN_FAST_GRID")) { const int gg = atoi(ge); if (gg >= 1 && gg < grid_) grid_ = gg; }
        *grid = *nslab = grid_;
        return 0;
    }
    int fwd_bwd(hipStream_t st, const PassArgs& a) override {
        const ChainStride cs = {a.img_stride, a.eta_stride, a.slab_stride, a.ctl, a.t};
        if (o->launch(grid_, st, &nd, a.img, a.eta, a.X, a.Y, a.n, a.slabs, a.pitch, a.pstat, a.C, cs)) return fail(-2, name_ + ": launch failed");
        return 0;
    }
    bool forward_batched() const override { return o->nforward != nullptr; }
    int forward(hipStream_t st, int nets, const float* q, const float* dX, long n, float* dOut, const int* imgmap, float* img) override {
        if (!o->nforward) return generic_forward(nd, st, nets, q, dX, n, dOut);
        // MFMA forward of the narrow family (k_forward_fast3): every network's image, then one launch (gridDim.y = network)
        hipLaunchKernelGGL(k_make_image, dim3((nd.P + 255) / 256, nets), dim3(256), 0, st, nd.P, q, imgmap, img, (long)nd.P, (long)o->img_floats);
        const long ntiles = (n + 15) / 16, wgs = (ntiles + FAST_WAVES - 1) / FAST_WAVES;
        // one network: fill the chip; an ensemble: the networks (grid.y) do that, fewer workgroups each re-use the image more
        const long cap = nets >= 64 ? 16 : (nets >= 8 ? 64 : 256);
        const int gx = (int)std::max<long>(1, std::min<long>(wgs, cap));
        if (o->nforward(gx, nets, st, img, o->img_floats, dX, n, dOut, n * nd.d_out))
            return fail(-2, nets > 1 ? "fast3 ensemble forward launch failed" : "fast3 forward launch failed");
        HIPCHK(hipGetLastError());
        return 0;
    }
    long traj_max_rows() const override { return o->traj ? o->traj_max_rows : 0; }
    int trajectory(hipStream_t st, int C, const float* qimg, long img_stride, const float* eta, const float* X, const float* Y, long n, float* q, float* p, float* g,
                   float* gd, const int* imgmap, double* pstat, int nstat, float eps, int L, const StepCtl* ctl) override {
        return o->traj(C, st, &nd, qimg, img_stride, eta, X, Y, n, q, p, g, gd, imgmap, pstat, nstat, eps, L, ctl);
    }
};

// The wide-layer family (TBNN_FAMILY_WIDE, kernels_wide.hpp): chain + dW + reduce kernels through an activation store and two slab
// sets of its own; the reduce kernel leaves ONE slab per chain, the dense gradient row.  Chain by chain through the same store.
class WideBackend final : public Backend {
    const FusedOps* o;
    WidePlan plan{};
    Buf<float> store, slabA, slabB;
  public:
    WideBackend(const NetDev& nd_, const FusedOps* ops_) : Backend(nd_), o(ops_) { name_ = o->name; }
    int img_floats() const override { return o->img_floats; }
    void image_map(int* map) const override { o->image_map(map); }
    bool slab_is_grad_row() const override { return true; }
    int prepare(hipStream_t, const float*, long n, int* grid, int* nslab) override {
        store.reset(); slabA.reset(); slabB.reset();
        o->plan(n, &plan);
        *grid = plan.gridA; *nslab = 1;
        HIPCHK(store.alloc(plan.store_floats));
        HIPCHK(slabA.alloc(plan.slabA_floats));
        HIPCHK(slabB.alloc(plan.slabB_floats));
        return 0;
    }
    int fwd_bwd(hipStream_t st, const PassArgs& a) override {
        for (int c = 0; c < a.C; ++c) {
            if (chain_past_L(a, c)) continue;
            if (o->wlaunch(&plan, st, &nd, a.img + c * a.img_stride, a.eta + c * a.eta_stride, a.X, a.Y, a.n, store, slabA, slabB,
                           a.pstat + (size_t)c * PSTAT_CAP, a.slabs + c * a.slab_stride))
                return fail(-2, name_ + ": launch failed");
        }
        return 0;
    }
    int forward(hipStream_t st, int nets, const float* q, const float* dX, long n, float* dOut, const int* imgmap, float* img) override {
        if (!o->wforward) return generic_forward(nd, st, nets, q, dX, n, dOut);
        // MFMA forward (k_chain_wide<S, FWD>): needs the padded image of q
        for (int i = 0; i < nets; ++i) {
            hipLaunchKernelGGL(k_make_image, dim3((nd.P + 255) / 256), dim3(256), 0, st, nd.P, q + (size_t)i * nd.P, imgmap, img);
            if (o->wforward(st, &nd, img, dX, n, dOut + (size_t)i * n * nd.d_out)) return fail(-2, "wide forward launch failed");
        }
        HIPCHK(hipGetLastError());
        return 0;
    }
};

// The layered family (kernels_layered.hpp): run-time-shape MFMA kernels, activations through HBM -- any architecture.  Chain by chain
// through the same activation store; predictions on a store of their own.
class LayeredBackend final : public Backend {
    LayPlan plan{};
    Buf<float> store;
    // the forward-only store (predict / metrics / ensembles): pooled like the record buffers of tbnn_hmc_run -- network.train predicts and
    // scores every displayed epoch; everything runs in order on the chain's one stream, so the next call may overwrite it
    Buf<float> fwd;
  public:
    LayeredBackend(const NetDev& nd_, bool weighted) : Backend(nd_) {
        lay_plan_shape(nd, plan);
        name_ = "layered<" + std::to_string(nd.in[0]);
        for (int l = 0; l < nd.nl; ++l) name_ += "," + std::to_string(nd.out[l]);
        name_ += weighted ? ",weighted>" : ">";
    }
    int img_floats() const override { return plan.img_floats; }
    void image_map(int* map) const override { lay_image_map(nd, plan, map); }
    int prepare(hipStream_t st, const float* dX, long n, int* grid, int* nslab) override {
        store.reset();
        lay_plan_rows(nd, n, plan);
        *grid = plan.NP; *nslab = plan.NS;
        HIPCHK(store.alloc((size_t)plan.store_floats));
        HIPCHK(hipMemsetAsync(store, 0, (size_t)plan.store_floats * sizeof(float), st));     // dz padding: written once, here
        // a_0 = the rows in block form, once per data set
        const long tot = plan.ntiles * plan.TK[0];
        hipLaunchKernelGGL(k_lay_pack_x, dim3((int)std::min<long>(tot, 4096)), dim3(256), 0, st, dX, n, nd.d_in, plan.TK[0], plan.ntiles, store + plan.aOff[0]);
        HIPCHK(hipGetLastError());
        return 0;
    }
    int fwd_bwd(hipStream_t st, const PassArgs& a) override {
        for (int c = 0; c < a.C; ++c)
            if (!chain_past_L(a, c) && lay_launch(nd, plan, st, a.img + c * a.img_stride, a.eta + c * a.eta_stride, a.Y, a.n, store, a.slabs + c * a.slab_stride,
                                                  a.pitch, a.pstat + (size_t)c * PSTAT_CAP, a.w))
                return fail(-2, "layered kernel launch failed");
        return 0;
    }
    // the forward chain (network.predict): the rows are packed once, then any number of networks run over them
    int forward(hipStream_t st, int nets, const float* q, const float* dX, long n, float* dOut, const int* imgmap, float* img) override {
        LayPlan pp = plan;
        lay_plan_rows(nd, n, pp);
        const size_t need = (size_t)(pp.aOff[nd.nl] + pp.ntiles * 256 * pp.TM[nd.nl - 1]);
        HIPCHK(fwd.grow(need, need));
        hipLaunchKernelGGL(k_lay_pack_x, dim3((int)std::min<long>(pp.ntiles * pp.TK[0], 4096)), dim3(256), 0, st, dX, n, nd.d_in, pp.TK[0], pp.ntiles,
                           fwd + pp.aOff[0]);
        HIPCHK(hipGetLastError());
        for (int i = 0; i < nets; ++i) {
            hipLaunchKernelGGL(k_make_image, dim3((nd.P + 255) / 256), dim3(256), 0, st, nd.P, q + (size_t)i * nd.P, imgmap, img, 0L, 0L);
            lay_forward_chain(nd, pp, st, img, fwd);
            hipLaunchKernelGGL(k_lay_unpack_f, dim3((int)std::min<long>(pp.ntiles, 2048)), dim3(256), 0, st, (const float*)(fwd + pp.aOff[nd.nl]), n, pp.ntiles,
                               pp.TM[nd.nl - 1], nd.d_out, dOut + (size_t)i * n * nd.d_out);
            if (hipGetLastError() != hipSuccess) return fail(-2, "layered forward launch failed");
        }
        return 0;
    }
};

// The thread-per-row kernel (kernels_generic.hpp): no image, a scratch per workgroup.  TBNN_KERNEL_GENERIC, or TBNN_LAYERED=0 where no
// table covers the shape.
class GenericBackend final : public Backend {
    Buf<float> scratch;
    size_t perWG = 0;
    int grid_ = 0;
  public:
    GenericBackend(const NetDev& nd_, bool weighted) : Backend(nd_) { name_ = weighted ? "generic<weighted>" : "generic"; }
    int prepare(hipStream_t, const float*, long n, int* grid, int* nslab) override {
        scratch.reset();
        const long nblk = (n + GEN_RB - 1) / GEN_RB;
        grid_ = (int)std::min<long>(nblk, 512);
        *grid = *nslab = grid_;
        perWG = generic_scratch_floats(nd);
        HIPCHK(scratch.alloc(perWG * (size_t)grid_));
        return 0;
    }
    int fwd_bwd(hipStream_t st, const PassArgs& a) override {
        for (int c = 0; c < a.C; ++c)
            if (!chain_past_L(a, c))
                hipLaunchKernelGGL(k_fwd_bwd_generic, dim3(grid_), dim3(GEN_RB), 0, st, nd, a.q + (size_t)c * nd.P, a.eta + c * a.eta_stride, a.X, a.Y, a.n, scratch,
                                   perWG, a.slabs + c * a.slab_stride, a.pitch, a.pstat + (size_t)c * PSTAT_CAP, a.w);
        return 0;
    }
    int forward(hipStream_t st, int nets, const float* q, const float* dX, long n, float* dOut, const int*, float*) override {
        return generic_forward(nd, st, nets, q, dX, n, dOut);
    }
};
