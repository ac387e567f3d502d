// libtbnn: C-ABI host driver (include/tbnn.h) for the gfx950 HMC kernels.
// One handle = one chain = one device + one stream; a whole transition is
// enqueued without a host round-trip and one small record is read back.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "common.hpp"
#include "kernels_generic.hpp"
#include "kernels_hmc.hpp"
#include "kernels_hyper.hpp"
#include "kernels_layered.hpp"
#include "kernels_ensemble.hpp"
#include "kernels_optim.hpp"
#include "aot_ops.hpp"
#include <mutex>

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(-2, std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)
#define NEED(h)                                                                                \
    do { if (!(h)) return fail(-1, "null handle"); } while (0)
// entry points that address ONE chain's state have no meaning on a multi-chain handle
#define ONE_CHAIN(h, what)                                                                     \
    do { if ((h)->C > 1) return fail(-1, what ": not available on a multi-chain handle (tbnn_create_multi)"); } while (0)

// ---- owners: every buffer, event and stream the library makes has exactly one, whose destructor releases it ----
// n elements of device memory (Pinned: of pinned host memory, hipHostMalloc with the given flags).  hipFree synchronises the device:
// a buffer is released where the calls that replace it (alloc / grow / reset) or its scope (tbnn_destroy, the end of a call) say.
template <class T, bool Pinned = false>
class Buf {
    T* p_ = nullptr;
    size_t cap_ = 0;                      // elements allocated
  public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buf& operator=(Buf&& o) noexcept { reset(); std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
    ~Buf() { reset(); }
    operator T*() const { return p_; }
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; cap_ = 0;
    }
    hipError_t alloc(size_t n, unsigned flags = 0) {          // (what it held is freed first)
        reset();
        const hipError_t e = Pinned ? hipHostMalloc((void**)&p_, n * sizeof(T), flags) : hipMalloc((void**)&p_, n * sizeof(T));
        if (e == hipSuccess) cap_ = n; else p_ = nullptr;
        return e;
    }
    // a pooled buffer: kept while it holds `need` elements, else freed and `n` allocated
    hipError_t grow(size_t need, size_t n) { return cap_ >= need ? hipSuccess : alloc(n); }
};
template <class T> using PinBuf = Buf<T, true>;
// a stream or an event: created into .v, destroyed with its owner
template <class T, hipError_t (*Destroy)(T)>
struct Owned {
    T v = nullptr;
    Owned() = default;
    explicit Owned(T x) : v(x) {}
    Owned(Owned&& o) noexcept : v(std::exchange(o.v, nullptr)) {}
    ~Owned() { if (v) (void)Destroy(v); }
    operator T() const { return v; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

#include "backend.hpp"                    // the kernel families (it uses the kernel headers, Buf, fail and HIPCHK above)

struct tbnn_comm {
    ncclComm_t comm = nullptr;
    int world = 1, rank = 0;
    int device = 0;
    Buf<float> gbuf;                      // library-owned gather buffer
};

struct tbnn_ctx {
    int device = 0;
    Stream stream;                        // (the first member: destroyed after every buffer and event)
    NetDev nd{};
    uint32_t key0 = 0, key1 = 0, epoch = 0;
    int C = 1;                            // chains of this handle (tbnn_create_multi): every per-chain buffer is a [C][...] array, the per-chain
    uint32_t seed_hi = 0;                 // kernels run with gridDim.y = C; chain c draws from the Philox key (seed, chain_id + c)
    std::unique_ptr<Backend> be;          // the kernel family of this shape (backend.hpp: select_kernels), with its plan and private buffers
    // data: the rows tbnn_set_data staged (Xown / Yown), or the caller's (tbnn_set_data_device: borrowed)
    Buf<float> Xown, Yown; const float* dX = nullptr; const float* dY = nullptr; long n = 0;
    // row weights (tbnn_set_row_weights): [n x d_out targets | n weights] in one buffer -- what the kernels read as Y while weights are
    // set (kernels_fast.hpp: row_weight) -- and W = their sum in fp64; null / 0: none
    Buf<float> dYw; double wsum = 0.0;
    // the degrees of freedom tbnn_ensemble_loglik / tbnn_ensemble_loo judge under TBNN_LIK_STUDENT_T with on a handle of another likelihood
    // (tbnn_set_lik_df; 0: not set -- a Student-t handle's own are nd.lik_df)
    float ens_df = 0.f;
    // TBNN_LIK_POISSON: C = sum_i w_i sum_k lgamma(y_ik + 1) of the staged rows (stage_lik_const; all chains share it); TBNN_LIK_NEG_BINOMIAL:
    // ... (lgamma(y_ik + 1) + lgamma(r) - lgamma(y_ik + r)); TBNN_LIK_GAMMA: ... (lgamma(a) - a log a - (a - 1) log y_ik); TBNN_LIK_WEIBULL: ... -d_ik (log k + (k - 1) log |y_ik|); 0 otherwise
    double lik_c = 0.0;
    int want = TBNN_KERNEL_AUTO;          // tbnn_net_desc::kernel (the re-selection of tbnn_set_row_weights follows it)
    // validation data (network.py:47-51) and the prediction buffer of tbnn_predict / tbnn_metrics
    Buf<float> dXv, dYv; long nv = 0;
    Buf<float> fbuf; Buf<double> mpart;
    // chain state
    Buf<float> q_cur, g_cur, q, p, g, eta;
    Buf<float> p0_inj, logu_inj, tmp;
    Buf<float> gd, gd_cur, eta_prev;      // data-term gradient of the proposal / current state; eta before a hyper step
    bool cur_valid = false;               // (logp, grad, stat) cached at q_cur for the current eta/data
    bool q_img_valid = false;             // h->qimg mirrors h->q (maintained by k_update)
    // fused-pass workspace common to all families (alloc_workspace): grid = statistic entries in use, nslab = gradient slabs k_update reduces
    int grid = 0, pitch = 0, nslab = 0; Buf<float> slabs; Buf<double> pstat;
    // row-sharded chain (tbnn_set_row_shard): all-reduce of the dense data-term gradient row + statistic
    tbnn_comm* shard = nullptr; long n_total = 0; Buf<float> grow; Buf<double> pstat_red;
    Buf<double> shard_buf;                // the all-reduce operand: P gradient values + the statistic, as doubles
    Buf<int> imgmap; Buf<float> qimg, qimg_cur; int img_floats = 0;   // padded weight images of a backend that reads them (be->img_floats())
    float* pin_dev = nullptr;              // device-side address of pin
    PinBuf<float> pin;                     // pinned staging for the per-epoch state read-back (P + H floats): a 22-KB D2H copy
                                           // into pageable memory costs ~180 us, through pinned memory ~15 us
    Buf<Scal> sc; PinBuf<Scal> sc_host; Buf<Scal> sc_out;   // sc_out: device copy for host
    Buf<double> trace;
    Buf<Scal> d_recs; PinBuf<Scal> h_recs;                  // tbnn_hmc_run: per-epoch records (pooled)
    Event ev0, ev1;
    int profile = 0; long launch_no = 0;   // profile: event pair around every profile-th fwd+bwd launch
    std::vector<Event> pev; size_t pev_used = 0;        // pooled events: created once, re-used after every drain (no allocator in the timed loop)
    std::vector<int> pev_div;                           // leapfrog steps the pair's launch covered (1: a fused pass; L: a trajectory launch)
    const char* last_path = "none";                     // which kernels ran the last transition's leapfrog steps (tbnn_last_transition_path)
    // hyper workspace
    Buf<float> hyp_ws;
    // per-chain step control (tbnn_hmc_step_each / tbnn_hyper_step_each): [C] on the device, staged through pinned memory
    Buf<StepCtl> ctl; PinBuf<StepCtl> ctl_host; Buf<float> epsh; PinBuf<float> epsh_host;
    // optimiser state (tbnn_optimize; allocated on its first call): Adam moments, the last total gradient and the best weights as [C][P],
    // the per-chain record k_optim_logp keeps, the objective trace [C][n_checks] (pooled), and the step counter t since the last reset
    Buf<float> opt_m, opt_v, opt_vhat, opt_g, opt_qbest; Buf<OptChain> opt_oc; PinBuf<OptChain> opt_oc_host; Buf<double> opt_trace;
    long opt_t = 0; bool opt_live = false;
    bool merge_ends = true;                // TBNN_MERGE_ENDS (read at tbnn_create): decision + record + commit in one k_energy launch
    bool traj = true;                      // TBNN_TRAJ (read at tbnn_create; 0: off): whole trajectories of small problems in one launch (kernels_traj.hpp)
};

extern "C" const char* tbnn_last_error(void) { return g_err.c_str(); }
extern "C" int tbnn_abi_version(void) { return TBNN_ABI_VERSION; }
// hash of the sources this library was built from (tensorbnn_amd/build.py: kernel headers, translation units, include/tbnn.h,
// compiler flags): what ties a committed rocprofv3 summary under profiles/ to the library bench.py has loaded
#ifndef TBNN_BUILD_ID
#define TBNN_BUILD_ID "unknown"
#endif
extern "C" const char* tbnn_build_id(void) { return TBNN_BUILD_ID; }
extern "C" int tbnn_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(-2, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return n;
}

// the TBNN_LIK_* values (4, 6 and 7 are not among them: include/tbnn.h)
static bool lik_known(int lik) {
    return (lik >= TBNN_LIK_GAUSSIAN && lik <= TBNN_LIK_CATEGORICAL) || lik == TBNN_LIK_POISSON || lik == TBNN_LIK_STUDENT_T || lik == TBNN_LIK_NEG_BINOMIAL ||
           lik == TBNN_LIK_HETERO_GAUSSIAN || lik == TBNN_LIK_GAMMA || lik == TBNN_LIK_WEIBULL;
}
// the count likelihoods: targets finite and >= 0, the last layer's output a log-rate, the constant of stage_lik_const
static bool lik_counts(int lik) { return lik == TBNN_LIK_POISSON || lik == TBNN_LIK_NEG_BINOMIAL; }
// the likelihoods whose log-probability has a constant that depends on the targets (stage_lik_const): the count ones, TBNN_LIK_GAMMA
// (targets finite and > 0) and TBNN_LIK_WEIBULL (targets signed: nonzero, 2^-100 <= |y| <= 2^100)
static bool lik_has_const(int lik) { return lik_counts(lik) || lik == TBNN_LIK_GAMMA || lik == TBNN_LIK_WEIBULL; }
// degrees of freedom a Student-t term can be formed with (and a dispersion a negative-binomial one can)
static bool df_ok(float df) { return df > 0.f && df < INFINITY; }

static int build_netdev(const tbnn_net_desc* d, NetDev& nd) {
    if (!d || !d->layers) return fail(-1, "null descriptor");
    if (d->n_layers < 1 || d->n_layers > TBNN_MAX_LAYERS) return fail(-1, "n_layers must be in [1,16]");
    memset(&nd, 0, sizeof(nd));
    nd.nl = d->n_layers;
    int off = 0, so = 0, mw = 0;
    for (int l = 0; l < nd.nl; ++l) {
        const tbnn_layer_desc& L = d->layers[l];
        if (L.in_dim < 1 || L.out_dim < 1) return fail(-1, "layer dims must be >= 1");
        if (l > 0 && L.in_dim != d->layers[l - 1].out_dim) return fail(-1, "layer dims do not chain");
        if (L.act < TBNN_ACT_NONE || L.act > TBNN_ACT_ELU) return fail(-1, "unknown activation");
        if (L.prior != TBNN_PRIOR_CAUCHY && L.prior != TBNN_PRIOR_GAUSSIAN) return fail(-1, "unknown prior");
        nd.in[l] = L.in_dim; nd.out[l] = L.out_dim; nd.act[l] = L.act; nd.prior[l] = L.prior;
        nd.offW[l] = off; off += L.in_dim * L.out_dim;
        nd.offB[l] = off; off += L.out_dim;
        nd.actOff[l] = so; so += L.out_dim;
        mw = std::max(mw, std::max(L.in_dim, L.out_dim));
    }
    if (!lik_known(d->likelihood)) return fail(-1, "unknown likelihood");
    if (d->likelihood == TBNN_LIK_POISSON && nd.act[nd.nl - 1] != TBNN_ACT_NONE)
        return fail(-1, "the Poisson likelihood takes the last layer's outputs as log-rates (log link): the last layer must carry no activation");
    if (d->likelihood == TBNN_LIK_CATEGORICAL) {
        if (nd.out[nd.nl - 1] < 2) return fail(-1, "the categorical likelihood needs at least 2 outputs (one logit per class)");
        if (nd.act[nd.nl - 1] != TBNN_ACT_NONE)
            return fail(-1, "the categorical likelihood takes the last layer's outputs as logits: the last layer must carry no activation");
    }
    if (d->likelihood == TBNN_LIK_NEG_BINOMIAL) {
        if (nd.act[nd.nl - 1] != TBNN_ACT_NONE)
            return fail(-1, "the negative-binomial likelihood takes the last layer's outputs as log-rates (log link): the last layer must carry no activation");
        if (!df_ok(d->lik_df)) return fail(-1, "the negative-binomial likelihood needs lik_df (its dispersion r) finite and > 0");
    }
    if (d->likelihood == TBNN_LIK_GAMMA) {
        if (nd.act[nd.nl - 1] != TBNN_ACT_NONE)
            return fail(-1, "the Gamma likelihood takes the last layer's outputs as log-means (log link): the last layer must carry no activation");
        if (!df_ok(d->lik_df)) return fail(-1, "the Gamma likelihood needs lik_df (its shape a) finite and > 0");
    }
    if (d->likelihood == TBNN_LIK_WEIBULL) {
        if (nd.act[nd.nl - 1] != TBNN_ACT_NONE)
            return fail(-1, "the Weibull likelihood takes the last layer's outputs as log-scales (log link): the last layer must carry no activation");
        if (!df_ok(d->lik_df)) return fail(-1, "the Weibull likelihood needs lik_df (its shape k) finite and > 0");
    }
    if (d->likelihood == TBNN_LIK_HETERO_GAUSSIAN) {
        if (nd.out[nd.nl - 1] != 2) return fail(-1, "the heteroscedastic Gaussian likelihood needs exactly 2 outputs: mean and log-sd");
        if (nd.act[nd.nl - 1] != TBNN_ACT_NONE)
            return fail(-1, "the heteroscedastic Gaussian likelihood takes the last layer's outputs as mean and log-sd: the last layer must carry no activation");
    }
    nd.P = off;
    nd.lik = d->likelihood;
    nd.H = 4 * nd.nl + (nd.lik == TBNN_LIK_GAUSSIAN ? 1 : 0);
    nd.d_in = nd.in[0]; nd.d_out = nd.out[nd.nl - 1];
    nd.sumOut = so; nd.maxW = mw;
    nd.fixed_sd = d->fixed_sd;
    if (nd.lik == TBNN_LIK_FIXED_GAUSSIAN && !(d->fixed_sd > 0.f)) return fail(-1, "fixed_sd must be > 0");
    if (nd.lik == TBNN_LIK_STUDENT_T) {
        if (!(d->fixed_sd > 0.f)) return fail(-1, "the Student-t likelihood takes its scale from fixed_sd, which must be > 0");
        if (!df_ok(d->lik_df)) return fail(-1, "the Student-t likelihood needs lik_df (its degrees of freedom) finite and > 0");
        nd.lik_df = d->lik_df;
    }
    if (nd.lik == TBNN_LIK_NEG_BINOMIAL || nd.lik == TBNN_LIK_GAMMA || nd.lik == TBNN_LIK_WEIBULL) nd.lik_df = d->lik_df;
    return 0;
}

// ---- kernel libraries compiled at run time for shapes outside the ahead-of-time registries ----
static std::mutex g_jit_mu;
static std::vector<FusedOps*> g_jit;              // never freed: handles keep pointers into it
static const FusedOps* find_jit(const NetDev& nd, bool weighted = false) {
    std::lock_guard<std::mutex> lk(g_jit_mu);
    for (const FusedOps* o : g_jit) if (fused_ops_match(*o, nd, weighted)) return o;
    return nullptr;
}
static bool env_off(const char* name) { const char* v = getenv(name); return v && atoi(v) == 0; }
// the FusedOps table for this network, in selection order: the ahead-of-time narrow, mid and wide instantiations, a run-time
// registered library, the ahead-of-time tall-fan-in instantiations.  weighted (row weights set): a registered weighted library only --
// no ahead-of-time table is weighted
static const FusedOps* find_ops(const NetDev& nd, bool mid_on, bool weighted = false) {
    if (weighted) return env_off("TBNN_REGISTERED") ? nullptr : find_jit(nd, true);
    const FusedOps* o = narrow_find(nd);
    if (!o && mid_on) o = mid_find(nd);
    if (!o) o = wide_find(nd);
    // TBNN_REGISTERED=0 (the layered family's tests): tbnn_create ignores kernel libraries registered earlier in the process
    if (!o && !env_off("TBNN_REGISTERED")) o = find_jit(nd);
    // TBNN_TALL=0 (diagnostic / A-B runs, the layered family's tests): shapes the tall-fan-in registry covers take the layered path
    if (!o && !env_off("TBNN_TALL")) o = tall_find(nd);
    return o;
}
extern "C" int tbnn_register_kernel_lib(const char* path) {
    if (!path) return fail(-1, "null path");
    void* lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!lib) return fail(-6, std::string("dlopen: ") + dlerror());
    typedef int (*ops_fn)(FusedOps*);
    ops_fn fn = (ops_fn)dlsym(lib, "tbnn_jit_ops");
    if (!fn) { dlclose(lib); return fail(-6, std::string(path) + " does not export tbnn_jit_ops"); }
    FusedOps* o = new (std::nothrow) FusedOps();
    if (!o) return fail(-4, "out of host memory");
    memset(o, 0, sizeof(*o));
    if (fn(o) != 0 || o->abi != TBNN_JIT_ABI || (o->family != TBNN_FAMILY_NARROW && o->family != TBNN_FAMILY_WIDE)) {
        delete o; dlclose(lib);
        return fail(-6, std::string(path) + ": kernel table rejected (ABI mismatch?)");
    }
    std::lock_guard<std::mutex> lk(g_jit_mu);
    g_jit.push_back(o);
    return 0;
}
// 0: generic kernel only; 1: ahead-of-time narrow MFMA kernel; 2: ahead-of-time wide path; 3: registered library
extern "C" int tbnn_fused_kernel_available(const tbnn_net_desc* desc) {
    NetDev nd;
    int rc = build_netdev(desc, nd);
    if (rc) return rc;
    const FusedOps* o = find_ops(nd, true);
    if (!o) return 0;
    if (o == find_jit(nd)) return 3;
    return o->family == TBNN_FAMILY_WIDE ? 2 : 1;
}

static void default_eta(const NetDev& nd, std::vector<float>& eta) {
    eta.assign(nd.H, 0.f);
    for (int l = 0; l < nd.nl; ++l) {
        if (nd.prior[l] == TBNN_PRIOR_CAUCHY) {          // layer.py:136-158
            eta[4 * l + 1] = sqrtf(0.5f); eta[4 * l + 3] = sqrtf(0.5f);
        } else {                                         // layer.py:316-339
            eta[4 * l + 1] = 1.f; eta[4 * l + 3] = 1.f;
        }
    }
    if (nd.lik == TBNN_LIK_GAUSSIAN) eta[nd.H - 1] = sqrtf(0.1f);   // GaussianLikelihood(sd=0.1)
}

extern "C" int tbnn_destroy(tbnn_handle h) {
    if (!h) return 0;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    delete h;                             // (its owners free the buffers and events, then the stream)
    return 0;
}

static int create_impl(const tbnn_net_desc* desc, int device, uint64_t seed, uint32_t chain_id, int n_chains, tbnn_handle* out);
extern "C" int tbnn_create(const tbnn_net_desc* desc, int device, uint64_t seed, uint32_t chain_id, tbnn_handle* out) {
    return create_impl(desc, device, seed, chain_id, 1, out);
}
// Several independent chains of one network on ONE device behind one handle (SURVEY 8(e) puts one chain on each GPU; small
// problems -- the reference's own examples -- leave most of a GPU idle and are bound by launch latency): chain c is exactly the chain
// tbnn_create(..., chain_id + c) would be, and the per-chain kernels of all of them run as ONE launch with gridDim.y = n_chains.
extern "C" int tbnn_create_multi(const tbnn_net_desc* desc, int device, uint64_t seed, uint32_t chain_id, int32_t n_chains, tbnn_handle* out) {
    if (n_chains < 1 || n_chains > 1024) return fail(-1, "n_chains must be in [1, 1024]");
    {   // element counts of the [chains][P] arrays are ints in the copy / commit kernels: refuse what would not fit
        NetDev nd;
        int rc = build_netdev(desc, nd);
        if (rc) return rc;
        if ((long long)n_chains * (long long)nd.P > 0x7FFFFFFFLL) return fail(-1, "n_chains x parameter count exceeds 2^31 - 1");
    }
    return create_impl(desc, device, seed, chain_id, n_chains, out);
}
extern "C" int tbnn_chain_count(tbnn_handle h) { NEED(h); return h->C; }
// the handle's backend: a FusedOps table (weighted: a registered weighted one), else the layered family (TBNN_KERNEL_AUTO), else the
// thread-per-row kernel; with the weight image map and the padded images it reads.  tbnn_create, and tbnn_set_row_weights /
// tbnn_set_data when the weights come or go (the caller re-allocates the fused-pass workspace when data are staged).  A refusal
// (TBNN_KERNEL_FAST without a table) is decided before the handle is touched: it keeps its backend, images and workspace.
static int select_kernels(tbnn_ctx* h, bool weighted) {
    const NetDev& nd = h->nd;
    const int want = h->want;
    // TBNN_MID=0 (diagnostic / A-B runs): shapes both families cover take the wide path (two kernels through HBM)
    const FusedOps* ops = find_ops(nd, !env_off("TBNN_MID"), weighted);
    if (want == TBNN_KERNEL_FAST && !ops)
        return fail(-1, weighted ? "TBNN_KERNEL_FAST requested but no weighted kernel library is registered for this shape (jit.ensure_registered(..., weighted=True))"
                                 : "TBNN_KERNEL_FAST requested but no specialised kernel covers this shape");
    h->qimg.reset(); h->qimg_cur.reset(); h->imgmap.reset();
    h->be.reset();                                      // (with its workspace: never two backends' at once)
    h->img_floats = 0; h->q_img_valid = false; h->cur_valid = false;
    if (ops && (want == TBNN_KERNEL_AUTO || want == TBNN_KERNEL_FAST)) {
        if (ops->family == TBNN_FAMILY_WIDE) h->be.reset(new (std::nothrow) WideBackend(nd, ops));
        else h->be.reset(new (std::nothrow) FusedBackend(nd, ops));
    } else if (want == TBNN_KERNEL_AUTO && !env_off("TBNN_LAYERED")) {
        // no shape-specialised kernel (and none registered at run time): the layered MFMA family takes any architecture
        h->be.reset(new (std::nothrow) LayeredBackend(nd, weighted));
    } else {
        h->be.reset(new (std::nothrow) GenericBackend(nd, weighted));     // TBNN_KERNEL_GENERIC, or TBNN_LAYERED=0
    }
    if (!h->be) return fail(-4, "out of host memory");
    h->img_floats = h->be->img_floats();
    if (h->img_floats) {
        std::vector<int> map(2 * (size_t)nd.P);
        h->be->image_map(map.data());
        const size_t imgs = (size_t)h->C * (size_t)h->img_floats;
        HIPCHK(h->imgmap.alloc(map.size()));
        HIPCHK(hipMemcpy(h->imgmap, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(h->qimg.alloc(imgs));
        HIPCHK(h->qimg_cur.alloc(imgs));
        HIPCHK(hipMemset(h->qimg, 0, imgs * sizeof(float)));       // padding stays zero for ever
        HIPCHK(hipMemset(h->qimg_cur, 0, imgs * sizeof(float)));
    }
    return 0;
}

static int create_impl(const tbnn_net_desc* desc, int device, uint64_t seed, uint32_t chain_id, int n_chains, tbnn_handle* out) {
    if (!out) return fail(-1, "null out");
    *out = nullptr;
    NetDev nd;
    int rc = build_netdev(desc, nd);
    if (rc) return rc;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(-3, "no HIP device visible: libtbnn has no CPU fallback (the HMC path runs on gfx950 only)");
    if (device < 0 || device >= ndev) return fail(-1, "device index out of range");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(-3, std::string("device is ") + prop.gcnArchName + ", libtbnn is built for gfx950 only");
    HIPCHK(hipSetDevice(device));
    // the new handle is tbnn_destroy'ed on every early return, and handed out at the end
    std::unique_ptr<tbnn_ctx, int (*)(tbnn_handle)> owner(new (std::nothrow) tbnn_ctx(), tbnn_destroy);
    tbnn_ctx* h = owner.get();
    if (!h) return fail(-4, "out of host memory");
    h->device = device; h->nd = nd; h->C = n_chains;
    // Philox key = (seed, chain_id); the high seed word is folded into the key
    h->key0 = (uint32_t)(seed & 0xFFFFFFFFull);
    h->seed_hi = (uint32_t)(seed >> 32);
    h->key1 = chain_id ^ h->seed_hi;
    const size_t NC = (size_t)n_chains;
    HIPCHK(hipStreamCreateWithFlags(&h->stream.v, hipStreamNonBlocking));
    const size_t PN = NC * (size_t)nd.P, HN = NC * (size_t)nd.H;    // per-chain arrays: [C][P], [C][H] (one chain: [P], [H])
    HIPCHK(h->q_cur.alloc(PN)); HIPCHK(h->g_cur.alloc(PN)); HIPCHK(h->q.alloc(PN));
    HIPCHK(h->p.alloc(PN)); HIPCHK(h->g.alloc(PN));
    HIPCHK(h->p0_inj.alloc((size_t)std::max(nd.P, nd.H)));   // injected momentum of either transition (H > P for tiny networks)
    HIPCHK(h->tmp.alloc(PN + HN));
    HIPCHK(h->eta.alloc(HN));
    HIPCHK(h->eta_prev.alloc(HN));
    HIPCHK(h->gd.alloc(PN)); HIPCHK(h->gd_cur.alloc(PN));
    HIPCHK(h->logu_inj.alloc(1));
    HIPCHK(h->sc.alloc(NC)); HIPCHK(h->sc_out.alloc(NC));
    HIPCHK(h->sc_host.alloc(NC));
    HIPCHK(h->pin.alloc(PN + HN, hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer((void**)&h->pin_dev, h->pin, 0));
    HIPCHK(hipMemset(h->sc, 0, NC * sizeof(Scal)));
    HIPCHK(hipMemset(h->q_cur, 0, PN * sizeof(float)));
    HIPCHK(hipEventCreate(&h->ev0.v)); HIPCHK(hipEventCreate(&h->ev1.v));
    HIPCHK(h->hyp_ws.alloc(NC * hyper_ws_bytes(nd) / sizeof(float)));
    HIPCHK(h->ctl.alloc(NC)); HIPCHK(h->ctl_host.alloc(NC));
    HIPCHK(h->epsh.alloc(NC)); HIPCHK(h->epsh_host.alloc(NC));
    std::vector<float> eta1, eta; default_eta(nd, eta1);
    for (size_t c = 0; c < NC; ++c) eta.insert(eta.end(), eta1.begin(), eta1.end());
    HIPCHK(hipMemcpy(h->eta, eta.data(), eta.size() * sizeof(float), hipMemcpyHostToDevice));
    // fused-kernel variant
    h->want = desc->kernel;
    if (const int rc = select_kernels(h, false)) return rc;
    { const char* e1 = getenv("TBNN_FAST_SINGLE"); if (e1 && atoi(e1)) h->nd.reserved_flags |= 1; }
    { const char* e2 = getenv("TBNN_MERGE_ENDS"); h->merge_ends = !(e2 && atoi(e2) == 0); }
    { const char* e3 = getenv("TBNN_TRAJ"); h->traj = !(e3 && atoi(e3) == 0); }
    const char* env = getenv("TBNN_PROFILE_FWDBWD");
    h->profile = env ? atoi(env) : 0;
    *out = owner.release();
    return 0;
}

extern "C" int tbnn_param_count(tbnn_handle h) { NEED(h); return h->nd.P; }
extern "C" int tbnn_hyper_count(tbnn_handle h) { NEED(h); return h->nd.H; }
extern "C" const char* tbnn_kernel_name(tbnn_handle h) { return h && h->be ? h->be->name() : ""; }
extern "C" const char* tbnn_last_transition_path(tbnn_handle h) { return h ? h->last_path : ""; }
extern "C" int tbnn_debug_stat_partials(tbnn_handle h) { NEED(h); return h->grid; }
extern "C" int tbnn_set_profiling(tbnn_handle h, int stride) {
    NEED(h);
    h->profile = stride > 0 ? stride : 0;
    if (h->profile) {                       // fill the event pool now, outside any timed loop
        HIPCHK(hipSetDevice(h->device));
        // 256 pairs: more than any tbnn_hmc_run of bench.py profiles between two drains
        while (h->pev.size() < 512) { hipEvent_t e = nullptr; HIPCHK(hipEventCreate(&e)); h->pev.emplace_back(e); }
    }
    return 0;
}
extern "C" int tbnn_set_epoch(tbnn_handle h, uint32_t epoch) { NEED(h); h->epoch = epoch; return 0; }

// (re)allocate the fused-pass workspace for n rows: the backend's own, then what all families share
static int alloc_workspace(tbnn_ctx* h, long n) {
    const NetDev& nd = h->nd;
    h->slabs.reset(); h->pstat.reset();
    if (const int rc = h->be->prepare(h->stream, h->dX, n, &h->grid, &h->nslab)) return rc;
    h->pitch = (nd.P + 3) & ~3;                  // float4-readable slabs
    const size_t slab_floats = (size_t)h->C * h->nslab * h->pitch;
    HIPCHK(h->slabs.alloc(slab_floats));                                             // [C][nslab][pitch]
    HIPCHK(hipMemset(h->slabs, 0, slab_floats * sizeof(float)));
    if (h->grid > PSTAT_CAP) return fail(-2, "grid exceeds PSTAT_CAP");
    HIPCHK(h->pstat.alloc((size_t)h->C * PSTAT_CAP));                                // [C][PSTAT_CAP]
    HIPCHK(hipMemset(h->pstat, 0, (size_t)h->C * PSTAT_CAP * sizeof(double)));      // entries >= grid stay zero
    HIPCHK(h->pstat_red.alloc(PSTAT_CAP));
    HIPCHK(hipMemset(h->pstat_red, 0, (size_t)PSTAT_CAP * sizeof(double)));
    HIPCHK(h->grow.alloc((size_t)h->pitch));
    HIPCHK(h->shard_buf.alloc((size_t)nd.P + 1));
    return 0;
}

// Poisson, negative binomial, Gamma and Weibull (TBNN_LIK_POISSON, TBNN_LIK_NEG_BINOMIAL, TBNN_LIK_GAMMA, TBNN_LIK_WEIBULL; any other likelihood: C = 0, nothing runs): the constant C of the n rows dY (device) under the row weights dw
// (device, null: none) -- k_pois_const, its partials added here in block order -- and the refusal of targets that are not counts (Gamma: not finite and > 0, or above 2^100; Weibull: NaN, zero or |y| outside [2^-100, 2^100]).  Called
// by everything that stages rows or weights BEFORE it changes the handle: a refusal leaves the handle as it was.
static int stage_lik_const(tbnn_ctx* h, const std::string& who, const float* dY, const float* dw, long n, double* C) {
    *C = 0.0;
    if (!lik_has_const(h->nd.lik)) return 0;
    const bool nb = h->nd.lik == TBNN_LIK_NEG_BINOMIAL, gam = h->nd.lik == TBNN_LIK_GAMMA, wei = h->nd.lik == TBNN_LIK_WEIBULL;
    Buf<double> part;
    HIPCHK(part.alloc(2 * LIKC_BLOCKS));
    hipLaunchKernelGGL(k_pois_const, dim3(LIKC_BLOCKS), dim3(256), 0, h->stream, dY, dw, n, h->nd.d_out, (double*)part, nb || gam || wei ? (double)h->nd.lik_df : 0.0,
                       gam ? (int)LIKC_GAMMA : wei ? (int)LIKC_WEIBULL : (int)LIKC_COUNTS);
    HIPCHK(hipGetLastError());
    double host[2 * LIKC_BLOCKS];
    HIPCHK(hipMemcpyAsync(host, part, sizeof(host), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    double c = 0.0, bad = 0.0;
    for (int b = 0; b < LIKC_BLOCKS; ++b) { c += host[2 * b]; bad += host[2 * b + 1]; }
    if (bad > 0.0 && gam)
        return fail(-1, who + ": " + std::to_string((long long)bad) + " target(s) are zero, negative, not finite or above the ceiling: under the Gamma likelihood targets must be finite and > 0 and at most 2^100 (1.2676506e30)");
    if (bad > 0.0 && wei)
        return fail(-1, who + ": " + std::to_string((long long)bad) + " target(s) are zero, not finite or out of range: under the Weibull likelihood a target is a signed time (y > 0 an event, y < 0 censored at |y|), finite, nonzero and 2^-100 <= |y| <= 2^100");
    if (bad > 0.0)
        return fail(-1, who + ": " + std::to_string((long long)bad) + " target(s) are negative or not finite: the " + (nb ? "negative-binomial" : "Poisson") + " likelihood takes counts (finite, >= 0)");
    *C = c;
    return 0;
}

// new rows: the row weights (which were the old rows') are dropped, and the unweighted kernels selected again
static int drop_row_weights(tbnn_ctx* h) {
    if (!h->dYw) return 0;
    h->dYw.reset(); h->wsum = 0.0;
    return select_kernels(h, false);
}

extern "C" int tbnn_set_data_device(tbnn_handle h, const float* dX, const float* dY, int64_t n) {
    NEED(h);
    if (!dX || !dY || n < 1) return fail(-1, "set_data: null pointer or n < 1");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    double C = 0.0;
    if (const int rc = stage_lik_const(h, "set_data", dY, nullptr, (long)n, &C)) return rc;
    h->Xown.reset(); h->Yown.reset();
    h->dX = dX; h->dY = dY; h->n = (long)n; h->lik_c = C;
    h->cur_valid = false;
    if (const int rc = drop_row_weights(h)) return rc;
    return alloc_workspace(h, (long)n);
}

extern "C" int tbnn_set_data(tbnn_handle h, const float* X, const float* Y, int64_t n) {
    NEED(h);
    if (!X || !Y || n < 1) return fail(-1, "set_data: null pointer or n < 1");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t nx = (size_t)n * h->nd.d_in, ny = (size_t)n * h->nd.d_out;
    double C = 0.0;
    Buf<float> newY;
    if (lik_has_const(h->nd.lik)) {
        // the targets are staged and judged first: refused ones leave the handle with the rows it had
        HIPCHK(newY.alloc(ny));
        HIPCHK(hipMemcpy(newY, Y, ny * sizeof(float), hipMemcpyHostToDevice));
        if (const int rc = stage_lik_const(h, "set_data", newY, nullptr, (long)n, &C)) return rc;
    }
    if (h->Xown) { h->Xown.reset(); h->Yown.reset(); h->dX = h->dY = nullptr; }
    HIPCHK(h->Xown.alloc(nx));
    HIPCHK(hipMemcpy(h->Xown, X, nx * sizeof(float), hipMemcpyHostToDevice));
    if (newY) h->Yown = std::move(newY);
    else {
        HIPCHK(h->Yown.alloc(ny));
        HIPCHK(hipMemcpy(h->Yown, Y, ny * sizeof(float), hipMemcpyHostToDevice));
    }
    h->dX = h->Xown; h->dY = h->Yown; h->n = (long)n; h->lik_c = C;
    h->cur_valid = false;
    if (const int rc = drop_row_weights(h)) return rc;
    return alloc_workspace(h, (long)n);
}

// Row weights (include/tbnn.h): validated on the host, W summed in fp64, staged behind a copy of the targets as [Y | w] -- the buffer
// every kernel reads as Y while they are set -- and the kernels re-selected: a registered weighted table, else the layered family
// (the thread-per-row kernel under TBNN_KERNEL_GENERIC / TBNN_LAYERED=0).  null: back to the unweighted kernels.
extern "C" int tbnn_set_row_weights(tbnn_handle h, const float* w, int64_t n) {
    NEED(h);
    if (!h->dX) return fail(-1, "set_row_weights: tbnn_set_data has not been called");
    if (h->shard) return fail(-1, "set_row_weights: not on a row-sharded handle (tbnn_set_row_shard): weighted row sharding needs the weight sum of all ranks");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!w) {
        double C = 0.0;
        if (const int rc = stage_lik_const(h, "set_row_weights", h->dY, nullptr, h->n, &C)) return rc;
        h->lik_c = C; h->cur_valid = false;               // (a cached logp_cur carries the constant it was formed with)
        if (const int rc = drop_row_weights(h)) return rc;
        return alloc_workspace(h, h->n);
    }
    if (n != h->n) return fail(-1, "set_row_weights: n = " + std::to_string((long long)n) + " does not match the " + std::to_string(h->n) + " staged rows");
    double W = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(w[i])) return fail(-1, "set_row_weights: weight " + std::to_string((long long)i) + " is not finite");
        if (w[i] < 0.f) return fail(-1, "set_row_weights: weight " + std::to_string((long long)i) + " is negative");
        W += (double)w[i];
    }
    if (!(W > 0.0)) return fail(-1, "set_row_weights: all weights are zero");
    const size_t ny = (size_t)h->n * h->nd.d_out;
    Buf<float> buf;
    HIPCHK(buf.alloc(ny + (size_t)h->n));
    if (hipMemcpy(buf, h->dY, ny * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess ||
        hipMemcpy(buf + ny, w, (size_t)h->n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail(-2, "set_row_weights: staging the weights failed");
    double C = 0.0;
    if (const int rc = stage_lik_const(h, "set_row_weights", buf, buf + ny, h->n, &C)) return rc;
    // the weighted kernels first: a refusal (TBNN_KERNEL_FAST and no weighted table) leaves the handle as it was -- its kernels, weights
    // and workspace; any other failure re-selects the kernels of the weights the handle keeps
    int rc = select_kernels(h, true);
    if (rc == 0) rc = alloc_workspace(h, h->n);
    if (rc) {
        buf.reset();                                   // (before the handle's own kernels and workspace are made again)
        const std::string err = g_err;
        select_kernels(h, h->dYw != nullptr);          // (the kernels of the weights the handle keeps: they were selected before)
        alloc_workspace(h, h->n);
        g_err = err;
        return rc;
    }
    h->dYw = std::move(buf); h->wsum = W; h->lik_c = C;
    h->cur_valid = false;
    return 0;
}

extern "C" int tbnn_set_state(tbnn_handle h, const float* theta) {
    NEED(h); if (!theta) return fail(-1, "null theta");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->q_cur, theta, (size_t)h->C * h->nd.P * sizeof(float), hipMemcpyHostToDevice, h->stream));     // [C][P]
    HIPCHK(hipStreamSynchronize(h->stream));
    h->cur_valid = false;
    return 0;
}
extern "C" int tbnn_get_state(tbnn_handle h, float* theta) {
    NEED(h); if (!theta) return fail(-1, "null theta");
    HIPCHK(hipSetDevice(h->device));
    // a kernel writes theta straight into the (device-mapped) pinned buffer: a D2H copy engine transfer of this size
    // has ~160 us of latency, the zero-copy store a few us
    const int PC = h->C * h->nd.P;
    hipLaunchKernelGGL(k_copy_f32, dim3((PC + 255) / 256), dim3(256), 0, h->stream, PC, (const float*)h->q_cur, h->pin_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(theta, h->pin, (size_t)PC * sizeof(float));
    return 0;
}
extern "C" int tbnn_set_hypers(tbnn_handle h, const float* eta) {
    NEED(h); if (!eta) return fail(-1, "null eta");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->eta, eta, (size_t)h->C * h->nd.H * sizeof(float), hipMemcpyHostToDevice, h->stream));        // [C][H]
    HIPCHK(hipStreamSynchronize(h->stream));
    h->cur_valid = false;
    return 0;
}
extern "C" int tbnn_get_hypers(tbnn_handle h, float* eta) {
    NEED(h); if (!eta) return fail(-1, "null eta");
    HIPCHK(hipSetDevice(h->device));
    float* stage = h->pin + (size_t)h->C * h->nd.P;
    HIPCHK(hipMemcpyAsync(stage, h->eta, (size_t)h->C * h->nd.H * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(eta, stage, (size_t)h->C * h->nd.H * sizeof(float));
    return 0;
}

// ---- RCCL, resolved at run time (no link-time dependency: single-GPU users never load it) ----
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi g_rccl;
static int rccl_load() {
    if (g_rccl.lib) return 0;
    // TBNN_RCCL_LIB: explicit collective library (tests run the N > 1 paths on a 1-GPU box against tests/stubccl).
    // Otherwise an RCCL the process has already loaded (torch ships its own copy) is re-used before a second copy
    // is brought in: two RCCL instances in one process would each run their own bootstrap / proxy threads.
    void* lib = nullptr;
    if (const char* ov = getenv("TBNN_RCCL_LIB")) {
        lib = dlopen(ov, RTLD_NOW | RTLD_GLOBAL);
        if (!lib) return fail(-5, std::string("TBNN_RCCL_LIB=") + ov + ": " + dlerror());
    }
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(-5, std::string("cannot load librccl.so: ") + dlerror());
    RcclApi a; a.lib = lib;
#define RSYM(field, name) do { *(void**)(&a.field) = dlsym(lib, name); if (!a.field) return fail(-5, std::string("librccl.so lacks ") + name); } while (0)
    RSYM(GetUniqueId, "ncclGetUniqueId"); RSYM(CommInitRank, "ncclCommInitRank"); RSYM(CommDestroy, "ncclCommDestroy");
    RSYM(CommCount, "ncclCommCount"); RSYM(AllReduce, "ncclAllReduce"); RSYM(AllGather, "ncclAllGather"); RSYM(GetErrorString, "ncclGetErrorString");
#undef RSYM
    g_rccl = a;
    return 0;
}
#define NCCLCHK(expr)                                                                          \
    do {                                                                                       \
        ncclResult_t r_ = (expr);                                                              \
        if (r_ != ncclSuccess) return fail(-5, std::string(#expr) + ": " + g_rccl.GetErrorString(r_)); \
    } while (0)

static_assert(sizeof(ncclUniqueId) == TBNN_COMM_ID_BYTES, "ncclUniqueId size");

extern "C" int tbnn_comm_unique_id(unsigned char id[TBNN_COMM_ID_BYTES]) {
    if (!id) return fail(-1, "null id");
    int rc = rccl_load(); if (rc) return rc;
    ncclUniqueId u;
    NCCLCHK(g_rccl.GetUniqueId(&u));
    memcpy(id, &u, TBNN_COMM_ID_BYTES);
    return 0;
}
extern "C" int tbnn_comm_create(tbnn_handle h, int world, int rank, const unsigned char id[TBNN_COMM_ID_BYTES],
                                tbnn_comm_handle* out) {
    NEED(h);
    if (!out || !id) return fail(-1, "null argument");
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world) return fail(-1, "bad world/rank");
    int rc = rccl_load(); if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    ncclUniqueId u; memcpy(&u, id, TBNN_COMM_ID_BYTES);
    tbnn_comm* c = new (std::nothrow) tbnn_comm();
    if (!c) return fail(-4, "out of host memory");
    c->world = world; c->rank = rank; c->device = h->device;
    ncclResult_t r = g_rccl.CommInitRank(&c->comm, world, u, rank);
    if (r != ncclSuccess) { delete c; return fail(-5, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r)); }
    *out = c;
    return 0;
}
// ranks in the communicator AS THE COLLECTIVE LIBRARY SEES IT (ncclCommCount): what bench.py reports per rank at N > 1
extern "C" int tbnn_comm_count(tbnn_comm_handle c) {
    if (!c) return fail(-1, "null communicator");
    int n = 0;
    NCCLCHK(g_rccl.CommCount(c->comm, &n));
    return n;
}
extern "C" int tbnn_comm_destroy(tbnn_comm_handle c) {
    if (!c) return 0;
    hipSetDevice(c->device);
    c->gbuf.reset();
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    delete c;
    return 0;
}
extern "C" int tbnn_gather_samples(tbnn_handle h, tbnn_comm_handle c, float* d_out, float* host_out) {
    NEED(h); if (!c) return fail(-1, "null communicator");
    ONE_CHAIN(h, "tbnn_gather_samples");
    HIPCHK(hipSetDevice(h->device));
    const size_t per = (size_t)h->nd.P + h->nd.H, tot = per * c->world;
    if (!d_out) {
        HIPCHK(c->gbuf.grow(tot, tot));
        d_out = c->gbuf;
    }
    // (theta, eta) staged contiguously in tmp (P+H floats)
    HIPCHK(hipMemcpyAsync(h->tmp, h->q_cur, (size_t)h->nd.P * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->tmp + h->nd.P, h->eta, (size_t)h->nd.H * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    NCCLCHK(g_rccl.AllGather(h->tmp, d_out, per, ncclFloat, c->comm, h->stream));
    if (host_out) HIPCHK(hipMemcpyAsync(host_out, d_out, tot * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
extern "C" int tbnn_set_row_shard(tbnn_handle h, tbnn_comm_handle c, int64_t n_total) {
    NEED(h);
    ONE_CHAIN(h, "tbnn_set_row_shard");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (c && n_total < 1) return fail(-1, "n_total must be >= 1");
    if (c && h->dYw) return fail(-1, "tbnn_set_row_shard: the handle has row weights (tbnn_set_row_weights): weighted row sharding needs the weight sum of all ranks");
    h->shard = c; h->n_total = c ? (long)n_total : 0;
    h->cur_valid = false;
    return 0;
}
// rows that normalise the likelihood (the sum of the row weights when they are set) / entries of the statistic buffer to sum
static inline double rows_total(const tbnn_ctx* h) { return h->dYw ? h->wsum : (double)(h->shard ? h->n_total : h->n); }
// Poisson's constant as data_logp takes it off the statistic; a row-sharded chain's statistic arrives without it: every rank took the C
// of its own rows off before the all-reduce (k_shard_pack), so all ranks hold the same full-data value and take the same decisions
static inline double lik_const(const tbnn_ctx* h) { return h->shard ? 0.0 : h->lik_c; }
// the targets the fused pass reads (with the row weights behind them when they are set) and the weights alone (null: none)
static inline const float* pass_Y(const tbnn_ctx* h) { return h->dYw ? h->dYw : h->dY; }
static inline const float* pass_w(const tbnn_ctx* h) { return h->dYw ? h->dYw + (size_t)h->n * h->nd.d_out : nullptr; }
static inline int stat_entries(const tbnn_ctx* h) { return h->shard ? 1 : h->grid; }      // sharded: pstat_red[0] is the all-reduced sum
// local statistic buffer: entries >= grid stay zero; the all-reduced copy is separate (ranks may have different grids)
static inline const double* stat_ptr(const tbnn_ctx* h) { return h->shard ? h->pstat_red : h->pstat; }
// the gradient slabs k_update reduces
static inline const float* grad_slabs(const tbnn_ctx* h) { return (h->shard && !h->be->slab_is_grad_row()) ? h->grow : h->slabs; }
static inline int grad_nslab(const tbnn_ctx* h) { return h->shard ? 1 : h->nslab; }

// ---- launch helpers (all on h->stream, no sync) ----
// an event pair from the pool around a launch, if this one is profiled (every h->profile-th): the opening event is recorded, the closing
// one returned for the caller to record behind the launch (null: not profiled).  steps: leapfrog steps the launch covers
static hipEvent_t profile_begin(tbnn_ctx* h, int steps) {
    if (!(h->profile > 0 && (h->launch_no++ % h->profile) == 0)) return nullptr;
    if (h->pev_used + 2 > h->pev.size()) {
        hipEvent_t a = nullptr, b = nullptr;
        hipEventCreate(&a); hipEventCreate(&b); h->pev.emplace_back(a); h->pev.emplace_back(b);
    }
    const hipEvent_t a = h->pev[h->pev_used], b = h->pev[h->pev_used + 1];
    h->pev_used += 2;
    h->pev_div.push_back(steps);
    hipEventRecord(a, h->stream);
    return b;
}
// q == h->q: the leapfrog position, whose padded image h->qimg is maintained by k_update;
// any other q gets its image built here (h->qimg_cur).
static int launch_fwd_bwd(tbnn_ctx* h, const float* q, const float* eta, const StepCtl* ctl = nullptr, int t = 0) {
    const float* img = nullptr;
    const int C = h->C;
    const long imgS = h->img_floats, slabS = (long)h->nslab * h->pitch;
    if (h->imgmap) {
        if (q == h->q && h->q_img_valid) img = h->qimg;
        else {
            hipLaunchKernelGGL(k_make_image, dim3((h->nd.P + 255) / 256, C), dim3(256), 0, h->stream, h->nd.P, q, h->imgmap, h->qimg_cur, (long)h->nd.P, imgS);
            img = h->qimg_cur;
        }
    }
    const hipEvent_t prof_end = profile_begin(h, 1);
    // one gradient for all chains of the handle: the one-kernel fused tables in ONE launch (gridDim.y = chain), the other backends
    // chain by chain through the same activation store (backend.hpp)
    const PassArgs pa = {img, imgS, q, eta, (long)h->nd.H, h->dX, pass_Y(h), pass_w(h), h->n, h->slabs, slabS, h->pitch, h->pstat, C, ctl, t, h->ctl_host};
    if (const int rc = h->be->fwd_bwd(h->stream, pa)) return rc;
    if (h->shard) {
        // ONE collective per fused pass: the dense data-term gradient row (P values; the wide path already has one) and the
        // statistic, summed to one value on the device, travel together as P + 1 doubles (the sum over the ranks is then
        // taken in double and rounded once; at configs[1]-class step times a second small all-reduce would cost as much as
        // the step), summed over the ranks in place, unpacked into the row k_update reads and pstat_red[0]
        const bool dense = h->be->slab_is_grad_row();
        float* row = dense ? h->slabs : h->grow;
        const int P = h->nd.P;
        if (!dense)
            hipLaunchKernelGGL(k_slab_reduce, dim3((P + 63) / 64), dim3(64, 4), 0, h->stream, (const float*)h->slabs, h->nslab,
                               h->pitch, P, (float*)nullptr, h->shard_buf);
        hipLaunchKernelGGL(k_shard_pack, dim3((P + 255) / 256), dim3(256), 0, h->stream, P, dense ? (const float*)row : (const float*)nullptr,
                           (const double*)h->pstat, h->grid, h->shard_buf,
                           h->nd.lik == TBNN_LIK_GAMMA ? -h->lik_c / (double)h->nd.lik_df :             // (Gamma: data_logp scales the statistic by -a)
                           h->nd.lik == TBNN_LIK_WEIBULL ? -h->lik_c : h->lik_c);                       // (Weibull: ... by -1)
        NCCLCHK(g_rccl.AllReduce(h->shard_buf, h->shard_buf, (size_t)P + 1, ncclDouble, ncclSum, h->shard->comm, h->stream));
        hipLaunchKernelGGL(k_shard_unpack, dim3((P + 255) / 256), dim3(256), 0, h->stream, P, (const double*)h->shard_buf, row, h->pstat_red);
    }
    if (prof_end) hipEventRecord(prof_end, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}
static void launch_update(tbnn_ctx* h, int mode, float eps, const float* eta, float* q, float* g, const StepCtl* ctl = nullptr, int t = 0) {
    const bool big = h->nd.P >= UPD_BIG_P;             // block geometry by parameter count (update_ops.hpp)
    const int ucols = big ? UPD_COLS_BIG : UPD_COLS;
    const int gx = (h->pitch / 4 + ucols - 1) / ucols;
    const bool img = h->imgmap && q == h->q;
    // the data-term gradient goes with its state: the proposal's (h->gd) or, for the bootstrap evaluation, the current one's
    float* gd = g == h->g_cur ? h->gd_cur : (g == h->g ? h->gd : nullptr);
    if (big)
        hipLaunchKernelGGL((k_update<UPD_COLS_BIG, UPD_GROUPS_BIG>), dim3(gx, h->C), dim3(UPD_COLS_BIG, UPD_GROUPS_BIG), 0, h->stream, h->nd, mode, eps, eta,
                           grad_slabs(h), grad_nslab(h), h->pitch, h->q_cur, h->g_cur, q, h->p, g, img ? h->imgmap : nullptr, h->qimg, gd, h->img_floats, ctl, t);
    else
        hipLaunchKernelGGL((k_update<UPD_COLS, UPD_GROUPS>), dim3(gx, h->C), dim3(UPD_COLS, UPD_GROUPS), 0, h->stream, h->nd, mode, eps, eta, grad_slabs(h),
                           grad_nslab(h), h->pitch, h->q_cur, h->g_cur, q, h->p, g, img ? h->imgmap : nullptr, h->qimg, gd, h->img_floats, ctl, t);
    if (img && (mode == UPD_FIRST || mode == UPD_MID)) h->q_img_valid = true;
}
static void launch_energy(tbnn_ctx* h, int which, const float* eta, const float* q, double* slot) {
    hipLaunchKernelGGL(k_energy, dim3(1, h->C), dim3(1024), 0, h->stream, h->nd, which, eta, q, h->p, h->q_cur, stat_ptr(h),
                       stat_entries(h), rows_total(h), lik_const(h), h->sc, slot);
}

// make (logp, grad, stat) at q_cur valid
static int ensure_current(tbnn_ctx* h, double* slot) {
    if (h->cur_valid) return 0;
    int rc = launch_fwd_bwd(h, h->q_cur, h->eta);
    if (rc) return rc;
    launch_update(h, UPD_GRAD_ONLY, 0.f, h->eta, h->q_cur, h->g_cur);
    launch_energy(h, EN_CUR, h->eta, h->q_cur, slot);
    h->cur_valid = true;
    return 0;
}
// mean duration (us) of the profiled fwd+bwd launches since the last drain
static float drain_profile(tbnn_ctx* h) {
    double tot = 0.0; int cnt = 0;
    for (size_t i = 0; i + 1 < h->pev_used; i += 2) {
        float ms = 0.f;
        const int div = i / 2 < h->pev_div.size() ? h->pev_div[i / 2] : 1;
        if (hipEventElapsedTime(&ms, h->pev[i], h->pev[i + 1]) == hipSuccess) { tot += ms * 1000.0 / (div > 0 ? div : 1); ++cnt; }
    }
    h->pev_used = 0;                      // the events stay in the pool
    h->pev_div.clear();
    return cnt ? (float)(tot / cnt) : 0.f;
}

// the weights a call evaluates at: the chain's own (theta == null), else theta copied into the proposal buffer h->q, whose image goes stale
static int stage_theta(tbnn_ctx* h, const float* theta, const float** dq) {
    *dq = h->q_cur;
    if (!theta) return 0;
    HIPCHK(hipMemcpyAsync(h->q, theta, (size_t)h->nd.P * sizeof(float), hipMemcpyHostToDevice, h->stream));
    *dq = h->q; h->q_img_valid = false;
    return 0;
}

extern "C" int tbnn_logp_grad(tbnn_handle h, const float* theta, const float* eta, double* logp, float* grad,
                              double* stat) {
    NEED(h);
    ONE_CHAIN(h, "tbnn_logp_grad");
    if (!h->dX) return fail(-1, "tbnn_set_data has not been called");
    HIPCHK(hipSetDevice(h->device));
    const NetDev& nd = h->nd;
    // evaluation happens on scratch copies (q, tmp-eta): the chain state is untouched
    const float* dq = nullptr;
    const float* de = h->eta;
    if (const int rc = stage_theta(h, theta, &dq)) return rc;
    if (eta) { HIPCHK(hipMemcpyAsync(h->tmp + nd.P, eta, (size_t)nd.H * sizeof(float), hipMemcpyHostToDevice, h->stream)); de = h->tmp + nd.P; }
    int rc = launch_fwd_bwd(h, dq, de);
    if (rc) return rc;
    const int gx = (h->pitch / 4 + UPD_COLS - 1) / UPD_COLS;
    hipLaunchKernelGGL((k_update<UPD_COLS, UPD_GROUPS>), dim3(gx), dim3(UPD_COLS, UPD_GROUPS), 0, h->stream, nd, (int)UPD_GRAD_ONLY, 0.f, de, grad_slabs(h), grad_nslab(h),
                       h->pitch, h->q_cur, h->g_cur, const_cast<float*>(dq), h->p, h->tmp, (const int*)nullptr, (float*)nullptr, (float*)nullptr);
    // EN_TRACE leaves the chain's scalar record alone; stat comes from the slabs
    HIPCHK(h->trace.grow(2, 4096));
    hipLaunchKernelGGL(k_energy, dim3(1), dim3(1024), 0, h->stream, nd, (int)EN_TRACE, de, dq, h->p, h->q_cur, stat_ptr(h),
                       stat_entries(h), rows_total(h), lik_const(h), h->sc, h->trace);
    HIPCHK(hipGetLastError());
    double lp = 0.0;
    HIPCHK(hipMemcpyAsync(&lp, h->trace, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad) HIPCHK(hipMemcpyAsync(grad, h->tmp, (size_t)nd.P * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    std::vector<double> ps;
    if (stat) { ps.resize(stat_entries(h)); HIPCHK(hipMemcpyAsync(ps.data(), stat_ptr(h), ps.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream)); }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->profile) drain_profile(h);
    if (logp) *logp = lp;
    if (stat) {
        double s = 0; for (double v : ps) s += v;
        *stat = s - lik_const(h);                                                          // (Poisson: the log-likelihood with its constant)
        if (nd.lik == TBNN_LIK_GAMMA) *stat = -(double)nd.lik_df * s - lik_const(h);       // (... as data_logp forms it from sum w (f + y e^-f))
        if (nd.lik == TBNN_LIK_WEIBULL) *stat = -s - lik_const(h);                         // (... from sum w (k d f + u))
        if (nd.lik == TBNN_LIK_HETERO_GAUSSIAN) *stat -= 0.5 * 1.8378770664093453 /* log 2pi */ * rows_total(h);      // (... as data_logp adds it)
    }
    return 0;
}

extern "C" int tbnn_forward(tbnn_handle h, const float* theta, const float* X, int64_t n, float* out) {
    NEED(h);
    if (!theta) ONE_CHAIN(h, "tbnn_forward at the chain's own state");
    if (!X || !out || n < 1) return fail(-1, "forward: null pointer or n < 1");
    HIPCHK(hipSetDevice(h->device));
    const NetDev& nd = h->nd;
    const float* dq = nullptr;
    if (const int rc = stage_theta(h, theta, &dq)) return rc;
    Buf<float> dXf, dOut;
    HIPCHK(dXf.alloc((size_t)n * nd.d_in));
    HIPCHK(dOut.alloc((size_t)n * nd.d_out));
    HIPCHK(hipMemcpyAsync(dXf, X, (size_t)n * nd.d_in * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (const int rc = h->be->forward(h->stream, 1, dq, dXf, (long)n, dOut, h->imgmap, h->qimg_cur)) return rc;
    HIPCHK(hipMemcpyAsync(out, dOut, (size_t)n * nd.d_out * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int tbnn_set_validation(tbnn_handle h, const float* X, const float* Y, int64_t n) {
    NEED(h);
    if (!X || !Y || n < 1) return fail(-1, "set_validation: null pointer or n < 1");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->dXv.reset(); h->dYv.reset();
    HIPCHK(h->dXv.alloc((size_t)n * h->nd.d_in));
    HIPCHK(h->dYv.alloc((size_t)n * h->nd.d_out));
    HIPCHK(hipMemcpy(h->dXv, X, (size_t)n * h->nd.d_in * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->dYv, Y, (size_t)n * h->nd.d_out * sizeof(float), hipMemcpyHostToDevice));
    h->nv = (long)n;
    return 0;
}

// predictions over the staged training (which = 0) or validation (1) rows into h->fbuf[d_out][n]
static int predict_resident(tbnn_ctx* h, int which, const float* theta, long* n_out) {
    const NetDev& nd = h->nd;
    if (!theta) ONE_CHAIN(h, "tbnn_predict / tbnn_metrics at the chain's own state");
    const float* dX = which ? h->dXv : h->dX;
    const long n = which ? h->nv : h->n;
    if (!dX || n < 1) return fail(-1, which ? "tbnn_set_validation has not been called" : "tbnn_set_data has not been called");
    const float* dq = nullptr;
    if (const int rc = stage_theta(h, theta, &dq)) return rc;
    const size_t need = (size_t)n * nd.d_out;
    HIPCHK(h->fbuf.grow(need, need));
    *n_out = n;
    return h->be->forward(h->stream, 1, dq, dX, n, h->fbuf, h->imgmap, h->qimg_cur);
}

extern "C" int tbnn_predict(tbnn_handle h, int which, const float* theta, float* out) {
    NEED(h);
    if (which != 0 && which != 1) return fail(-1, "which must be 0 (training rows) or 1 (validation rows)");
    HIPCHK(hipSetDevice(h->device));
    long n = 0;
    int rc = predict_resident(h, which, theta, &n);
    if (rc) return rc;
    if (out) HIPCHK(hipMemcpyAsync(out, h->fbuf, (size_t)n * h->nd.d_out * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

#include "ensemble_api.hpp"               // tbnn_forward_many and the ensemble reductions (it uses tbnn_ctx, lik_known, Buf, fail, HIPCHK and NEED above)

extern "C" int tbnn_metrics(tbnn_handle h, int which, const float* theta, float mean, float sd, int exp_pred, int exp_real,
                            double out3[3]) {
    NEED(h);
    if (!out3) return fail(-1, "null out3");
    if (which != 0 && which != 1) return fail(-1, "which must be 0 (training rows) or 1 (validation rows)");
    HIPCHK(hipSetDevice(h->device));
    long n = 0;
    int rc = predict_resident(h, which, theta, &n);
    if (rc) return rc;
    const int MB = 256;
    HIPCHK(h->mpart.grow(3 * MB, 3 * MB));
    // (heteroscedastic Gaussian: output 1 is the log-sd and target column 1 is not read -- the mean against column 0 alone)
    const int d_cmp = h->nd.lik == TBNN_LIK_HETERO_GAUSSIAN ? 1 : h->nd.d_out;
    const long tot = n * d_cmp;
    const int grid = (int)std::min<long>(MB, (tot + 255) / 256);
    hipLaunchKernelGGL(k_metrics, dim3(grid), dim3(256), 0, h->stream, (const float*)h->fbuf, (const float*)(which ? h->dYv : h->dY), n,
                       d_cmp, h->nd.d_out, mean, sd, exp_pred, exp_real, h->mpart);
    HIPCHK(hipGetLastError());
    std::vector<double> part(3 * (size_t)grid);
    HIPCHK(hipMemcpyAsync(part.data(), h->mpart, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    double a[3] = {0, 0, 0};
    for (int b = 0; b < grid; ++b) for (int k = 0; k < 3; ++k) a[k] += part[3 * b + k];
    for (int k = 0; k < 3; ++k) out3[k] = a[k] / (double)tot;
    return 0;
}

// enqueue one transition (no sync).  trace: device array of L+1 doubles or null.
// ctl (device, mirrored in h->ctl_host) != null: every chain at its own (eps, L) -- L is then max_c L_c and eps unused
static int enqueue_transition(tbnn_ctx* h, float eps, int L, const float* d_p0, const float* d_logu, double* d_trace,
                              Scal* d_out, const StepCtl* ctl = nullptr) {
    const NetDev& nd = h->nd;
    // logp0 of the trace: a fresh bootstrap evaluation writes it; a cached one (cur_valid) is copied from the chain's
    // scalar record -- h->pstat then holds the statistic of the LAST fused launch (a rejected proposal, a
    // tbnn_logp_grad probe), not of q_cur, so EN_CUR must not be re-derived from it
    const bool cached = h->cur_valid;
    int rc = ensure_current(h, d_trace);
    if (rc) return rc;
    if (d_trace && cached) hipLaunchKernelGGL(k_trace_logp_cur, dim3(1), dim3(64), 0, h->stream, (const Scal*)h->sc, d_trace);
    hipLaunchKernelGGL(k_begin, dim3(1, h->C), dim3(1024), 0, h->stream, nd, d_p0, d_logu, h->epoch, h->key0, h->key1, h->p, h->sc, h->seed_hi);
    launch_update(h, UPD_FIRST, eps, h->eta, h->q, h->g, ctl, 0);
    // a small problem on an ahead-of-time narrow kernel: the L leapfrog steps in ONE launch, one workgroup per chain (kernels_traj.hpp).
    // Not for a traced transition (per-step energies) or a sharded gradient.  Profiling (tbnn_set_profiling) does NOT change the path (round 6;
    // ADVICE round 5): a profiled trajectory launch is bracketed by one event pair and reported per leapfrog step (its time / L).
    const bool traj = h->traj && !d_trace && L >= 1 && h->n <= h->be->traj_max_rows() && !h->shard;
    h->last_path = traj ? "trajectory" : "per-step";
    if (traj) {
        const hipEvent_t prof_end = profile_begin(h, L);
        const int trc = h->be->trajectory(h->stream, h->C, h->qimg, (long)h->img_floats, h->eta, h->dX, h->dY, h->n, h->q, h->p, h->g, h->gd, h->imgmap, h->pstat,
                                          stat_entries(h), eps, L, ctl);
        if (prof_end) hipEventRecord(prof_end, h->stream);
        if (trc)
            return fail(-2, "trajectory kernel launch failed");
        h->q_img_valid = false;            // the images the kernel advanced lived in LDS
    }
    for (int t = 1; t <= L && !traj; ++t) {
        rc = launch_fwd_bwd(h, h->q, h->eta, ctl, t);
        if (rc) return rc;
        if (d_trace && t < L) {
            // logp at q_t needs the prior at q_t: evaluate before the drift
            launch_update(h, UPD_GRAD_ONLY, 0.f, h->eta, h->q, h->g);
            launch_energy(h, EN_TRACE, h->eta, h->q, d_trace + t);
        }
        launch_update(h, t < L ? UPD_MID : UPD_LAST, eps, h->eta, h->q, h->g, ctl, t);
    }
    // the Metropolis decision, the host record and the commit in ONE single-workgroup launch for networks whose state that
    // workgroup copies in a few trips (TBNN_MERGE_ENDS=0: three launches, as before round 3)
    if (h->merge_ends && nd.P <= 32768) {
        hipLaunchKernelGGL(k_energy, dim3(1, h->C), dim3(1024), 0, h->stream, h->nd, (int)EN_NEW, (const float*)h->eta, (const float*)h->q, (const float*)h->p,
                           (const float*)h->q_cur, stat_ptr(h), stat_entries(h), rows_total(h), lik_const(h), h->sc, d_trace ? d_trace + L : (double*)nullptr,
                           d_out, (const float*)h->g, h->q_cur, h->g_cur, (const float*)h->gd, h->gd_cur);
    } else {
        launch_energy(h, EN_NEW, h->eta, h->q, d_trace ? d_trace + L : nullptr);
        hipLaunchKernelGGL(k_commit, dim3((nd.P + 255) / 256, h->C), dim3(256), 0, h->stream, nd.P, (const Scal*)h->sc, (const float*)h->q, (const float*)h->g,
                           h->q_cur, h->g_cur, (const float*)h->gd, h->gd_cur);
        hipLaunchKernelGGL(k_commit_scal, dim3(h->C), dim3(64), 0, h->stream, h->sc, d_out);
    }
    HIPCHK(hipGetLastError());
    h->epoch += 1;
    return 0;
}

static void fill_out(const Scal& s, int L, float dev_us, float fb_us, tbnn_step_out* o) {
    o->accepted = s.accepted; o->n_leapfrog = L;
    o->log_accept_ratio = (float)s.lar;
    o->accept_prob = s.lar < 0 ? (float)exp(s.lar) : 1.f;      // network.py:410-411
    o->logp_old = s.logp_cur; o->logp_new = s.logp_new;
    o->kinetic_old = s.k0; o->kinetic_new = s.k1;
    o->sjd = s.sjd; o->device_us = dev_us; o->fwdbwd_us = fb_us;
}

extern "C" int tbnn_hmc_step(tbnn_handle h, float eps, int32_t L, const float* p0, const float* log_u,
                             tbnn_step_out* out, double* trace_logp) {
    NEED(h);
    if (!h->dX) return fail(-1, "tbnn_set_data has not been called");
    if (L < 1) return fail(-1, "L must be >= 1");
    if (h->C > 1 && (p0 || log_u || trace_logp)) return fail(-1, "hmc_step on a multi-chain handle: no injected draws, no trace (out: one record per chain)");
    HIPCHK(hipSetDevice(h->device));
    const NetDev& nd = h->nd;
    const float* d_p0 = nullptr; const float* d_lu = nullptr;
    if (p0) { HIPCHK(hipMemcpyAsync(h->p0_inj, p0, (size_t)nd.P * sizeof(float), hipMemcpyHostToDevice, h->stream)); d_p0 = h->p0_inj; }
    if (log_u) { HIPCHK(hipMemcpyAsync(h->logu_inj, log_u, sizeof(float), hipMemcpyHostToDevice, h->stream)); d_lu = h->logu_inj; }
    double* d_trace = nullptr;
    if (trace_logp) {
        HIPCHK(h->trace.grow((size_t)L + 1, (size_t)L + 1 + 4096));
        d_trace = h->trace;
    }
    // the bootstrap evaluation (Q10: the reference pays it every epoch) is outside the timed events only
    // when it is cached; ensure_current is part of enqueue_transition.
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    int rc = enqueue_transition(h, eps, L, d_p0, d_lu, d_trace, h->sc_out);
    if (rc) return rc;
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipMemcpyAsync(h->sc_host, h->sc_out, (size_t)h->C * sizeof(Scal), hipMemcpyDeviceToHost, h->stream));
    if (trace_logp) HIPCHK(hipMemcpyAsync(trace_logp, h->trace, (size_t)(L + 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0.f; hipEventElapsedTime(&ms, h->ev0, h->ev1);
    const float fb = h->profile ? drain_profile(h) : 0.f;
    if (out)
        for (int c = 0; c < h->C; ++c) fill_out(h->sc_host[c], L, ms * 1000.f, fb, out + c);
    return 0;
}

// per-epoch records: a pooled device buffer and a pooled pinned host mirror (no allocator call -- hipFree synchronises
// the device -- inside a caller's timed loop once the pool has grown to the largest n_epochs seen)
static int grow_records(tbnn_ctx* h, int n_epochs) {
    const size_t need = (size_t)n_epochs * h->C;
    HIPCHK(h->d_recs.grow(need, std::max<size_t>(need, 64)));
    HIPCHK(h->h_recs.grow(need, std::max<size_t>(need, 64)));
    return 0;
}
extern "C" int tbnn_hmc_run(tbnn_handle h, float eps, int32_t L, int32_t n_epochs, tbnn_step_out* outs) {
    NEED(h);
    if (!h->dX) return fail(-1, "tbnn_set_data has not been called");
    if (L < 1 || n_epochs < 1) return fail(-1, "L and n_epochs must be >= 1");
    if ((long long)n_epochs * (long long)h->C > (1LL << 24)) return fail(-1, "n_epochs x chains exceeds 2^24 records per call: split the run");
    HIPCHK(hipSetDevice(h->device));
    const int C = h->C;                                  // records: [epoch][chain] on the device, outs[chain][epoch] for the caller
    if (const int rc = grow_records(h, n_epochs)) return rc;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int e = 0; e < n_epochs; ++e) {
        int rc = enqueue_transition(h, eps, L, nullptr, nullptr, nullptr, h->d_recs + (size_t)e * C);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipMemcpyAsync(h->h_recs, h->d_recs, (size_t)n_epochs * C * sizeof(Scal), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0.f; hipEventElapsedTime(&ms, h->ev0, h->ev1);
    const float fb = h->profile ? drain_profile(h) : 0.f;
    if (outs)
        for (int c = 0; c < C; ++c)
            for (int e = 0; e < n_epochs; ++e) fill_out(h->h_recs[(size_t)e * C + c], L, ms * 1000.f / n_epochs, fb, outs + (size_t)c * n_epochs + e);
    return 0;
}

// every chain of the handle at its own (eps, L): stage the control block, run max L lockstep steps (enqueue_transition)
static int stage_ctl(tbnn_ctx* h, const float* eps, const int32_t* L, int* Lmax) {
    if (!eps || !L) return fail(-1, "null eps / L array");
    int m = 0;
    for (int c = 0; c < h->C; ++c) {
        if (L[c] < 1) return fail(-1, "every L[c] must be >= 1");
        h->ctl_host[c].eps = eps[c]; h->ctl_host[c].L = L[c];
        m = std::max(m, (int)L[c]);
    }
    HIPCHK(hipMemcpyAsync(h->ctl, h->ctl_host, (size_t)h->C * sizeof(StepCtl), hipMemcpyHostToDevice, h->stream));
    *Lmax = m;
    return 0;
}
extern "C" int tbnn_hmc_run_each(tbnn_handle h, const float* eps, const int32_t* L, int32_t n_epochs, tbnn_step_out* outs) {
    NEED(h);
    if (!h->dX) return fail(-1, "tbnn_set_data has not been called");
    if (n_epochs < 1) return fail(-1, "n_epochs must be >= 1");
    if ((long long)n_epochs * (long long)h->C > (1LL << 24)) return fail(-1, "n_epochs x chains exceeds 2^24 records per call: split the run");
    HIPCHK(hipSetDevice(h->device));
    const int C = h->C;
    // (the stream is idle here -- every entry point returns after its work has completed -- so re-staging ctl_host is safe)
    int Lmax = 0;
    int rc = stage_ctl(h, eps, L, &Lmax);
    if (rc) return rc;
    if ((rc = grow_records(h, n_epochs))) return rc;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int e = 0; e < n_epochs; ++e) {
        rc = enqueue_transition(h, 0.f, Lmax, nullptr, nullptr, nullptr, h->d_recs + (size_t)e * C, h->ctl);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipMemcpyAsync(h->h_recs, h->d_recs, (size_t)n_epochs * C * sizeof(Scal), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0.f; hipEventElapsedTime(&ms, h->ev0, h->ev1);
    const float fb = h->profile ? drain_profile(h) : 0.f;
    if (outs)
        for (int c = 0; c < C; ++c)
            for (int e = 0; e < n_epochs; ++e) fill_out(h->h_recs[(size_t)e * C + c], L[c], ms * 1000.f / n_epochs, fb, outs + (size_t)c * n_epochs + e);
    return 0;
}
extern "C" int tbnn_hmc_step_each(tbnn_handle h, const float* eps, const int32_t* L, tbnn_step_out* out) {
    return tbnn_hmc_run_each(h, eps, L, 1, out);
}

extern "C" int tbnn_set_lik_df(tbnn_handle h, float df) {
    NEED(h);
    if (h->nd.lik == TBNN_LIK_STUDENT_T) return fail(-1, "set_lik_df: a Student-t handle takes its degrees of freedom from the descriptor's lik_df");
    if (h->nd.lik == TBNN_LIK_NEG_BINOMIAL) return fail(-1, "set_lik_df: a negative-binomial handle takes its dispersion from the descriptor's lik_df");
    if (h->nd.lik == TBNN_LIK_GAMMA) return fail(-1, "set_lik_df: a Gamma handle takes its shape from the descriptor's lik_df");
    if (h->nd.lik == TBNN_LIK_WEIBULL) return fail(-1, "set_lik_df: a Weibull handle takes its shape from the descriptor's lik_df");
    if (!df_ok(df)) return fail(-1, "set_lik_df: df must be finite and > 0");
    h->ens_df = df;
    return 0;
}

// ---- pre-training (include/tbnn.h: tbnn_optimize): Adam / AMSGrad ascent of the target log-probability, the whole run queued on the
// chain's stream.  Replaces BNN_functions.trainBasicRegression / trainBasicClassification's Keras loop (BNN_functions.py:136-161, :255-279).
static void launch_optim_logp(tbnn_ctx* h, int lik_only, int step, int n_checks, int k) {
    hipLaunchKernelGGL(k_optim_logp, dim3(1, h->C), dim3(1024), 0, h->stream, h->nd, lik_only, (const float*)h->eta, (const float*)h->q, stat_ptr(h),
                       stat_entries(h), rows_total(h), lik_const(h), (OptChain*)h->opt_oc, step, (double*)h->opt_trace, n_checks, k);
}
static void launch_optim(tbnn_ctx* h, int lik_only, const OptStep& s, int checked) {
    const bool big = h->nd.P >= UPD_BIG_P;             // k_update's choice of block geometry (update_ops.hpp)
    const int ucols = big ? UPD_COLS_BIG : UPD_COLS;
    const int gx = (h->pitch / 4 + ucols - 1) / ucols;
    const int* map = h->imgmap;
    if (big)
        hipLaunchKernelGGL((k_optim<UPD_COLS_BIG, UPD_GROUPS_BIG>), dim3(gx, h->C), dim3(UPD_COLS_BIG, UPD_GROUPS_BIG), 0, h->stream, h->nd, lik_only, s, checked,
                           (const float*)h->eta, grad_slabs(h), grad_nslab(h), h->pitch, (float*)h->q, (float*)h->opt_g, (float*)h->opt_m, (float*)h->opt_v,
                           (float*)h->opt_vhat, (float*)h->opt_qbest, (const OptChain*)h->opt_oc, map, (float*)h->qimg, h->img_floats);
    else
        hipLaunchKernelGGL((k_optim<UPD_COLS, UPD_GROUPS>), dim3(gx, h->C), dim3(UPD_COLS, UPD_GROUPS), 0, h->stream, h->nd, lik_only, s, checked,
                           (const float*)h->eta, grad_slabs(h), grad_nslab(h), h->pitch, (float*)h->q, (float*)h->opt_g, (float*)h->opt_m, (float*)h->opt_v,
                           (float*)h->opt_vhat, (float*)h->opt_qbest, (const OptChain*)h->opt_oc, map, (float*)h->qimg, h->img_floats);
}
extern "C" int tbnn_optimize(tbnn_handle h, const tbnn_optim_cfg* cfg, int32_t n_steps, int32_t reset, tbnn_optim_out* out, double* trace) {
    NEED(h);
    // every refusal comes before the handle is touched
    if (!cfg || !out) return fail(-1, "tbnn_optimize: null cfg or out");
    if (!h->dX) return fail(-1, "tbnn_optimize: tbnn_set_data has not been called");
    if (h->shard) return fail(-1, "tbnn_optimize: not on a row-sharded handle (tbnn_set_row_shard): the optimiser runs on unsharded handles only");
    if (n_steps < 0) return fail(-1, "tbnn_optimize: n_steps must be >= 0");
    if (cfg->check_every < 1) return fail(-1, "tbnn_optimize: check_every must be >= 1");
    if (!std::isfinite(cfg->lr) || !(cfg->lr > 0.f)) return fail(-1, "tbnn_optimize: lr must be finite and > 0");
    if (!std::isfinite(cfg->epsilon) || !(cfg->epsilon > 0.f)) return fail(-1, "tbnn_optimize: epsilon must be finite and > 0");
    if (!(cfg->beta1 >= 0.f && cfg->beta1 < 1.f) || !(cfg->beta2 >= 0.f && cfg->beta2 < 1.f)) return fail(-1, "tbnn_optimize: beta1 and beta2 must be in [0, 1)");
    if (cfg->objective != TBNN_OPT_POSTERIOR && cfg->objective != TBNN_OPT_LIKELIHOOD) return fail(-1, "tbnn_optimize: unknown objective");
    HIPCHK(hipSetDevice(h->device));
    const NetDev& nd = h->nd;
    const int C = h->C, T = n_steps, every = cfg->check_every;
    const int n_checks = (T + every - 1) / every + 1;            // t in {0, k, 2k, .. < T}, and T
    const size_t PN = (size_t)C * nd.P;
    const dim3 pgrid((nd.P + 255) / 256, C);
    if (!h->opt_live) {
        HIPCHK(h->opt_m.alloc(PN)); HIPCHK(h->opt_v.alloc(PN)); HIPCHK(h->opt_vhat.alloc(PN)); HIPCHK(h->opt_g.alloc(PN)); HIPCHK(h->opt_qbest.alloc(PN));
        HIPCHK(h->opt_oc.alloc((size_t)C)); HIPCHK(h->opt_oc_host.alloc((size_t)C));
    }
    HIPCHK(h->opt_trace.grow((size_t)C * n_checks, (size_t)C * n_checks + 1024));
    if (reset || !h->opt_live) {
        hipLaunchKernelGGL(k_optim_reset, pgrid, dim3(256), 0, h->stream, nd.P, C, (const float*)h->q_cur, (float*)h->opt_m, (float*)h->opt_v, (float*)h->opt_vhat,
                           (float*)h->opt_g, (float*)h->opt_qbest, (OptChain*)h->opt_oc);
        h->opt_t = 0; h->opt_live = true;
    }
    const int lik_only = cfg->objective == TBNN_OPT_LIKELIHOOD;
    // theta_0 = the chain's state, in the proposal buffer with its padded image: k_optim keeps both current from here on
    HIPCHK(hipMemcpyAsync(h->q, h->q_cur, PN * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    h->q_img_valid = false; h->cur_valid = false;
    if (h->imgmap) {
        hipLaunchKernelGGL(k_make_image, pgrid, dim3(256), 0, h->stream, nd.P, (const float*)h->q, h->imgmap, h->qimg, (long)nd.P, (long)h->img_floats);
        h->q_img_valid = true;
    }
    struct ImageStale {                                        // on EVERY exit: the proposal buffer no longer mirrors a leapfrog position
        tbnn_ctx* h;
        ~ImageStale() { h->q_img_valid = false; h->cur_valid = false; }
    } guard{h};
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    const double b1 = (double)cfg->beta1, b2 = (double)cfg->beta2;
    OptStep s;
    s.b1 = cfg->beta1; s.b2 = cfg->beta2; s.omb1 = (float)(1.0 - b1); s.omb2 = (float)(1.0 - b2); s.epsilon = cfg->epsilon; s.amsgrad = cfg->amsgrad != 0;
    int k = 0;
    for (int i = 0; i < T; ++i) {
        if (const int rc = launch_fwd_bwd(h, h->q, h->eta)) return rc;
        const int checked = i % every == 0;
        if (checked) launch_optim_logp(h, lik_only, (int)(h->opt_t + i), n_checks, k++);
        const double t = (double)(h->opt_t + i + 1);
        s.a_t = (float)((double)cfg->lr / (1.0 - std::pow(b1, t)));
        s.r_t = (float)(1.0 / std::sqrt(1.0 - std::pow(b2, t)));
        launch_optim(h, lik_only, s, checked);
    }
    if (const int rc = launch_fwd_bwd(h, h->q, h->eta)) return rc;
    launch_optim_logp(h, lik_only, (int)(h->opt_t + T), n_checks, k++);
    hipLaunchKernelGGL(k_optim_finish, pgrid, dim3(256), 0, h->stream, nd.P, cfg->keep_best != 0, (const OptChain*)h->opt_oc, (const float*)h->q,
                       (float*)h->opt_qbest, (float*)h->q_cur);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    h->opt_t += T;
    std::vector<double> tr((size_t)C * n_checks);
    HIPCHK(hipMemcpyAsync(tr.data(), h->opt_trace, tr.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->opt_oc_host, h->opt_oc, (size_t)C * sizeof(OptChain), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0.f; hipEventElapsedTime(&ms, h->ev0, h->ev1);
    if (h->profile) drain_profile(h);
    for (int c = 0; c < C; ++c) {
        const OptChain& oc = h->opt_oc_host[c];
        const double* tc = tr.data() + (size_t)c * n_checks;
        tbnn_optim_out& o = out[c];
        o.steps_done = T; o.diverged = oc.frozen; o.best_step = oc.best_step; o.n_checks = n_checks;
        if (oc.frozen)                                        // the step whose check froze the chain (0: it was frozen when the call began)
            for (int j = 0; j < n_checks; ++j)
                if (!std::isfinite(tc[j])) { o.steps_done = std::min(T, j * every); break; }
        o.obj_first = tc[0]; o.obj_last = tc[n_checks - 1]; o.obj_best = oc.best; o.device_us = ms * 1000.f;
    }
    if (trace) memcpy(trace, tr.data(), tr.size() * sizeof(double));
    return 0;
}
extern "C" int tbnn_optim_state(tbnn_handle h, float* m, float* v, float* vhat, float* g, int32_t* t) {
    NEED(h);
    if (!h->opt_live) return fail(-1, "tbnn_optim_state: tbnn_optimize has not been called on this handle");
    HIPCHK(hipSetDevice(h->device));
    const size_t B = (size_t)h->C * h->nd.P * sizeof(float);
    if (m) HIPCHK(hipMemcpyAsync(m, h->opt_m, B, hipMemcpyDeviceToHost, h->stream));
    if (v) HIPCHK(hipMemcpyAsync(v, h->opt_v, B, hipMemcpyDeviceToHost, h->stream));
    if (vhat) HIPCHK(hipMemcpyAsync(vhat, h->opt_vhat, B, hipMemcpyDeviceToHost, h->stream));
    if (g) HIPCHK(hipMemcpyAsync(g, h->opt_g, B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (t) *t = (int32_t)h->opt_t;
    return 0;
}

extern "C" int tbnn_hyper_logp_grad(tbnn_handle h, const float* eta, double* logp, float* grad) {
    NEED(h);
    ONE_CHAIN(h, "tbnn_hyper_logp_grad");
    if (!h->dX) return fail(-1, "tbnn_set_data has not been called");
    HIPCHK(hipSetDevice(h->device));
    const NetDev& nd = h->nd;
    int rc = ensure_current(h, nullptr);   // stat_cur = sum (y-f)^2 at q_cur (closed-form data term)
    if (rc) return rc;
    float* de = h->eta;
    if (eta) { HIPCHK(hipMemcpyAsync(h->tmp + nd.P, eta, (size_t)nd.H * sizeof(float), hipMemcpyHostToDevice, h->stream)); de = h->tmp + nd.P; }
    hipLaunchKernelGGL(k_hyper, dim3(1), dim3(HYP_THREADS), 0, h->stream, nd, (int)HYP_EVAL, 0.f, 0, de, h->q_cur, rows_total(h),
                       (const float*)nullptr, (const float*)nullptr, 0u, h->key0, h->key1, h->sc, h->hyp_ws, h->sc_out);
    HIPCHK(hipGetLastError());
    std::vector<float> ws(hyper_ws_bytes(nd) / sizeof(float));
    HIPCHK(hipMemcpyAsync(ws.data(), h->hyp_ws, hyper_ws_bytes(nd), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->sc_host, h->sc_out, sizeof(Scal), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (logp) *logp = h->sc_host[0].logp_new;
    if (grad) memcpy(grad, ws.data() + HYP_WS_GRAD * nd.H, (size_t)nd.H * sizeof(float));
    return 0;
}

static int hyper_step_impl(tbnn_handle h, float eps_h, const float* eps_each, int32_t L_h, const float* p0, const float* log_u, tbnn_step_out* out);
extern "C" int tbnn_hyper_step(tbnn_handle h, float eps_h, int32_t L_h, const float* p0, const float* log_u,
                               tbnn_step_out* out) {
    return hyper_step_impl(h, eps_h, nullptr, L_h, p0, log_u, out);
}
extern "C" int tbnn_hyper_step_each(tbnn_handle h, const float* eps_h, int32_t L_h, tbnn_step_out* out) {
    NEED(h);
    if (!eps_h) return fail(-1, "null eps_h array");
    return hyper_step_impl(h, 0.f, eps_h, L_h, nullptr, nullptr, out);
}
// eps_each (host, [chains]) != null: chain c's hyper transition at eps_each[c]
static int hyper_step_impl(tbnn_handle h, float eps_h, const float* eps_each, int32_t L_h, const float* p0, const float* log_u, tbnn_step_out* out) {
    NEED(h);
    if (!h->dX) return fail(-1, "tbnn_set_data has not been called");
    if (L_h < 1) return fail(-1, "L_h must be >= 1");
    if (h->C > 1 && (p0 || log_u)) return fail(-1, "hyper_step on a multi-chain handle: no injected draws (out: one record per chain)");
    HIPCHK(hipSetDevice(h->device));
    const NetDev& nd = h->nd;
    const int C = h->C;
    int rc = ensure_current(h, nullptr);
    if (rc) return rc;
    const float* d_p0 = nullptr; const float* d_lu = nullptr;
    if (p0) { HIPCHK(hipMemcpyAsync(h->p0_inj, p0, (size_t)nd.H * sizeof(float), hipMemcpyHostToDevice, h->stream)); d_p0 = h->p0_inj; }
    if (log_u) { HIPCHK(hipMemcpyAsync(h->logu_inj, log_u, sizeof(float), hipMemcpyHostToDevice, h->stream)); d_lu = h->logu_inj; }
    HIPCHK(hipMemcpyAsync(h->eta_prev, h->eta, (size_t)C * nd.H * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    const float* d_each = nullptr;
    if (eps_each) {
        memcpy(h->epsh_host, eps_each, (size_t)C * sizeof(float));
        HIPCHK(hipMemcpyAsync(h->epsh, h->epsh_host, (size_t)C * sizeof(float), hipMemcpyHostToDevice, h->stream));
        d_each = h->epsh;
    }
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    // the hyper transition uses the epoch counter of the weight transition that preceded it
    const uint32_t ep = h->epoch > 0 ? h->epoch - 1 : 0;
    // (one workgroup runs one chain's whole hyper transition: the chains of a multi-chain handle side by side, gridDim.x = chain)
    static_assert(sizeof(float) * 4 == 16, "hyper work space: 4 H floats per chain (hyper_ws_bytes)");
    hipLaunchKernelGGL(k_hyper, dim3(C), dim3(HYP_THREADS), 0, h->stream, nd, (int)HYP_STEP, eps_h, (int)L_h, h->eta, (const float*)h->q_cur, rows_total(h),
                       d_p0, d_lu, ep, h->key0, h->key1, h->sc, h->hyp_ws, h->sc_out, h->seed_hi, d_each);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipMemcpyAsync(h->sc_host, h->sc_out, (size_t)C * sizeof(Scal), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0.f; hipEventElapsedTime(&ms, h->ev0, h->ev1);
    if (out)
        for (int c = 0; c < C; ++c) fill_out(h->sc_host[c], L_h, ms * 1000.f, 0.f, out + c);
    // eta changed => the weight target changed.  The prediction does not depend on eta: the cached statistic stays, the
    // data-term gradient rescales with sigma, the prior terms are recomputed -- O(P), no pass over the rows
    // (TBNN_HYPER_FULL_REFRESH=1: the round-1 behaviour, a whole bootstrap evaluation)
    bool any = false;
    for (int c = 0; c < C; ++c) any = any || h->sc_host[c].accepted;
    if (any) {
        static const bool full = getenv("TBNN_HYPER_FULL_REFRESH") && atoi(getenv("TBNN_HYPER_FULL_REFRESH"));
        if (full || !h->cur_valid) h->cur_valid = false;
        else {
            // one launch each for all chains (gridDim.y = chain); a chain whose hyper proposal was rejected returns at once, on the
            // device, by its record in sc_out (it keeps its cached gradient bit for bit)
            const Scal* gate = C > 1 ? (const Scal*)h->sc_out : (const Scal*)nullptr;
            hipLaunchKernelGGL(k_refresh_grad_after_hyper, dim3((nd.P + 255) / 256, C), dim3(256), 0, h->stream, nd,
                               (const float*)h->eta, (const float*)h->q_cur, (const float*)h->gd_cur, h->g_cur, gate);
            hipLaunchKernelGGL(k_energy, dim3(1, C), dim3(1024), 0, h->stream, nd, (int)EN_REFRESH, (const float*)h->eta,
                               (const float*)h->q_cur, (const float*)h->p, (const float*)h->q_cur,
                               stat_ptr(h), stat_entries(h), rows_total(h), lik_const(h), h->sc, (double*)nullptr,
                               (Scal*)nullptr, (const float*)nullptr, (float*)nullptr, (float*)nullptr, (const float*)nullptr, (float*)nullptr, gate);
            HIPCHK(hipGetLastError());
        }
    }
    return 0;
}

// predictor.trainProbs / reweight (predictor.py:188-206, :248-266): sum over the dense layers of calculateHyperProbs for m saved
// (theta, eta) pairs in ONE launch (grid.x = network).  priors: nl prior families to judge the layers under, or null (the chain's)
extern "C" int tbnn_hyper_probs_many(tbnn_handle h, const int32_t* priors, const float* thetas, int64_t theta_stride,
                                     const float* etas, int64_t eta_stride, int32_t m, double* out) {
    NEED(h);
    const NetDev& nd0 = h->nd;
    if (!thetas || !etas || !out || m < 1 || theta_stride < nd0.P || eta_stride < 4 * nd0.nl)
        return fail(-1, "hyper_probs_many: null pointer, m < 1, theta_stride < P or eta_stride < 4 * layers");
    NetDev nd = nd0;
    if (priors)
        for (int l = 0; l < nd.nl; ++l) {
            if (priors[l] != TBNN_PRIOR_CAUCHY && priors[l] != TBNN_PRIOR_GAUSSIAN) return fail(-1, "hyper_probs_many: unknown prior");
            nd.prior[l] = priors[l];
        }
    HIPCHK(hipSetDevice(h->device));
    Buf<float> dTh, dEt; Buf<double> dOut;
    const int chunk = (int)std::min<size_t>((size_t)m, std::max<size_t>(1, ((size_t)1 << 28) / (size_t)nd.P));      // <= 1 GiB of weights per pass
    HIPCHK(dTh.alloc((size_t)chunk * nd.P));
    HIPCHK(dEt.alloc((size_t)chunk * 4 * nd.nl));
    HIPCHK(dOut.alloc((size_t)chunk));
    for (int i0 = 0; i0 < m; i0 += chunk) {
        const int c = std::min(chunk, m - i0);
        HIPCHK(hipMemcpy2DAsync(dTh, (size_t)nd.P * sizeof(float), thetas + (size_t)i0 * theta_stride, (size_t)theta_stride * sizeof(float),
                                (size_t)nd.P * sizeof(float), (size_t)c, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpy2DAsync(dEt, (size_t)4 * nd.nl * sizeof(float), etas + (size_t)i0 * eta_stride, (size_t)eta_stride * sizeof(float),
                                (size_t)4 * nd.nl * sizeof(float), (size_t)c, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_hyper_probs, dim3(c), dim3(256), 0, h->stream, nd, (const float*)dTh, (long)nd.P, (const float*)dEt, (long)(4 * nd.nl), dOut);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + i0, dOut, (size_t)c * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

extern "C" int tbnn_export_sample_device(tbnn_handle h, float* d_out) {
    NEED(h); if (!d_out) return fail(-1, "null d_out");
    ONE_CHAIN(h, "tbnn_export_sample_device");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(d_out, h->q_cur, (size_t)h->nd.P * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_out + h->nd.P, h->eta, (size_t)h->nd.H * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// diagnostic (tests): the momentum the last trajectory ENDED with (p_L, after the closing half kick), whether or not the proposal
// was accepted -- what a time-reversal test needs (include/tbnn.h)
extern "C" int tbnn_debug_momentum(tbnn_handle h, float* p_out) {
    NEED(h); if (!p_out) return fail(-1, "null p_out");
    ONE_CHAIN(h, "tbnn_debug_momentum");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(p_out, h->p, (size_t)h->nd.P * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int tbnn_debug_draw(tbnn_handle h, uint32_t epoch, uint32_t purpose, int32_t n, float* out_normals,
                               float* out_log_u) {
    NEED(h);
    if (n < 1 || !out_normals) return fail(-1, "debug_draw: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    Buf<float> d;
    HIPCHK(d.alloc((size_t)n + 1));
    hipLaunchKernelGGL(k_debug_draw, dim3((n + 255) / 256), dim3(256), 0, h->stream, epoch, purpose, h->key0, h->key1, (int)n, d, d + n);
    HIPCHK(hipGetLastError());
    std::vector<float> host(n + 1);
    HIPCHK(hipMemcpyAsync(host.data(), d, (size_t)(n + 1) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(out_normals, host.data(), (size_t)n * sizeof(float));
    if (out_log_u) *out_log_u = host[n];
    return 0;
}

// diagnostic: stamps of workgroup 0 inside one fused launch (include/tbnn.h)
extern "C" int tbnn_debug_stamps(tbnn_handle h, uint64_t* out5) {
    if (!out5) return fail(-1, "null out16");
    NEED(h);
    const FusedOps* ops = h->be->ops();
    if (!ops || ops != narrow_find(h->nd) || !h->dX || h->C > 1) return fail(-1, "debug_stamps: narrow fast kernel + data required");
    HIPCHK(hipSetDevice(h->device));
    Buf<unsigned long long> d;
    HIPCHK(d.alloc(16));
    HIPCHK(hipMemset(d, 0, 16 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_make_image, dim3((h->nd.P + 255) / 256), dim3(256), 0, h->stream, h->nd.P, h->q_cur, h->imgmap, h->qimg_cur);
    for (int rep = 0; rep < 3; ++rep)
        if (narrow_launch_stamped(ops, h->grid, h->stream, h->nd, h->qimg_cur, h->eta, h->dX, h->dY, h->n, h->slabs, h->pitch, h->pstat, d))
            return fail(-2, "debug_stamps: launch failed");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out5, d, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tbnn_debug_fused_burst(tbnn_handle h, int32_t reps, float* us_per_pass) {
    if (!us_per_pass || reps < 1) return fail(-1, "fused_burst: reps >= 1 and an output pointer required");
    NEED(h);
    if (!h->dX) return fail(-1, "fused_burst: no data");
    if (h->shard) return fail(-1, "fused_burst: not on a row-sharded handle (every pass would be a collective; the other ranks are not in this call)");
    HIPCHK(hipSetDevice(h->device));
    const size_t PB = (size_t)h->C * h->nd.P * sizeof(float);
    // the proposal buffers (free between two transitions) take a copy of the current state; its image is built once
    HIPCHK(hipMemcpyAsync(h->q, h->q_cur, PB, hipMemcpyDeviceToDevice, h->stream));
    if (h->imgmap) {
        hipLaunchKernelGGL(k_make_image, dim3((h->nd.P + 255) / 256, h->C), dim3(256), 0, h->stream, h->nd.P, (const float*)h->q, h->imgmap, h->qimg, (long)h->nd.P,
                           (long)h->img_floats);
        h->q_img_valid = true;
    }
    struct ProfileOff {                                    // restored on EVERY exit (HIPCHK returns early)
        tbnn_ctx* h; int saved;
        explicit ProfileOff(tbnn_ctx* h_) : h(h_), saved(h_->profile) { h->profile = 0; }
        ~ProfileOff() { h->profile = saved; h->q_img_valid = false; }
    } guard(h);
    int rc = launch_fwd_bwd(h, h->q, h->eta);              // one untimed pass (first touch)
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int r = 0; r < reps && !rc; ++r) rc = launch_fwd_bwd(h, h->q, h->eta);
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    if (rc) return rc;
    HIPCHK(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *us_per_pass = ms * 1000.f / (float)reps;
    return 0;
}

#ifdef TBNN_TILE_STAMPS
// the stamps of the narrow kernels (tbnn_narrow.hip's copy) over those of the hyper step (this unit's copy, kernels_hyper.hpp: HSTAMP)
extern "C" int tbnn_debug_tile_stamps(tbnn_handle h, uint64_t* out64) {
    NEED(h);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_tile_stamps), 64 * sizeof(uint64_t)));
    unsigned long long narrow[64];
    if (tbnn_jit_tile_stamps(narrow)) return fail(-2, "tbnn_jit_tile_stamps failed");
    for (int k = 0; k < 64; ++k) if (narrow[k]) out64[k] = narrow[k];
    return 0;
}
#endif
