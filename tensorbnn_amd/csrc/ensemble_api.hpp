// libtbnn: the host side of tbnn_forward_many and the ensemble reductions (include/tbnn.h; kernels: kernels_ensemble.hpp).  Host code only,
// included by tbnn_api.hip alone, once, after tbnn_ctx, lik_known and the launch helpers (it uses them, and Buf, fail, HIPCHK and NEED).
// First what the entry points share -- uploads, result copies, argument checks, the block budget, the forward stage and its two drivers.
#pragma once
#define ENS_TRY(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

// count elements of src into buf, allocated here, on h->stream.  src is read when the copy runs: it must outlive the next synchronise
template <class T>
static int ens_upload(tbnn_ctx* h, Buf<T>& buf, const T* src, size_t count) {
    HIPCHK(buf.alloc(count));
    HIPCHK(hipMemcpyAsync(buf, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return 0;
}
// a block's result planes src[planes][r] -> the host result dst[planes][rows] at column r0
static int ens_copy_planes(tbnn_ctx* h, double* dst, long r0, long rows, const double* src, long r, size_t planes) {
    HIPCHK(hipMemcpy2DAsync(dst + r0, (size_t)rows * sizeof(double), src, (size_t)r * sizeof(double), (size_t)r * sizeof(double), planes,
                            hipMemcpyDeviceToHost, h->stream));
    return 0;
}

static int ens_check_xform(const std::string& who, int xform, int d_out) {
    if (xform < TBNN_XFORM_NONE || xform > TBNN_XFORM_SOFTMAX) return fail(-1, who + ": unknown transform");
    if (xform == TBNN_XFORM_SOFTMAX && d_out < 2) return fail(-1, who + ": a softmax needs at least 2 outputs (one logit per class)");
    return 0;
}
static int ens_check_lik(const std::string& who, int likelihood, int d_out, const float* X, const float* Y) {
    if (!lik_known(likelihood)) return fail(-1, who + ": unknown likelihood");
    if (likelihood == TBNN_LIK_CATEGORICAL && d_out < 2) return fail(-1, who + ": the categorical likelihood needs at least 2 outputs (one logit per class)");
    if (likelihood == TBNN_LIK_HETERO_GAUSSIAN && d_out != 2)
        return fail(-1, who + ": the heteroscedastic Gaussian likelihood needs exactly 2 outputs: mean and log-sd");
    if (X && !Y) return fail(-1, who + ": rows X without their targets Y");
    return 0;
}
static bool ens_gaussian(int likelihood) { return likelihood == TBNN_LIK_GAUSSIAN || likelihood == TBNN_LIK_FIXED_GAUSSIAN; }
// importance weights of the networks: the rules of tbnn_set_row_weights.  W = their sum (fp64, network order); null: equal, W = m
static int ens_check_weights(const std::string& who, const float* net_w, int32_t m, double* W) {
    double s = 0.0;
    for (int32_t i = 0; i < m; ++i) {
        if (!net_w) { s += 1.0; continue; }
        if (!std::isfinite(net_w[i])) return fail(-1, who + ": weight " + std::to_string(i) + " is not finite");
        if (net_w[i] < 0.f) return fail(-1, who + ": weight " + std::to_string(i) + " is negative");
        s += (double)net_w[i];
    }
    if (!(s > 0.0)) return fail(-1, who + ": all weights are zero");
    *W = s;
    return 0;
}
// per network under a Gaussian likelihood: sig[i] = sd[i] (null: fixed_sd) clipped to [1e-8, 1e8] in fp32 (layer.py:62) and, where cst is
// wanted, cst[i] = -log sigma - 1/2 log 2 pi from the clipped value widened
static int ens_sigmas(const std::string& who, const float* sd, float fixed_sd, int32_t m, std::vector<float>& sig, std::vector<double>* cst = nullptr) {
    sig.resize((size_t)m);
    if (cst) cst->resize((size_t)m);
    for (int32_t i = 0; i < m; ++i) {
        const float s = sd ? sd[i] : fixed_sd;
        if (std::isnan(s)) return fail(-1, who + ": sd " + std::to_string(i) + " is not a number");
        sig[i] = std::min(std::max(s, 1e-8f), 1e8f);
        if (cst) (*cst)[i] = -std::log((double)sig[i]) - 0.5 * std::log(2.0 * M_PI);
    }
    return 0;
}

// what tbnn_ensemble_loglik and tbnn_ensemble_loo stage per network: *scaled = the likelihood has a scale (the Gaussian kinds, Student-t) -- sig
// and cst as ens_sigmas forms them; under TBNN_LIK_STUDENT_T *nu = the handle's degrees of freedom (its descriptor's, or what
// tbnn_set_lik_df set on a handle of another likelihood; under TBNN_LIK_NEG_BINOMIAL the dispersion r, under TBNN_LIK_GAMMA the shape a and under TBNN_LIK_WEIBULL the shape k, by the same rule) and cst[i] = lgamma((nu+1)/2) - lgamma(nu/2) - 1/2 log(nu pi) - log sigma_i
static int ens_lik_consts(tbnn_ctx* h, const std::string& who, int likelihood, const float* sd, int32_t m, bool* scaled, std::vector<float>& sig,
                          std::vector<double>& cst, double* nu) {
    const bool student = likelihood == TBNN_LIK_STUDENT_T;
    *scaled = ens_gaussian(likelihood) || student;
    *nu = 0.0;
    if (student) {
        const float df = h->nd.lik == TBNN_LIK_STUDENT_T ? h->nd.lik_df : h->ens_df;
        if (!df_ok(df)) return fail(-1, who + ": judging under TBNN_LIK_STUDENT_T needs the degrees of freedom: call tbnn_set_lik_df on this handle first");
        *nu = (double)df;
    }
    if (likelihood == TBNN_LIK_NEG_BINOMIAL) {
        // the dispersion r travels where nu does: the descriptor's lik_df on a negative-binomial handle, else what tbnn_set_lik_df set
        const float r = h->nd.lik == TBNN_LIK_NEG_BINOMIAL ? h->nd.lik_df : h->ens_df;
        if (!df_ok(r)) return fail(-1, who + ": judging under TBNN_LIK_NEG_BINOMIAL needs the dispersion: call tbnn_set_lik_df on this handle first");
        *nu = (double)r;
    }
    if (likelihood == TBNN_LIK_GAMMA) {
        // the shape a travels where nu does: the descriptor's lik_df on a Gamma handle, else what tbnn_set_lik_df set
        const float a = h->nd.lik == TBNN_LIK_GAMMA ? h->nd.lik_df : h->ens_df;
        if (!df_ok(a)) return fail(-1, who + ": judging under TBNN_LIK_GAMMA needs the shape: call tbnn_set_lik_df on this handle first");
        *nu = (double)a;
    }
    if (likelihood == TBNN_LIK_WEIBULL) {
        // the shape k travels where nu does: the descriptor's lik_df on a Weibull handle, else what tbnn_set_lik_df set
        const float k = h->nd.lik == TBNN_LIK_WEIBULL ? h->nd.lik_df : h->ens_df;
        if (!df_ok(k)) return fail(-1, who + ": judging under TBNN_LIK_WEIBULL needs the shape: call tbnn_set_lik_df on this handle first");
        *nu = (double)k;
    }
    if (*scaled) ENS_TRY(ens_sigmas(who, sd, h->nd.fixed_sd, m, sig, &cst));
    if (student) {
        const double c0 = std::lgamma(0.5 * (*nu + 1.0)) - std::lgamma(0.5 * *nu) - 0.5 * std::log(*nu * M_PI);
        for (int32_t i = 0; i < m; ++i) cst[i] = c0 - std::log((double)sig[i]);
    }
    return 0;
}

// The targets of the rows an entry point judges: the caller's Y (n rows), or the ones staged with the rows `which` selects.  What can be
// refused before the driver touches the device is refused here; a `which` that selects nothing is left to EnsStage::stage_rows.
static int ens_check_targets(tbnn_ctx* h, const std::string& who, int which, const float* X, const float* Y, int64_t n) {
    if (X || (which != 0 && which != 1)) return 0;
    const long staged = which ? h->nv : h->n;
    if (staged < 1) return 0;
    if (Y && n != staged) return fail(-1, who + ": n = " + std::to_string((long long)n) + " does not match the " + std::to_string(staged) + " staged rows");
    if (!Y && !(which ? h->dYv : h->dY)) return fail(-1, who + ": no staged targets");
    return 0;
}
// ... and, inside a driver's begin (the rows are staged by then): the device pointer of those targets, the caller's uploaded into own
static int ens_stage_targets(tbnn_ctx* h, int which, const float* Y, int64_t n, Buf<float>& own, const float** dY) {
    if (Y) ENS_TRY(ens_upload(h, own, Y, (size_t)n * h->nd.d_out));
    *dY = Y ? (const float*)own : which ? (const float*)h->dYv : h->dY;
    return 0;
}

// networks per pass: the chunk of predictions stays below 1 GiB
static const size_t ENS_CHUNK_FLOATS = (size_t)1 << 28;
// the ensemble reductions alone: TBNN_ENS_CHUNK_FLOATS (debug) cuts the chunks smaller, so that a test reaches the carry-over between
// chunks with a small problem; tbnn_forward_many does not read it
// (the row-block entry points cut rows with it, in multiples of 64: there the value may be exceeded by up to 64 rows' worth)
static size_t ens_chunk_floats() {
    if (const char* e = getenv("TBNN_ENS_CHUNK_FLOATS")) { const long long v = atoll(e); if (v >= 1 && (size_t)v < ENS_CHUNK_FLOATS) return (size_t)v; }
    return ENS_CHUNK_FLOATS;
}
// The block rule of the entry points that need all m networks of a row at once.  Refused: 64 rows at per_row floats each above the
// budget.  *rb (where wanted): the rows of a block -- what keeps it within ens_chunk_floats(), read at every call, rounded down to a
// multiple of 64 and never below 64, so that a block starts as aligned within dX as dX itself is for the forward kernels' vector loads
// (the debug override may therefore be exceeded by up to 64 rows' worth) -- and never more than total.
static int ens_block_rows(const std::string& who, long total, size_t per_row, long* rb, const char* rows_of = "rows of all m networks") {
    if (per_row * 64 > ENS_CHUNK_FLOATS) return fail(-1, who + ": 64 " + rows_of + " exceed the block budget of 2^28 floats");
    if (rb) *rb = std::min<long>(total, std::max<long>(64, (long)(ens_chunk_floats() / per_row) / 64 * 64));
    return 0;
}
static int ens_grid(long items) { return (int)std::max<long>(1, std::min<long>((items + ENS_TB - 1) / ENS_TB, 4096)); }

// The forward stage both drivers run: the rows, the staged thetas, the predictions and the weight-image scratch of one call.  Every buffer
// is allocated once per call (Buf::alloc frees what it held, and hipFree synchronises the device), never per chunk or block.
struct EnsStage {
    tbnn_ctx* h;
    Buf<float> dXown, dTh, dOut, dImg;
    const float* dX = nullptr;            // the staged rows `which` selects, or the caller's n rows copied into dXown
    long rows = 0;

    // the arguments every entry point checks alike, and the rows
    int stage_rows(const std::string& who, const float* thetas, int32_t m, int64_t theta_stride, int which, const float* X, int64_t n) {
        if (!thetas || m < 1 || theta_stride < h->nd.P) return fail(-1, who + ": null pointer, m < 1 or theta_stride < P");
        HIPCHK(hipSetDevice(h->device));
        if (X) {
            if (n < 1) return fail(-1, who + ": n < 1");
            rows = (long)n;
            ENS_TRY(ens_upload(h, dXown, X, (size_t)rows * h->nd.d_in));
            dX = dXown;
        } else {
            if (which != 0 && which != 1) return fail(-1, "which must be 0 (training rows) or 1 (validation rows)");
            dX = which ? h->dXv : h->dX; rows = which ? h->nv : h->n;
            if (!dX || rows < 1) return fail(-1, which ? "tbnn_set_validation has not been called" : "tbnn_set_data has not been called");
        }
        return 0;
    }
    // room for `nets` networks' thetas and out_floats of predictions
    int alloc(int nets, size_t out_floats) {
        HIPCHK(dTh.alloc((size_t)nets * h->nd.P));
        HIPCHK(dOut.alloc(out_floats));
        return 0;
    }
    // one zeroed image per network of a pass where the backend runs them as one launch, else the handle's one image in turn
    int images(int nets) {
        if (!h->be->forward_batched()) return 0;
        HIPCHK(dImg.alloc((size_t)nets * h->img_floats));
        HIPCHK(hipMemsetAsync(dImg, 0, (size_t)nets * h->img_floats * sizeof(float), h->stream));
        return 0;
    }
    // c networks, theta_i = thetas + i * theta_stride, into dTh
    int upload_thetas(const float* thetas, int64_t theta_stride, int c) {
        HIPCHK(hipMemcpy2DAsync(dTh, (size_t)h->nd.P * sizeof(float), thetas, (size_t)theta_stride * sizeof(float), (size_t)h->nd.P * sizeof(float),
                                (size_t)c, hipMemcpyHostToDevice, h->stream));
        return 0;
    }
    // the c networks of dTh over rows [r0, r0 + r) into dOut[c][d_out][r]
    int forward(int c, long r0, long r) {
        ENS_TRY(h->be->forward(h->stream, c, dTh, dX + (size_t)r0 * h->nd.d_in, r, dOut, h->imgmap, dImg ? (float*)dImg : (float*)h->qimg_cur));
        HIPCHK(hipGetLastError());
        return 0;
    }
    int sync() { HIPCHK(hipStreamSynchronize(h->stream)); return 0; }
};

// The part tbnn_forward_many and the ensemble reductions share: m networks, theta_i = thetas + i * theta_stride, over the same rows.
// X == null: the staged rows selected by `which` (0 training, 1 validation); else n host rows.  The rows are staged, the networks cut
// into chunks whose predictions take at most chunk_floats floats, each chunk's weights (and, narrow shapes, images) built and its forward
// passes run into dOut[c][d_out][rows] on h->stream.  begin(rows, chunk) runs once before the first chunk (the consumer's buffers),
// each(i0, c, dOut, rows) after every chunk's forward passes are enqueued; the stream is synchronised after each chunk, and before an
// error is returned, so that no buffer is freed under a copy.
template <class Begin, class Each>
static int ensemble_forward(tbnn_ctx* h, const std::string& who, const float* thetas, int32_t m, int64_t theta_stride, int which, const float* X,
                            int64_t n, size_t chunk_floats, Begin&& begin, Each&& each) {
    EnsStage st{h};
    ENS_TRY(st.stage_rows(who, thetas, m, theta_stride, which, X, n));
    const size_t per_net = (size_t)st.rows * h->nd.d_out;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)m, chunk_floats / std::max<size_t>(per_net, 1)));
    int rc = begin(st.rows, chunk);
    if (!rc) rc = st.alloc(chunk, (size_t)chunk * per_net);
    if (!rc) rc = st.images(chunk);
    for (int i0 = 0; i0 < m && !rc; i0 += chunk) {
        const int c = std::min(chunk, m - i0);
        rc = st.upload_thetas(thetas + (size_t)i0 * theta_stride, theta_stride, c);
        if (!rc) rc = st.forward(c, 0, st.rows);
        if (!rc) rc = each(i0, c, (const float*)st.dOut, st.rows);
        if (!rc) rc = st.sync();
    }
    hipStreamSynchronize(h->stream);
    return rc;
}

// Quantiles, chain diagnostics, the predictive distribution and PSIS need all m networks of an element at once, so this driver cuts the
// ROWS where ensemble_forward cuts the networks: blocks of rb rows (ens_block_rows), every block's m forward passes into
// dOut[m][d_out][rb], then the transform (kernels_ensemble.hpp) and each(r0, r, rows, t): the consumer's kernels over t[m][d_out r] and its
// copies into the strided host result, on h->stream, which is synchronised after every block.  The consumer's per-block results are
// outside the budget: never more than the caller's own output.  extra_row_bytes: what a consumer keeps per row BESIDE the predictions in
// proportion to m (tbnn_ensemble_loo's matrix and tail), counted into the budget in floats; 0 for the others.  begin(rb) runs once before
// the first block (the consumer's buffers and staged arguments).  Thetas are staged once; be->forward builds a block's weight images into
// the stage's one scratch.
template <class Begin, class Each>
static int ensemble_row_blocks(tbnn_ctx* h, const std::string& who, const float* thetas, int32_t m, int64_t theta_stride, int xform, float scale,
                               float shift, int which, const float* X, int64_t n, Begin&& begin, Each&& each, size_t extra_row_bytes = 0) {
    const int d_out = h->nd.d_out;
    const size_t per_row = (size_t)m * (size_t)d_out + (extra_row_bytes + sizeof(float) - 1) / sizeof(float);
    ENS_TRY(ens_block_rows(who, 0, per_row, nullptr));
    EnsStage st{h};
    ENS_TRY(st.stage_rows(who, thetas, m, theta_stride, which, X, n));
    long rb = 0;
    ENS_TRY(ens_block_rows(who, st.rows, per_row, &rb));
    int rc = st.alloc(m, (size_t)m * d_out * rb);
    if (!rc) rc = st.upload_thetas(thetas, theta_stride, m);
    if (!rc) rc = begin(rb);
    if (!rc) rc = st.images(m);
    for (long r0 = 0; r0 < st.rows && !rc; r0 += rb) {
        const long r = std::min(rb, st.rows - r0), tot = r * d_out;
        rc = st.forward(m, r0, r);
        if (rc) break;
        float* t = st.dOut;
        if (xform == TBNN_XFORM_SOFTMAX)
            hipLaunchKernelGGL(k_ens_transform_softmax, dim3(ens_grid((long)m * r)), dim3(ENS_TB), 0, h->stream, t, m, r, d_out, scale, shift);
        else if (xform != TBNN_XFORM_NONE || scale != 1.f || shift != 0.f)
            hipLaunchKernelGGL(k_ens_transform, dim3(ens_grid((long)m * tot)), dim3(ENS_TB), 0, h->stream, t, (long)m * tot, xform, scale, shift);
        rc = each(r0, r, st.rows, (const float*)t);
        if (!rc) rc = st.sync();
    }
    hipStreamSynchronize(h->stream);
    return rc;
}

// Ensemble prediction (predictor.py:132-155).  out[m][d_out][n].
extern "C" int tbnn_forward_many(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int which, const float* X,
                                 int64_t n, float* out) {
    NEED(h);
    if (!out) return fail(-1, "forward_many: null pointer, m < 1 or theta_stride < P");
    const size_t d_out = (size_t)h->nd.d_out;
    return ensemble_forward(h, "forward_many", thetas, m, theta_stride, which, X, n, ENS_CHUNK_FLOATS, [](long, int) { return 0; },
                            [&](int i0, int c, const float* dOut, long rows) -> int {
                                const size_t per_net = (size_t)rows * d_out;
                                HIPCHK(hipMemcpyAsync(out + (size_t)i0 * per_net, dOut, (size_t)c * per_net * sizeof(float), hipMemcpyDeviceToHost, h->stream));
                                return 0;
                            });
}

extern "C" int tbnn_ensemble_moments(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, const float* net_w, int xform,
                                     float scale, float shift, int which, const float* X, int64_t n, double* mean_out, double* var_out) {
    NEED(h);
    const std::string who = "ensemble_moments";
    const int d_out = h->nd.d_out;
    if (!mean_out) return fail(-1, who + ": null mean_out");
    ENS_TRY(ens_check_xform(who, xform, d_out));
    if (m < 1) return fail(-1, who + ": null pointer, m < 1 or theta_stride < P");
    double W = 0.0;
    ENS_TRY(ens_check_weights(who, net_w, m, &W));
    Buf<double> acc;
    Buf<float> dW;
    long tot = 0;
    ENS_TRY(ensemble_forward(h, who, thetas, m, theta_stride, which, X, n, ens_chunk_floats(),
        [&](long rows, int) -> int {
            tot = rows * d_out;
            HIPCHK(acc.alloc(3 * (size_t)tot));
            if (net_w) ENS_TRY(ens_upload(h, dW, net_w, (size_t)m));
            return 0;
        },
        [&](int i0, int c, const float* dOut, long rows) -> int {
            const float* w = net_w ? dW + i0 : nullptr;
            if (xform == TBNN_XFORM_SOFTMAX)
                hipLaunchKernelGGL(k_ens_moments_softmax, dim3(ens_grid(rows)), dim3(ENS_TB), 0, h->stream, dOut, c, rows, d_out, scale, shift, w,
                                   (int)(i0 == 0), (double*)acc);
            else
                hipLaunchKernelGGL(k_ens_moments, dim3(ens_grid(tot)), dim3(ENS_TB), 0, h->stream, dOut, c, tot, xform, scale, shift, w, (int)(i0 == 0),
                                   (double*)acc);
            HIPCHK(hipGetLastError());
            return 0;
        }));
    hipLaunchKernelGGL(k_ens_moments_finish, dim3(ens_grid(tot)), dim3(ENS_TB), 0, h->stream, (double*)acc, tot, W);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(mean_out, acc, (size_t)tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (var_out) HIPCHK(hipMemcpyAsync(var_out, acc + tot, (size_t)tot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// Classification uncertainty: sums over networks like the moments', so the NETWORKS are cut (ensemble_forward), not the rows.  One device
// buffer carries S, V and A across the chunks and takes the finish kernel's two planes behind them: (2 d_out + 3) n doubles categorical,
// 5 d_out n Bernoulli.
extern "C" int tbnn_ensemble_uncertainty(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int likelihood, const float* net_w,
                                         int which, const float* X, int64_t n, double* prob_out, double* vote_out, double* total_out,
                                         double* aleatoric_out, double* epistemic_out) {
    NEED(h);
    const std::string who = "ensemble_uncertainty";
    const int d_out = h->nd.d_out;
    if (!prob_out && !vote_out && !total_out && !aleatoric_out && !epistemic_out) return fail(-1, who + ": every output is null");
    const bool cat = likelihood == TBNN_LIK_CATEGORICAL;
    if (likelihood == TBNN_LIK_WEIBULL)
        return fail(-1, who + ": the entropy split and the votes are those of a label, not of TBNN_LIK_WEIBULL's time to an event (tbnn_ensemble_predictive "
                              "gives its CDF and quantiles)");
    if (!cat && likelihood != TBNN_LIK_BERNOULLI)
        return fail(-1, who + ": the entropy split and the votes are those of a label: TBNN_LIK_BERNOULLI or TBNN_LIK_CATEGORICAL (regression and "
                              "count kinds: tbnn_ensemble_predictive and tbnn_ensemble_moments)");
    if (cat && d_out < 2) return fail(-1, who + ": the categorical likelihood needs at least 2 outputs (one logit per class)");
    if (m < 1) return fail(-1, who + ": null pointer, m < 1 or theta_stride < P");
    double W = 0.0;
    ENS_TRY(ens_check_weights(who, net_w, m, &W));
    Buf<double> acc;
    Buf<float> dW;
    long tot = 0, rt = 0, nrows = 0;
    ENS_TRY(ensemble_forward(h, who, thetas, m, theta_stride, which, X, n, ens_chunk_floats(),
        [&](long rows, int) -> int {
            nrows = rows;
            tot = rows * d_out;
            rt = cat ? rows : tot;                          // the entropies: one per row, Bernoulli one per element
            HIPCHK(acc.alloc(2 * (size_t)tot + 3 * (size_t)rt));
            if (net_w) ENS_TRY(ens_upload(h, dW, net_w, (size_t)m));
            return 0;
        },
        [&](int i0, int c, const float* dOut, long rows) -> int {
            const float* w = net_w ? dW + i0 : nullptr;
            if (cat)
                hipLaunchKernelGGL(k_ens_uncert_softmax, dim3(ens_grid(rows)), dim3(ENS_TB), 0, h->stream, dOut, c, rows, d_out, w, (int)(i0 == 0),
                                   (double*)acc);
            else
                hipLaunchKernelGGL(k_ens_uncert, dim3(ens_grid(tot)), dim3(ENS_TB), 0, h->stream, dOut, c, tot, w, (int)(i0 == 0), (double*)acc);
            HIPCHK(hipGetLastError());
            return 0;
        }));
    if (cat) hipLaunchKernelGGL(k_ens_uncert_finish_softmax, dim3(ens_grid(nrows)), dim3(ENS_TB), 0, h->stream, (double*)acc, nrows, d_out, W);
    else hipLaunchKernelGGL(k_ens_uncert_finish, dim3(ens_grid(tot)), dim3(ENS_TB), 0, h->stream, (double*)acc, tot, W);
    HIPCHK(hipGetLastError());
    // the buffer's planes in order: pbar, vote [d_out][n]; aleatoric, total, epistemic [rt]
    double* const outs[5] = {prob_out, vote_out, aleatoric_out, total_out, epistemic_out};
    const size_t offs[5] = {0, (size_t)tot, 2 * (size_t)tot, 2 * (size_t)tot + (size_t)rt, 2 * (size_t)tot + 2 * (size_t)rt};
    for (int k = 0; k < 5; ++k)
        if (outs[k]) HIPCHK(hipMemcpyAsync(outs[k], acc + offs[k], (size_t)(k < 2 ? tot : rt) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int tbnn_ensemble_quantiles(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, const float* net_w, int method,
                                       int xform, float scale, float shift, int which, const float* X, int64_t n, const double* probs,
                                       int32_t n_probs, double* out) {
    NEED(h);
    const std::string who = "ensemble_quantiles";
    const int d_out = h->nd.d_out;
    if (!probs || !out) return fail(-1, who + ": null probs or out");
    if (n_probs < 1 || n_probs > 64) return fail(-1, who + ": n_probs must be 1 .. 64");
    for (int32_t j = 0; j < n_probs; ++j)
        if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) return fail(-1, who + ": probability " + std::to_string(j) + " is not in [0, 1]");
    if (method != TBNN_QUANT_LINEAR && method != TBNN_QUANT_INVERTED_CDF) return fail(-1, who + ": unknown method");
    ENS_TRY(ens_check_xform(who, xform, d_out));
    if (m < 1) return fail(-1, who + ": null pointer, m < 1 or theta_stride < P");
    if (method == TBNN_QUANT_LINEAR && net_w) return fail(-1, who + ": TBNN_QUANT_LINEAR takes no weights (TBNN_QUANT_INVERTED_CDF does)");
    double W = 0.0;
    ENS_TRY(ens_check_weights(who, net_w, m, &W));
    Buf<float> dW;
    Buf<double> dP, dQ;
    // [2][n_probs]: p, and LINEAR's h = (m - 1) p as one rounded fp64 product (k_ens_quantiles)
    std::vector<double> ph(2 * (size_t)n_probs);
    for (int32_t j = 0; j < n_probs; ++j) { ph[j] = probs[j]; ph[n_probs + j] = (double)(m - 1) * probs[j]; }
    return ensemble_row_blocks(h, who, thetas, m, theta_stride, xform, scale, shift, which, X, n,
        [&](long rb) -> int {
            HIPCHK(dQ.alloc((size_t)n_probs * d_out * rb));
            ENS_TRY(ens_upload(h, dP, ph.data(), ph.size()));
            if (net_w) ENS_TRY(ens_upload(h, dW, net_w, (size_t)m));
            return 0;
        },
        [&](long r0, long r, long rows, const float* t) -> int {
            const long tot = r * d_out;
            const dim3 grid(ens_grid(tot)), tb(ENS_TB);
            const float* w = net_w ? (const float*)dW : nullptr;
            const double* p = dP;
            double* q = dQ;
            // up to half of ENS_QP probabilities (an interval's three): the kernel that carries half the slots
            if (net_w && n_probs <= ENS_QP / 2) hipLaunchKernelGGL((k_ens_quantiles<true, ENS_QP / 2>), grid, tb, 0, h->stream, t, m, tot, w, method, p, n_probs, W, q);
            else if (net_w) hipLaunchKernelGGL((k_ens_quantiles<true, ENS_QP>), grid, tb, 0, h->stream, t, m, tot, w, method, p, n_probs, W, q);
            else if (n_probs <= ENS_QP / 2) hipLaunchKernelGGL((k_ens_quantiles<false, ENS_QP / 2>), grid, tb, 0, h->stream, t, m, tot, w, method, p, n_probs, W, q);
            else hipLaunchKernelGGL((k_ens_quantiles<false, ENS_QP>), grid, tb, 0, h->stream, t, m, tot, w, method, p, n_probs, W, q);
            HIPCHK(hipGetLastError());
            return ens_copy_planes(h, out, r0, rows, q, r, (size_t)n_probs * d_out);
        });
}

// the checks of the chain structure both diagnostics entry points share: S = m / n_chains draws per chain
static int diag_check(const std::string& who, int32_t m, int32_t n_chains, const double* rhat_out, const double* ess_out) {
    if (!rhat_out && !ess_out) return fail(-1, who + ": rhat_out and ess_out are both null");
    if (n_chains < 1 || n_chains > ENS_MAX_CHAINS) return fail(-1, who + ": n_chains must be 1 .. " + std::to_string(ENS_MAX_CHAINS));
    if (m < 1) return fail(-1, who + ": null pointer, m < 1 or theta_stride < P");
    if (m % n_chains) return fail(-1, who + ": m is not divisible by n_chains");
    if (m / n_chains < 8) return fail(-1, who + ": fewer than 8 draws per chain");
    return 0;
}

// k_ens_diagnostics over one block t[m][tot]; dR / dE: [tot] each, null where the result is not wanted
static int diag_launch(tbnn_ctx* h, const float* t, int32_t m, int32_t n_chains, long tot, double* dMu, double* dR, double* dE) {
    hipLaunchKernelGGL(k_ens_diagnostics, dim3(ens_grid(tot)), dim3(ENS_TB), 0, h->stream, t, (int)n_chains, (int)(m / n_chains), tot, dMu, dR, dE);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int tbnn_ensemble_diagnostics(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int32_t n_chains, int xform,
                                         float scale, float shift, int which, const float* X, int64_t n, double* rhat_out, double* ess_out) {
    NEED(h);
    const std::string who = "ensemble_diagnostics";
    const int d_out = h->nd.d_out;
    ENS_TRY(diag_check(who, m, n_chains, rhat_out, ess_out));
    ENS_TRY(ens_check_xform(who, xform, d_out));
    Buf<double> dMu, dRE;
    long rbk = 0;
    return ensemble_row_blocks(h, who, thetas, m, theta_stride, xform, scale, shift, which, X, n,
        [&](long rb) -> int {
            rbk = rb * d_out;
            HIPCHK(dMu.alloc(2 * (size_t)n_chains * rbk));
            HIPCHK(dRE.alloc(2 * (size_t)rbk));
            return 0;
        },
        [&](long r0, long r, long rows, const float* t) -> int {
            ENS_TRY(diag_launch(h, t, m, n_chains, r * d_out, dMu, rhat_out ? (double*)dRE : nullptr, ess_out ? dRE + rbk : nullptr));
            if (rhat_out) ENS_TRY(ens_copy_planes(h, rhat_out, r0, rows, dRE, r, (size_t)d_out));
            if (ess_out) ENS_TRY(ens_copy_planes(h, ess_out, r0, rows, dRE + rbk, r, (size_t)d_out));
            return 0;
        });
}

// The same kernel over a caller's series: no forward pass, nothing staged on the handle is read.  The columns are cut into blocks of cb
// (ens_block_rows at m floats per column), each uploaded as [m][cb].
extern "C" int tbnn_series_diagnostics(tbnn_handle h, const float* series, int32_t m, int64_t tot, int32_t n_chains, double* rhat_out,
                                       double* ess_out) {
    NEED(h);
    const std::string who = "series_diagnostics";
    ENS_TRY(diag_check(who, m, n_chains, rhat_out, ess_out));
    if (!series || tot < 1) return fail(-1, who + ": null series or tot < 1");
    long cb = 0;
    ENS_TRY(ens_block_rows(who, (long)tot, (size_t)m, &cb, "columns of all m draws"));
    HIPCHK(hipSetDevice(h->device));
    Buf<float> dT;
    Buf<double> dMu, dRE;
    HIPCHK(dT.alloc((size_t)m * cb));
    HIPCHK(dMu.alloc(2 * (size_t)n_chains * cb));
    HIPCHK(dRE.alloc(2 * (size_t)cb));
    for (long c0 = 0; c0 < (long)tot; c0 += cb) {
        const long c = std::min(cb, (long)tot - c0);
        HIPCHK(hipMemcpy2DAsync(dT, (size_t)c * sizeof(float), series + c0, (size_t)tot * sizeof(float), (size_t)c * sizeof(float), (size_t)m,
                                hipMemcpyHostToDevice, h->stream));
        ENS_TRY(diag_launch(h, dT, m, n_chains, c, dMu, rhat_out ? (double*)dRE : nullptr, ess_out ? dRE + cb : nullptr));
        if (rhat_out) HIPCHK(hipMemcpyAsync(rhat_out + c0, dRE, (size_t)c * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (ess_out) HIPCHK(hipMemcpyAsync(ess_out + c0, dRE + cb, (size_t)c * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

extern "C" int tbnn_ensemble_loglik(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int likelihood, const float* sd,
                                    const float* net_w, int which, const float* X, const float* Y, int64_t n, double* per_net,
                                    double* lppd_rows) {
    NEED(h);
    const std::string who = "ensemble_loglik";
    const int d_out = h->nd.d_out;
    if (!per_net && !lppd_rows) return fail(-1, who + ": per_net and lppd_rows are both null");
    ENS_TRY(ens_check_lik(who, likelihood, d_out, X, Y));
    if (m < 1) return fail(-1, who + ": null pointer, m < 1 or theta_stride < P");
    double W = 0.0;
    ENS_TRY(ens_check_weights(who, net_w, m, &W));
    // per network: sigma, the constant of the density (Gaussian kinds: -log sigma - 1/2 log 2 pi; Student-t: ens_lik_consts), log w
    bool gauss = false;                  // (the likelihood has a scale: the Gaussian kinds and Student-t)
    double nu = 0.0;
    std::vector<float> sig;
    std::vector<double> cst, lw;
    ENS_TRY(ens_lik_consts(h, who, likelihood, sd, m, &gauss, sig, cst, &nu));
    if (net_w && lppd_rows) {
        lw.resize((size_t)m);
        for (int32_t i = 0; i < m; ++i) lw[i] = std::log((double)net_w[i]);          // (log 0 = -inf: the network drops out of the mixture)
    }
    ENS_TRY(ens_check_targets(h, who, which, X, Y, n));
    Buf<float> dSig, dY;
    Buf<double> dCst, dLw, lse, part;
    std::vector<double> hpart;
    const float* dYrows = nullptr;
    int nblk = 0;
    long nrows = 0;
    ENS_TRY(ensemble_forward(h, who, thetas, m, theta_stride, which, X, n, ens_chunk_floats(),
        [&](long rows, int chunk) -> int {
            nrows = rows;
            ENS_TRY(ens_stage_targets(h, which, Y, n, dY, &dYrows));
            nblk = (int)((rows + ENS_TB - 1) / ENS_TB);
            if (gauss) {
                ENS_TRY(ens_upload(h, dSig, sig.data(), (size_t)m));
                ENS_TRY(ens_upload(h, dCst, cst.data(), (size_t)m));
            }
            if (!lw.empty()) ENS_TRY(ens_upload(h, dLw, lw.data(), (size_t)m));
            if (lppd_rows) HIPCHK(lse.alloc(2 * (size_t)rows));
            if (per_net) {
                HIPCHK(part.alloc((size_t)nblk * chunk));
                hpart.resize((size_t)nblk * chunk);
                for (int32_t i = 0; i < m; ++i) per_net[i] = 0.0;
            }
            return 0;
        },
        [&](int i0, int c, const float* dOut, long rows) -> int {
            hipLaunchKernelGGL(k_ens_loglik, dim3(nblk), dim3(ENS_TB), 0, h->stream, dOut, c, rows, d_out, likelihood, dYrows,
                               gauss ? (const float*)(dSig + i0) : nullptr, gauss ? (const double*)(dCst + i0) : nullptr,
                               lw.empty() ? nullptr : (const double*)(dLw + i0), (int)(i0 == 0), (double*)lse, (double*)part, nu);
            HIPCHK(hipGetLastError());
            if (per_net) {
                // the workgroups' partial sums of this chunk, added in index order: the same bits from run to run
                HIPCHK(hipMemcpyAsync(hpart.data(), part, (size_t)nblk * c * sizeof(double), hipMemcpyDeviceToHost, h->stream));
                HIPCHK(hipStreamSynchronize(h->stream));
                for (int b = 0; b < nblk; ++b) for (int i = 0; i < c; ++i) per_net[i0 + i] += hpart[(size_t)b * c + i];
            }
            return 0;
        }));
    if (lppd_rows) {
        hipLaunchKernelGGL(k_ens_lppd_finish, dim3(ens_grid(nrows)), dim3(ENS_TB), 0, h->stream, (double*)lse, nrows, std::log(W));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(lppd_rows, lse, (size_t)nrows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

// Phi^-1(p), 0 < p < 1: Wichura's algorithm AS 241 (Applied Statistics 37 (1988) 477-484), routine PPND16, about 1e-16 relative
static double ens_norm_ppf(double p) {
    const double q = p - 0.5;
    if (std::fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return q * (((((((2.5090809287301226727e3 * r + 3.3430575583588128105e4) * r + 6.7265770927008700853e4) * r + 4.5921953931549871457e4) * r +
                        1.3731693765509461125e4) * r + 1.9715909503065514427e3) * r + 1.3314166789178437745e2) * r + 3.3871328727963666080e0) /
               (((((((5.2264952788528545610e3 * r + 2.8729085735721942674e4) * r + 3.9307895800092710610e4) * r + 2.1213794301586595867e4) * r +
                    5.3941960214247511077e3) * r + 6.8718700749205790830e2) * r + 4.2313330701600911252e1) * r + 1.0);
    }
    double r = std::sqrt(-std::log(q < 0.0 ? p : 1.0 - p)), v;
    if (r <= 5.0) {
        r -= 1.6;
        v = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r + 1.27045825245236838258e0) * r +
                3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r + 4.63033784615654529590e0) * r + 1.42343711074968357734e0) /
            (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
                6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r + 2.05319162663775882187e0) * r + 1.0);
    } else {
        r -= 5.0;
        v = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
                2.96560571828504891230e-1) * r + 1.78482653991729133580e0) * r + 5.46378491116411436990e0) * r + 6.65790464350110377720e0) /
            (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
                1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r + 5.99832206555887937690e-1) * r + 1.0);
    }
    return q < 0.0 ? -v : v;
}

// the p-quantile of the standard Gamma(a, 1) distribution, for the bracket of k_ens_pred_quantiles alone (the kernel verifies and repairs
// the bracket, so this is a seed, not a result): outward from a by factors of 4 until P(a, lo) < p <= P(a, hi) by ens_gamma_p compiled for
// the host, then bisection on the log scale
static double ens_std_gamma_ppf(double a, double p) {
    double lo = a, hi = a;
    for (int k = 0; k < 600 && !(ens_gamma_p(a, lo) < p) && lo > 1e-300; ++k) lo *= 0.25;
    for (int k = 0; k < 600 && !(ens_gamma_p(a, hi) >= p) && hi < 1e300; ++k) hi *= 4.0;
    for (int k = 0; k < 200 && hi > lo * (1.0 + 4e-16); ++k) {
        const double mid = std::sqrt(lo) * std::sqrt(hi);
        if (!(mid > lo && mid < hi)) break;
        if (ens_gamma_p(a, mid) >= p) hi = mid; else lo = mid;
    }
    return hi;
}

// what tbnn_ensemble_predictive refuses before it touches a device, and the per-network constants it stages: cst[3][m] = w_i / W,
// 1 / (s_i sqrt 2), s_i (the last two: Gaussian kinds); pz[2][n_probs] = p, Phi^-1(p) (TBNN_LIK_WEIBULL: p, (-log1p(-p))^(1 / shape), the standard Weibull quantile; TBNN_LIK_GAMMA: p, g_p / shape, g_p the standard
// Gamma(shape, 1) quantile -- the caller passes the shape, 0 otherwise); *smax = the largest s_i among the networks that count
static int pred_check(const std::string& who, int likelihood, float fixed_sd, int d_out, const float* sd, const float* net_w, int32_t m, const float* X,
                      const float* Y, const double* probs, int32_t n_probs, const double* q_out, const double* cdf_out, const double* cdf_below_out,
                      std::vector<double>& cst, std::vector<double>& pz, double* smax, double shape) {
    if (!q_out && !cdf_out) return fail(-1, who + ": q_out and cdf_out are both null");
    if (q_out && !probs) return fail(-1, who + ": null probs with q_out");
    if (cdf_below_out && !cdf_out) return fail(-1, who + ": cdf_below_out without cdf_out");
    if (cdf_out && X && !Y) return fail(-1, who + ": rows X without their targets Y");
    if (q_out) {
        if (n_probs < 1 || n_probs > 64) return fail(-1, who + ": n_probs must be 1 .. 64");
        for (int32_t j = 0; j < n_probs; ++j)
            if (!(probs[j] > 0.0 && probs[j] < 1.0)) return fail(-1, who + ": probability " + std::to_string(j) + " is not in (0, 1)");
    }
    if (likelihood == TBNN_LIK_BERNOULLI || likelihood == TBNN_LIK_CATEGORICAL)
        return fail(-1, who + ": the predictive distribution of a label is its posterior-mean probability: tbnn_ensemble_moments returns it");
    if (likelihood == TBNN_LIK_STUDENT_T)
        return fail(-1, who + ": the Student-t predictive distribution (a mixture of t CDFs: the incomplete beta function on the device) is not built");
    const bool gauss = ens_gaussian(likelihood), het = likelihood == TBNN_LIK_HETERO_GAUSSIAN;
    const bool wei = likelihood == TBNN_LIK_WEIBULL, gam = likelihood == TBNN_LIK_GAMMA || wei;       // (gam: a continuous kind on the positive axis)
    if (!gauss && !het && !gam && likelihood != TBNN_LIK_POISSON && likelihood != TBNN_LIK_NEG_BINOMIAL) return fail(-1, who + ": unknown likelihood");
    // (heteroscedastic Gaussian: every network brings its own s_i(x) = exp(gc_i) in output 1 -- sd is not read, cst keeps w_i / W alone)
    if (het && d_out != 2) return fail(-1, who + ": the heteroscedastic Gaussian likelihood needs exactly 2 outputs: mean and log-sd");
    // (the wording predates the negative binomial, which takes cdf_below_out too; tests match on it)
    if (cdf_below_out && (gauss || het || gam)) return fail(-1, who + ": cdf_below_out is for TBNN_LIK_POISSON (a continuous CDF has no step)");
    if (m < 1) return fail(-1, who + ": null pointer, m < 1 or theta_stride < P");
    // the budget of ensemble_row_blocks, judged here before m values of sd and net_w are read and 3 m doubles staged
    ENS_TRY(ens_block_rows(who, 0, (size_t)m * (size_t)d_out, nullptr));
    if (!q_out) n_probs = 0;                                                          // (not read, whatever the caller left there)
    double W = 0.0;
    ENS_TRY(ens_check_weights(who, net_w, m, &W));
    std::vector<float> sig;
    if (gauss) ENS_TRY(ens_sigmas(who, sd, fixed_sd, m, sig));
    cst.assign(3 * (size_t)m, 0.0);
    *smax = 0.0;
    for (int32_t i = 0; i < m; ++i) {
        cst[i] = (net_w ? (double)net_w[i] : 1.0) / W;
        if (!gauss) continue;
        const double sc = (double)sig[i];
        cst[(size_t)m + i] = 1.0 / (sc * std::sqrt(2.0));
        cst[2 * (size_t)m + i] = sc;
        if (cst[i] > 0.0) *smax = std::max(*smax, sc);
    }
    pz.assign(2 * (size_t)std::max(n_probs, 1), 0.0);
    for (int32_t j = 0; j < n_probs; ++j) {
        pz[j] = probs[j];
        // (a Weibull shape so small that the standard quantile leaves fp64's normal range would seed a bracket end of 0 or inf)
        if (wei) {
            const double g = std::pow(-std::log1p(-probs[j]), 1.0 / shape);
            if (!(g >= 0x1p-1022 && g < (double)INFINITY))
                return fail(-1, who + ": the standard Weibull quantile (-log1p(-p))^(1/k) at one of the probabilities is not a normal fp64 number: the shape is too small for it");
        }
        pz[(size_t)n_probs + j] = wei ? std::pow(-std::log1p(-probs[j]), 1.0 / shape) : gam ? ens_std_gamma_ppf(shape, probs[j]) / shape : ens_norm_ppf(probs[j]);
    }
    return 0;
}

extern "C" int tbnn_ensemble_predictive(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int likelihood, const float* sd,
                                        const float* net_w, int which, const float* X, const float* Y, int64_t n, const double* probs,
                                        int32_t n_probs, double* q_out, double* cdf_out, double* cdf_below_out) {
    NEED(h);
    const std::string who = "ensemble_predictive";
    const int d_out = h->nd.d_out;
    std::vector<double> cst, pz;
    double smax = 0.0;
    // the shape of the Gamma likelihood: the descriptor's lik_df on such a handle, what tbnn_set_lik_df set on any other
    const bool gam = likelihood == TBNN_LIK_GAMMA, wei = likelihood == TBNN_LIK_WEIBULL;
    double shape = 0.0;
    if (wei) {
        // (the Weibull likelihood's: by the same rule)
        const float k = h->nd.lik == TBNN_LIK_WEIBULL ? h->nd.lik_df : h->ens_df;
        if (!df_ok(k)) return fail(-1, who + ": the predictive distribution under TBNN_LIK_WEIBULL needs the shape: call tbnn_set_lik_df on this handle first");
        shape = (double)k;
    }
    if (gam) {
        const float a = h->nd.lik == TBNN_LIK_GAMMA ? h->nd.lik_df : h->ens_df;
        if (!df_ok(a)) return fail(-1, who + ": the predictive distribution under TBNN_LIK_GAMMA needs the shape: call tbnn_set_lik_df on this handle first");
        shape = (double)a;
    }
    ENS_TRY(pred_check(who, likelihood, h->nd.fixed_sd, d_out, sd, net_w, m, X, Y, probs, n_probs, q_out, cdf_out, cdf_below_out, cst, pz, &smax, shape));
    if (!q_out) n_probs = 0;
    const bool pois = likelihood == TBNN_LIK_POISSON, negb = likelihood == TBNN_LIK_NEG_BINOMIAL, het = likelihood == TBNN_LIK_HETERO_GAUSSIAN;
    // result planes per row: one per output; the heteroscedastic Gaussian's two outputs describe ONE distribution per row
    const int od = het ? 1 : d_out;
    // the dispersion of the negative binomial: the descriptor's lik_df on such a handle, what tbnn_set_lik_df set on any other
    double disp = shape;
    if (negb) {
        const float r = h->nd.lik == TBNN_LIK_NEG_BINOMIAL ? h->nd.lik_df : h->ens_df;
        if (!df_ok(r)) return fail(-1, who + ": the predictive distribution under TBNN_LIK_NEG_BINOMIAL needs the dispersion: call tbnn_set_lik_df on this handle first");
        disp = (double)r;
    }
    if (cdf_out) ENS_TRY(ens_check_targets(h, who, which, X, Y, n));
    const float* dYrows = nullptr;
    Buf<float> dY;
    Buf<double> dCst, dP, dRes;
    long rbk = 0;
    return ensemble_row_blocks(h, who, thetas, m, theta_stride, TBNN_XFORM_NONE, 1.f, 0.f, which, X, n,
        [&](long rb) -> int {
            rbk = rb * od;
            // a block's results: n_probs quantile planes, then the CDF and the CDF below
            HIPCHK(dRes.alloc(((size_t)n_probs + 2) * rbk));
            ENS_TRY(ens_upload(h, dCst, cst.data(), cst.size()));
            ENS_TRY(ens_upload(h, dP, pz.data(), pz.size()));
            if (cdf_out) ENS_TRY(ens_stage_targets(h, which, Y, n, dY, &dYrows));
            return 0;
        },
        [&](long r0, long r, long rows, const float* t) -> int {
            const long tot = r * od;                       // elements: (output, row) pairs; heteroscedastic Gaussian: rows
            const dim3 grid(ens_grid(tot)), tb(ENS_TB);
            const double* c = dCst;
            const double* p = dP;
            double* q = dRes;
            double* F = dRes + (size_t)n_probs * rbk;
            double* Fb = cdf_below_out ? F + rbk : nullptr;
            if (q_out) {
                if (pois) hipLaunchKernelGGL((k_ens_pred_quantiles<TBNN_LIK_POISSON, ENS_PQ>), grid, tb, 0, h->stream, t, m, tot, c, p, n_probs, smax, q, disp);
                else if (negb) hipLaunchKernelGGL((k_ens_pred_quantiles<TBNN_LIK_NEG_BINOMIAL, ENS_PQ>), grid, tb, 0, h->stream, t, m, tot, c, p, n_probs, smax, q, disp);
                else if (gam) hipLaunchKernelGGL((k_ens_pred_quantiles<TBNN_LIK_GAMMA, ENS_PQ>), grid, tb, 0, h->stream, t, m, tot, c, p, n_probs, smax, q, disp);
                else if (wei) hipLaunchKernelGGL((k_ens_pred_quantiles<TBNN_LIK_WEIBULL, ENS_PQ>), grid, tb, 0, h->stream, t, m, tot, c, p, n_probs, smax, q, disp);
                else if (het) hipLaunchKernelGGL((k_ens_pred_quantiles<TBNN_LIK_HETERO_GAUSSIAN, ENS_PQ>), grid, tb, 0, h->stream, t, m, tot, c, p, n_probs, smax, q, disp);
                else hipLaunchKernelGGL((k_ens_pred_quantiles<TBNN_LIK_GAUSSIAN, ENS_PQ>), grid, tb, 0, h->stream, t, m, tot, c, p, n_probs, smax, q, disp);
                HIPCHK(hipGetLastError());
                ENS_TRY(ens_copy_planes(h, q_out, r0, rows, q, r, (size_t)n_probs * od));
            }
            if (cdf_out) {
                const float* y = dYrows + (size_t)r0 * d_out;
                if (pois) hipLaunchKernelGGL(k_ens_pred_cdf<TBNN_LIK_POISSON>, grid, tb, 0, h->stream, t, m, tot, r, d_out, y, c, F, Fb, disp);
                else if (negb) hipLaunchKernelGGL(k_ens_pred_cdf<TBNN_LIK_NEG_BINOMIAL>, grid, tb, 0, h->stream, t, m, tot, r, d_out, y, c, F, Fb, disp);
                else if (gam) hipLaunchKernelGGL(k_ens_pred_cdf<TBNN_LIK_GAMMA>, grid, tb, 0, h->stream, t, m, tot, r, d_out, y, c, F, Fb, disp);
                else if (wei) hipLaunchKernelGGL(k_ens_pred_cdf<TBNN_LIK_WEIBULL>, grid, tb, 0, h->stream, t, m, tot, r, d_out, y, c, F, Fb, disp);
                else if (het) hipLaunchKernelGGL(k_ens_pred_cdf<TBNN_LIK_HETERO_GAUSSIAN>, grid, tb, 0, h->stream, t, m, tot, r, d_out, y, c, F, Fb, disp);
                else hipLaunchKernelGGL(k_ens_pred_cdf<TBNN_LIK_GAUSSIAN>, grid, tb, 0, h->stream, t, m, tot, r, d_out, y, c, F, Fb, disp);
                HIPCHK(hipGetLastError());
                ENS_TRY(ens_copy_planes(h, cdf_out, r0, rows, F, r, (size_t)od));
                if (Fb) ENS_TRY(ens_copy_planes(h, cdf_below_out, r0, rows, Fb, r, (size_t)od));
            }
            return 0;
        });
}

// what tbnn_ensemble_crps refuses before it touches a device, and the per-network constants it stages: cst[2][m] = w_i / W and, Gaussian
// kinds with noise, s_i (with noise = 0 sd is not read)
static int crps_check(const std::string& who, int likelihood, float fixed_sd, int d_out, const float* sd, const float* net_w, int32_t m, const float* X,
                      const float* Y, int noise, const double* crps_out, const double* error_out, const double* spread_out, std::vector<double>& cst) {
    if (!crps_out && !error_out && !spread_out) return fail(-1, who + ": every output is null");
    if (X && !Y) return fail(-1, who + ": rows X without their targets Y");
    if (noise != 0 && noise != 1) return fail(-1, who + ": noise must be 0 (the networks' outputs alone) or 1 (with the observation noise)");
    if (likelihood == TBNN_LIK_BERNOULLI || likelihood == TBNN_LIK_CATEGORICAL)
        return fail(-1, who + ": the CRPS is a score of a real-valued prediction; a label's uncertainty and calibration: tbnn_ensemble_uncertainty");
    if (likelihood == TBNN_LIK_POISSON || likelihood == TBNN_LIK_NEG_BINOMIAL)
        return fail(-1, who + ": the CRPS of a count distribution is not built (the pair term E|Y_i - Y_j| of two count distributions has no closed "
                              "form: a sum of (F(k) - 1{y <= k})^2 over the support, another kernel)");
    if (likelihood == TBNN_LIK_GAMMA)
        return fail(-1, who + ": the CRPS under TBNN_LIK_GAMMA is not built (the pair term E|Y_i - Y_j| of two Gamma distributions has no closed form)");
    if (likelihood == TBNN_LIK_WEIBULL)
        return fail(-1, who + ": the CRPS under TBNN_LIK_WEIBULL is not built (no kernel forms the pair term E|Y_i - Y_j| of two Weibull distributions, and a censored "
                              "row has no observed value to score)");
    if (likelihood == TBNN_LIK_STUDENT_T)
        return fail(-1, who + ": the CRPS under TBNN_LIK_STUDENT_T is not built (the pair term of two t distributions has no closed form, and the "
                              "Student-t predictive distribution is not built either)");
    const bool gauss = ens_gaussian(likelihood), het = likelihood == TBNN_LIK_HETERO_GAUSSIAN;
    if (!gauss && !het) return fail(-1, who + ": unknown likelihood");
    if (het && d_out != 2) return fail(-1, who + ": the heteroscedastic Gaussian likelihood needs exactly 2 outputs: mean and log-sd");
    if (m < 1) return fail(-1, who + ": null pointer, m < 1 or theta_stride < P");
    if (m > ENS_CRPS_MAX_M)
        return fail(-1, who + ": m = " + std::to_string(m) + " exceeds " + std::to_string(ENS_CRPS_MAX_M) + " networks (the work is quadratic in m)");
    ENS_TRY(ens_block_rows(who, 0, (size_t)m * (size_t)d_out, nullptr));
    double W = 0.0;
    ENS_TRY(ens_check_weights(who, net_w, m, &W));
    std::vector<float> sig;
    const bool scales = gauss && noise;
    if (scales) ENS_TRY(ens_sigmas(who, sd, fixed_sd, m, sig));
    cst.assign(2 * (size_t)m, 0.0);
    for (int32_t i = 0; i < m; ++i) {
        cst[i] = (net_w ? (double)net_w[i] : 1.0) / W;
        if (scales) cst[(size_t)m + i] = (double)sig[i];
    }
    return 0;
}

// The CRPS of the predictive mixture: every (output, row) needs all m networks at once, so the rows are cut (ensemble_row_blocks); a block's
// three result planes are held beside it.
extern "C" int tbnn_ensemble_crps(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int likelihood, const float* sd,
                                  const float* net_w, int which, const float* X, const float* Y, int64_t n, int noise, double* crps_out,
                                  double* error_out, double* spread_out) {
    NEED(h);
    const std::string who = "ensemble_crps";
    const int d_out = h->nd.d_out;
    std::vector<double> cst;
    ENS_TRY(crps_check(who, likelihood, h->nd.fixed_sd, d_out, sd, net_w, m, X, Y, noise, crps_out, error_out, spread_out, cst));
    const bool het = likelihood == TBNN_LIK_HETERO_GAUSSIAN;
    const int od = het ? 1 : d_out;                          // (its two outputs describe ONE distribution per row)
    ENS_TRY(ens_check_targets(h, who, which, X, Y, n));
    const float* dYrows = nullptr;
    Buf<float> dY;
    Buf<double> dCst, dRes;
    long rbk = 0;
    return ensemble_row_blocks(h, who, thetas, m, theta_stride, TBNN_XFORM_NONE, 1.f, 0.f, which, X, n,
        [&](long rb) -> int {
            rbk = rb * od;
            HIPCHK(dRes.alloc(3 * (size_t)rbk));
            ENS_TRY(ens_upload(h, dCst, cst.data(), cst.size()));
            return ens_stage_targets(h, which, Y, n, dY, &dYrows);
        },
        [&](long r0, long r, long rows, const float* t) -> int {
            const long tot = r * od;                       // elements: (output, row) pairs; heteroscedastic Gaussian: rows
            const dim3 grid((unsigned)std::min<long>((tot + ENS_CE - 1) / ENS_CE, 65536)), tb(ENS_TB);
            const float* y = dYrows + (size_t)r0 * d_out;
            const double* c = dCst;
            double* res = dRes;
            if (het && noise) hipLaunchKernelGGL((k_ens_crps<TBNN_LIK_HETERO_GAUSSIAN, true>), grid, tb, 0, h->stream, t, (int)m, tot, r, d_out, y, c, res, rbk);
            else if (het) hipLaunchKernelGGL((k_ens_crps<TBNN_LIK_HETERO_GAUSSIAN, false>), grid, tb, 0, h->stream, t, (int)m, tot, r, d_out, y, c, res, rbk);
            else if (noise) hipLaunchKernelGGL((k_ens_crps<TBNN_LIK_GAUSSIAN, true>), grid, tb, 0, h->stream, t, (int)m, tot, r, d_out, y, c, res, rbk);
            else hipLaunchKernelGGL((k_ens_crps<TBNN_LIK_GAUSSIAN, false>), grid, tb, 0, h->stream, t, (int)m, tot, r, d_out, y, c, res, rbk);
            HIPCHK(hipGetLastError());
            double* const outs[3] = {crps_out, error_out, spread_out};
            for (int k = 0; k < 3; ++k)
                if (outs[k]) ENS_TRY(ens_copy_planes(h, outs[k], r0, rows, res + (size_t)k * rbk, r, (size_t)od));
            return 0;
        });
}

// M = ceil(min(0.2 m, 3 sqrt(m / r_eff))), G = 30 + floor(sqrt M), q = floor(M / 4 + 1/2) (include/tbnn.h, tbnn_ensemble_loo)
static void psis_sizes(int32_t m, double r_eff, int* M, int* G, int* q) {
    *M = (int)std::ceil(std::min(0.2 * (double)m, 3.0 * std::sqrt((double)m / r_eff)));
    *G = 30 + (int)std::floor(std::sqrt((double)*M));
    *q = (int)std::floor((double)*M / 4.0 + 0.5);
}
// what tbnn_ensemble_loo keeps per row beside the predictions: the matrix column (m doubles) and the tail's two planes (2 M doubles)
static size_t psis_row_bytes(int32_t m, int M) { return sizeof(double) * ((size_t)m + 2 * (size_t)M); }

extern "C" int tbnn_ensemble_loo(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int likelihood, const float* sd,
                                 int which, const float* X, const float* Y, int64_t n, double r_eff, double* elpd_loo_rows,
                                 double* pareto_k_rows, double* lppd_rows, double* p_waic_rows, double* pointwise) {
    NEED(h);
    const std::string who = "ensemble_loo";
    const int d_out = h->nd.d_out;
    if (!elpd_loo_rows && !pareto_k_rows && !lppd_rows && !p_waic_rows && !pointwise) return fail(-1, who + ": every output is null");
    if (!(r_eff > 0.0) || !std::isfinite(r_eff)) return fail(-1, who + ": r_eff must be finite and > 0");
    ENS_TRY(ens_check_lik(who, likelihood, d_out, X, Y));
    if (m < 2) return fail(-1, who + ": fewer than 2 networks");
    int M = 0, G = 0, q = 0;
    psis_sizes(m, r_eff, &M, &G, &q);
    const size_t extra = psis_row_bytes(m, M);
    // the budget of ensemble_row_blocks, judged here before m values of sd are read
    ENS_TRY(ens_block_rows(who, 0, (size_t)m * (size_t)d_out + extra / sizeof(float), nullptr));
    ENS_TRY(ens_check_targets(h, who, which, X, Y, n));
    // per network: sigma and the constant of the density, as tbnn_ensemble_loglik's
    bool gauss = false;
    double nu = 0.0;
    std::vector<float> sig;
    std::vector<double> cst;
    ENS_TRY(ens_lik_consts(h, who, likelihood, sd, m, &gauss, sig, cst, &nu));
    const bool psis = elpd_loo_rows || pareto_k_rows;
    const double logm = std::log((double)m);
    const float* dYrows = nullptr;
    Buf<float> dSig, dY;
    Buf<double> dCst, dL, dTail, dRes;
    long rbk = 0;
    return ensemble_row_blocks(h, who, thetas, m, theta_stride, TBNN_XFORM_NONE, 1.f, 0.f, which, X, n,
        [&](long rb) -> int {
            rbk = rb;
            HIPCHK(dL.alloc((size_t)m * rb));
            if (psis) HIPCHK(dTail.alloc(2 * (size_t)M * rb));
            // a block's row results: elpd_loo, pareto_k, lppd, p_waic
            HIPCHK(dRes.alloc(4 * (size_t)rb));
            if (gauss) {
                ENS_TRY(ens_upload(h, dSig, sig.data(), (size_t)m));
                ENS_TRY(ens_upload(h, dCst, cst.data(), (size_t)m));
            }
            return ens_stage_targets(h, which, Y, n, dY, &dYrows);
        },
        [&](long r0, long r, long rows, const float* t) -> int {
            const dim3 grid(ens_grid(r)), tb(ENS_TB);
            double* res = dRes;
            hipLaunchKernelGGL(k_ens_pointwise, grid, tb, 0, h->stream, t, (int)m, r, d_out, likelihood, dYrows + (size_t)r0 * d_out,
                               gauss ? (const float*)dSig : nullptr, gauss ? (const double*)dCst : nullptr, logm, (double*)dL,
                               lppd_rows ? res + 2 * rbk : nullptr, p_waic_rows ? res + 3 * rbk : nullptr, nu);
            HIPCHK(hipGetLastError());
            if (psis) {
                hipLaunchKernelGGL(k_ens_psis, grid, tb, 0, h->stream, (const double*)dL, (int)m, r, M, G, q, (double*)dTail, dTail + (size_t)M * rbk,
                                   elpd_loo_rows ? res : nullptr, pareto_k_rows ? res + rbk : nullptr);
                HIPCHK(hipGetLastError());
            }
            double* const outs[4] = {elpd_loo_rows, pareto_k_rows, lppd_rows, p_waic_rows};
            for (int k = 0; k < 4; ++k)
                if (outs[k]) HIPCHK(hipMemcpyAsync(outs[k] + r0, res + (size_t)k * rbk, (size_t)r * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            // l[m][r] -> pointwise[m][rows] at column r0
            if (pointwise) ENS_TRY(ens_copy_planes(h, pointwise, r0, rows, dL, r, (size_t)m));
            return 0;
        }, extra);
}
