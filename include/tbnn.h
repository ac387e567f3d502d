/*
 * tbnn.h -- C ABI of the MI355X-native HMC sampler for dense Bayesian neural
 * networks (drop-in for the HMC hot path of alpha-davidson/TensorBNN).
 *
 * The reference has no FFI boundary of its own: its hot path is Python calling
 * TensorFlow-Probability.  Each entry point below
 * names the reference interface (file:line under /root/reference) it replaces.
 * A reference maintainer binds these with ctypes; the stub is shown in
 * INTEGRATION.md and shipped as tensorbnn_amd/_native.py.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success, <0 on error
 *     (message via tbnn_last_error(), thread-local).
 *   - caller owns all host buffers, the library owns all device buffers.
 *   - one handle = one chain = one HIP device + one HIP stream.  A handle is
 *     not thread-safe; distinct handles are.
 *   - every call returns after its stream work has completed.
 *   - there is NO CPU fallback: tbnn_create fails when no gfx950 device is
 *     visible.  tbnn_adapter_* is host-only C++ (the reference's adapter is
 *     host-side TF-eager code as well) and works without a GPU.
 *
 * State-vector contract:
 *   theta = concat over dense layers of ( W row-major [out,in], b [out] )
 *   eta   = concat over dense layers of ( loc_w, g_w, loc_b, g_b ), then
 *           sqrt(sd) when the likelihood is TBNN_LIK_GAUSSIAN.
 */
#ifndef TBNN_H
#define TBNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TBNN_MAX_LAYERS 16
#define TBNN_ABI_VERSION 3   /* 3: tbnn_lint_status, tbnn_last_transition_path; 2: tbnn_hmc_step_each / _run_each / tbnn_hyper_step_each, tbnn_debug_fused_burst, multi-chain handles (tbnn_create_multi: buffers of set/get_state, hmc_step/run, hyper_step are [chains][...]), tbnn_build_id, tbnn_comm_count, tbnn_hyper_probs_many, tbnn_debug_momentum */

/* activation layer that follows a dense layer
 * (tensorBNN/activationFunctions.py:27-63) */
enum { TBNN_ACT_NONE = 0, TBNN_ACT_RELU = 1, TBNN_ACT_TANH = 2, TBNN_ACT_SIGMOID = 3,
       TBNN_ACT_EXP = 4 /* activationFunctions.py:14-24 */, TBNN_ACT_ELU = 5 /* :66-76 */ };
/* prior family of a dense layer: CauchyDenseLayer (= DenseLayer) layer.py:101,
 * GaussianDenseLayer layer.py:282 */
enum { TBNN_PRIOR_CAUCHY = 0, TBNN_PRIOR_GAUSSIAN = 1 };
/* likelihood.py:63 (Gaussian), :136 (FixedGaussian), :205 (Bernoulli); CATEGORICAL: a softmax over each row's d_out >= 2 outputs
 * (logits: the last layer carries no activation), Y one-hot or probability rows: sum_rows sum_k y_k log softmax_k(f);
 * POISSON: counts, any d_out >= 1 independent outputs, the last layer without an activation and its output f the LOG of the rate:
 * log p(y | f) = y f - exp(f) - lgamma(y + 1) per (row, output), dL/df = y - exp(f).  Y finite and >= 0 (non-integers allowed):
 * tbnn_set_data[_device] refuses anything else.  No likelihood hyper.  The constant C = sum_i w_i sum_k lgamma(y_ik + 1) is computed
 * once when the data (or row weights) are staged, in fp64 and bit for bit the same from run to run; the kernels accumulate y f - exp(f)
 * and C is subtracted where the log-probability is formed.  After tbnn_set_data_device C does not follow later in-place changes of the
 * caller's Y (stage the data again).  A log-rate beyond the fp32 range of exp gives a non-finite log-probability: such a proposal is
 * rejected (log_accept_ratio -inf) and the chain keeps its state.  Code 4 is not assigned: it is refused as an unknown likelihood, as
 * before TBNN_LIK_POISSON existed;
 * STUDENT_T: robust regression, any d_out >= 1 independent outputs, the last layer with any activation the Gaussian kinds accept.  With
 * the scale s = the descriptor's fixed_sd (> 0), the degrees of freedom nu = the descriptor's lik_df (finite, > 0) and r = y - f, per
 * (row, output):  log p = lgamma((nu+1)/2) - lgamma(nu/2) - 1/2 log(nu pi) - log s - (nu+1)/2 log1p(r^2 / (nu s^2)),
 * dL/df = (nu+1) r / (nu s^2 + r^2): a row's pull is bounded (largest at |r| = s sqrt nu) and falls off as 1/r beyond.  No likelihood
 * hyper (H = 4 n_layers; the hyper transition touches no data).  The kernels accumulate sum_i w_i log1p(r^2 / (nu s^2)) (stat of
 * tbnn_logp_grad) and the constant, W d_out times the first four terms with W the rows that normalise the Gaussian kinds too (their
 * count, the sum of the row weights, n_total of a row-sharded chain), is added in fp64 where the log-probability is formed.  Codes 4, 6,
 * 7 and every other value are not assigned: refused as an unknown likelihood.  Under TBNN_LIK_STUDENT_T tbnn_create,
 * tbnn_create_multi and tbnn_fused_kernel_available refuse a lik_df that is not finite and > 0 and a fixed_sd that is not > 0;
 * NEG_BINOMIAL: over-dispersed counts, any d_out >= 1 independent outputs; Poisson's admission rules (no last activation, f the LOG of the
 * mean, Y finite and >= 0, non-integers allowed, no likelihood hyper).  The dispersion r = the descriptor's lik_df (finite, > 0: tbnn_create,
 * tbnn_create_multi and tbnn_fused_kernel_available refuse any other lik_df); mean mu = exp(f), variance mu + mu^2 / r, r -> inf the Poisson
 * model.  With t = f - log r, p = sigmoid(t) = mu / (r + mu), q = 1 - p, per (row, output):
 * log p(y | f) = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y log p + r log q,  dL/df = y q - r p = r (y - mu) / (r + mu): a row's pull is
 * bounded by r from below, however large the rate.  The kernels form -log p = max(-t, 0) + log1p(e^-|t|) and -log q = max(t, 0) +
 * log1p(e^-|t|) and never exp(f): every finite f gives a finite term (Poisson's overflow past the fp32 range of exp does not occur).  They
 * accumulate y log p + r log q; the constant C = sum_i w_i sum_k (lgamma(y + 1) + lgamma(r) - lgamma(y + r)) is computed with the data (or
 * row weights), in fp64 and bit for bit the same from run to run, and subtracted where the log-probability is formed -- Poisson's rules for
 * tbnn_set_data_device and row shards hold.  Code 9 and every other value are not assigned;
 * HETERO_GAUSSIAN: regression whose noise scale the network predicts.  The network has EXACTLY 2 outputs and no activation after the last
 * layer (anything else is refused by tbnn_create, tbnn_create_multi and tbnn_fused_kernel_available): output 0 is the mean f, output 1 is
 * g = log s, and y ~ N(f, exp(g)^2).  Per ROW, with G = log(1e8) (the clip the Gaussian kinds apply to their sd), gc = min(max(g, -G), G),
 * u = exp(-2 gc) and r = y - f:  log p(y | f, g) = -1/2 log(2 pi) - gc - 1/2 r^2 u,  dL/df = r u,  dL/dg = r^2 u - 1 for -G <= g <= G,
 * else 0 (the derivative of the clipped function, as the Bernoulli clip's zero gradient outside its range).  No likelihood hyper
 * (H = 4 n_layers; the hyper transition touches no data); fixed_sd and lik_df are not read.  A row weight scales the row's term and both
 * deltas.  The kernels accumulate sum_i w_i (-gc - 1/2 r^2 u); the constant -1/2 log(2 pi) W, W the rows that normalise the Gaussian kinds
 * (their count, the sum of the row weights, n_total of a row-sharded chain), is added in fp64 where the log-probability is formed, and stat
 * of tbnn_logp_grad is the data term INCLUDING it, as under Poisson.  Targets stay [n][d_out] = [n][2] at this interface: column 0 is y,
 * column 1 is NOT READ.  A non-finite statistic rejects the proposal.  tbnn_metrics compares output 0 with target column 0 only;
 * GAMMA: positive, continuous, right-skewed targets (durations, amounts, concentrations), any d_out >= 1 independent outputs, no
 * activation after the last layer: its output f is the LOG of the mean, mu = exp(f).  The shape a = the descriptor's lik_df, finite and
 * > 0 (tbnn_create, tbnn_create_multi and tbnn_fused_kernel_available refuse any other lik_df); variance mu^2 / a, a constant coefficient
 * of variation 1 / sqrt(a); a = 1 is the exponential distribution.  fixed_sd is not read.  No likelihood hyper (H = 4 n_layers).  Targets
 * are finite, strictly > 0 and at most 2^100 (1.2676506e30): staging refuses anything else, zero too (log y enters the constant).  The
 * ceiling: where exp(-f) leaves fp32's normal range (f > 87.3) the hardware exp returns 0 and an element loses y exp(-f) < y 2^-126, below
 * 2^-26 of the 1 it is subtracted from for every admitted target.  fp32-denormal targets are admitted: the kernels' products and the
 * constant keep them (tests/test_gpu_likelihood_edges.py test_denormal_targets).  Per (row, output):
 * log p(y | f) = a log a - lgamma(a) + (a - 1) log y - a f - a y exp(-f),  dL/df = a (y exp(-f) - 1).  The kernels accumulate
 * stat = sum_i w_i (f + y e^-f) with one hardware exp per element and return the delta w a (y e^-f - 1); the constant
 * C = sum_i w_i sum_k (lgamma(a) - a log a - (a - 1) log y_ik) is computed with the data (or row weights), in fp64 and bit for bit the same
 * from run to run, and the log-probability is formed as -a stat - C -- Poisson's rules for tbnn_set_data_device, validation data and row
 * shards hold, and stat of tbnn_logp_grad is the data term -a stat - C itself.  A log-mean below the fp32 range of exp(-f) gives a
 * non-finite statistic: the proposal is rejected and the chain keeps its state (Poisson's rule, on the other side);
 * WEIBULL: times to an event, some rows RIGHT-CENSORED (survival data: time to failure, relapse, churn), any d_out >= 1 independent
 * outputs, no activation after the last layer: its output f is the LOG of the Weibull scale, lambda = exp(f) (the accelerated-failure-time
 * parameterisation).  The shape k = the descriptor's lik_df, finite and > 0 (tbnn_create, tbnn_create_multi and
 * tbnn_fused_kernel_available refuse any other lik_df); k = 1 is the exponential model.  fixed_sd is not read.  No likelihood hyper
 * (H = 4 n_layers).  CENSORING TRAVELS IN THE SIGN OF THE TARGET: y > 0 is an event observed at time y, y < 0 a row right-censored at
 * time |y| (the event had not happened by then); times are positive, so the sign is free, and target layout, staging, row shards and row
 * weights keep their shape.  With d = 1 for an event and 0 for a censored row, t = |y| and u = (t e^-f)^k = exp(k (log t - f)), per
 * (row, output):   event  log p = log k + (k - 1) log t - k f - u;   censored  log S = -u;   dL/df = k (u - d).
 * A row weight scales the row's term and its delta.  Targets are admitted when they are finite, nonzero and 2^-100 <= |y| <= 2^100 (the
 * floor hands the hardware log a normal fp32 number, the ceiling is Gamma's): staging refuses anything else and names the rule, and the
 * handle keeps the rows it had.  The kernels accumulate stat = sum_i w_i (k d f + u), one fp32 term per element from one hardware log and
 * one hardware exp, and return the delta w k (u - d); the constant C = -sum_i w_i sum_out d (log k + (k - 1) log t) is computed with the
 * data (or row weights), in fp64 and bit for bit the same from run to run, and the log-probability is formed as -stat - C -- Gamma's rules
 * for tbnn_set_data_device, validation data and row shards hold, and stat of tbnn_logp_grad is the data term -stat - C itself.  If u
 * overflows fp32 the statistic is not finite: the proposal is rejected and the chain keeps its state (Poisson's and Gamma's rule).
 * tbnn_metrics reads the target as staged, sign included.  Left and interval censoring, and a sampled or predicted shape, are not built.
 * Codes 4, 6, 7, 9, 11, 13, 15 and every other value are not assigned. */
enum { TBNN_LIK_GAUSSIAN = 0, TBNN_LIK_FIXED_GAUSSIAN = 1, TBNN_LIK_BERNOULLI = 2, TBNN_LIK_CATEGORICAL = 3, TBNN_LIK_POISSON = 5,
       TBNN_LIK_STUDENT_T = 8, TBNN_LIK_NEG_BINOMIAL = 10, TBNN_LIK_HETERO_GAUSSIAN = 12, TBNN_LIK_GAMMA = 14, TBNN_LIK_WEIBULL = 16 };

/* kernel selection for the forward+backward pass.  AUTO: a fused shape-specialised MFMA kernel where one covers the network
 * (built in or registered at run time), else the layered run-time-shape MFMA kernels (any architecture); FAST: a fused kernel or
 * an error; GENERIC: the thread-per-row kernel (on-device cross-check) */
enum { TBNN_KERNEL_AUTO = 0, TBNN_KERNEL_GENERIC = 1, TBNN_KERNEL_FAST = 2 };

typedef struct tbnn_layer_desc {
    int32_t in_dim;   /* layer.py:110 inputDims  */
    int32_t out_dim;  /* layer.py:111 outputDims */
    int32_t act;      /* TBNN_ACT_*   */
    int32_t prior;    /* TBNN_PRIOR_* */
} tbnn_layer_desc;

typedef struct tbnn_net_desc {
    int32_t n_layers;
    const tbnn_layer_desc* layers;
    int32_t likelihood;  /* TBNN_LIK_* */
    float fixed_sd;      /* FixedGaussianLikelihood(sd=) likelihood.py:138-141; the scale s of TBNN_LIK_STUDENT_T */
    int32_t kernel;      /* TBNN_KERNEL_* */
    float lik_df;        /* TBNN_LIK_STUDENT_T: the degrees of freedom nu; TBNN_LIK_NEG_BINOMIAL: the dispersion r; TBNN_LIK_GAMMA: the shape a; TBNN_LIK_WEIBULL: the shape k; ignored under every other likelihood (this was `int32_t reserved`:
                          * the same size and offset, and the all-zero bits callers passed there are 0.0) */
} tbnn_net_desc;

/* per-transition results: what network.train prints/threads through
 * (network.py:410-411 acceptRate; :596-600 prints; paramAdapter.py:219-222 SJD) */
typedef struct tbnn_step_out {
    int32_t accepted;          /* Metropolis decision */
    int32_t n_leapfrog;        /* leapfrog steps executed (= L) */
    float log_accept_ratio;    /* TFP log_accept_ratio (non-finite -> -inf) */
    float accept_prob;         /* lar<0 ? exp(lar) : 1   network.py:410-411 */
    double logp_old;           /* target log-prob at the start state (the true log-density: Poisson includes its constant C) */
    double logp_new;           /* target log-prob at the proposal */
    double kinetic_old;        /* 1/2 |p0|^2 */
    double kinetic_new;        /* 1/2 |p_L|^2 */
    double sjd;                /* sum (new-old)^2 over theta (0 when rejected) */
    float device_us;           /* hipEvent time of the whole transition */
    float fwdbwd_us;           /* mean hipEvent duration of the profiled fused fwd+bwd launches (0: profiling off) */
} tbnn_step_out;

typedef struct tbnn_ctx* tbnn_handle;

const char* tbnn_last_error(void);
int tbnn_abi_version(void);
/* hash of the sources (kernel headers, translation units, this header, compiler flags) the loaded library was built from;
 * profiles/rocprof_kernel_us.json and pmc_traffic.json carry the id of the library they were measured on, and bench.py
 * quotes them only when it matches */
const char* tbnn_build_id(void);
/* what the build-time MFMA hazard check (tensorbnn_amd/hazard_lint.py, through checked_compile.py) did to each kernel unit of the loaded library:
 * "<unit>: listing checked (<n> repaired: <rule>:<count> ..); disassembly clean; ..." -- a library cannot be built without the check */
const char* tbnn_lint_status(void);
/* number of visible HIP devices (<0: error) */
int tbnn_device_count(void);

/* network.__init__/add/setupMCMC state on the device (network.py:19-58,
 * :173-191).  seed/chain_id key the Philox4x32-10 chain RNG that replaces
 * tf.random.set_seed(50) (network.py:562). */
int tbnn_create(const tbnn_net_desc* desc, int device, uint64_t seed, uint32_t chain_id,
                tbnn_handle* out);
/* Several independent chains of one network on ONE device behind one handle (round 4).  SURVEY 8(e) puts one chain on each
 * GPU; small problems -- the reference's own examples: Examples/trainRegression.py:33 has 11 rows -- leave most of a GPU idle
 * and are bound by launch latency, so the per-chain kernels of all n_chains chains run as ONE launch each (gridDim.y = chain).
 * Chain c is bit for bit the chain tbnn_create(desc, device, seed, chain_id + c) would be, at the same step size and leapfrog
 * count for all (they advance in lockstep).  On such a handle
 *   tbnn_set_state / tbnn_get_state take [n_chains][P] floats, tbnn_set_hypers / tbnn_get_hypers [n_chains][H];
 *   tbnn_hmc_run fills outs[chain][epoch], tbnn_hmc_step and tbnn_hyper_step out[chain] (no injected draws, no trace);
 *   tbnn_set_data[_device], tbnn_set_validation, tbnn_forward / tbnn_predict / tbnn_metrics with an explicit theta,
 *   tbnn_forward_many and tbnn_hyper_probs_many work as usual; everything that addresses ONE chain's state (tbnn_logp_grad,
 *   tbnn_hyper_logp_grad, theta == NULL predictions, tbnn_gather_samples, tbnn_set_row_shard) returns an error. */
int tbnn_create_multi(const tbnn_net_desc* desc, int device, uint64_t seed, uint32_t chain_id, int32_t n_chains,
                      tbnn_handle* out);
int tbnn_chain_count(tbnn_handle h);  /* 1 for tbnn_create */
int tbnn_destroy(tbnn_handle h);
int tbnn_param_count(tbnn_handle h);  /* P */
int tbnn_hyper_count(tbnn_handle h);  /* H */
/* name of the kernel variant in use ("fast3<...>", "mid<...>", "wide<...>", "layered<...>", "generic") */
const char* tbnn_kernel_name(tbnn_handle h);
/* which kernels ran the leapfrog steps of the LAST transition: "per-step" (a fused pass + k_update per step) or "trajectory" (small narrow
 * problems: the L steps in one launch, kernels_traj.hpp); "none" before the first.  The choice does not depend on tbnn_set_profiling; a traced
 * transition (trace_logp) always takes the per-step kernels, whose sums run in another order: not bit-equal to the untraced one. */
const char* tbnn_last_transition_path(tbnn_handle h);

/* trainX / trainY staging, network.py:41-45.  X [n,d_in] row-major, Y [n,d_out]. */
int tbnn_set_data(tbnn_handle h, const float* X, const float* Y, int64_t n);
/* same, from device pointers (e.g. a torch tensor's data_ptr on this device) */
int tbnn_set_data_device(tbnn_handle h, const float* dX, const float* dY, int64_t n);
/* Per-row likelihood weights: w[n] (host), n == the staged rows; every row's data term and its output-layer delta are scaled by w_i, and
 * the Gaussian normaliser counts W = sum_i w_i (fp64) rows instead of n.  Priors are not weighted.  Weights must be finite and >= 0 with
 * at least one > 0.  w == NULL clears them; tbnn_set_data[_device] clears them too (new rows).  All chains of a multi-chain handle share
 * them.  Setting / clearing re-selects the kernels: a registered weighted library of the shape (tbnn_kernel_name shows ",weighted"),
 * else the layered family (the generic kernel under TBNN_KERNEL_GENERIC).  Weighted transitions always take the per-step kernels
 * (tbnn_last_transition_path: "per-step").  Refused: negative / non-finite / all-zero weights, n not matching, a row-sharded handle
 * (tbnn_set_row_shard, in either order: a weighted shard would need the weight sum of all ranks).  A refused call leaves the handle as
 * it was (its kernels and its previous weights, if any).  The weights are staged together with a COPY of the targets: after
 * tbnn_set_data_device, a weighted handle does not see later in-place changes of the caller's Y (an unweighted one reads Y live, and
 * both read X live) -- call tbnn_set_row_weights again after changing Y.  tbnn_metrics is not weighted.  Under TBNN_LIK_POISSON setting and
 * clearing also recompute the constant C with the new weights (a row of weight 0 adds nothing to it); there even an UNWEIGHTED handle
 * staged from device pointers keeps the C of the Y it was staged with. */
int tbnn_set_row_weights(tbnn_handle h, const float* w, int64_t n);

/* network.states / network.hyperStates, network.py:53-56 */
int tbnn_set_state(tbnn_handle h, const float* theta);
int tbnn_get_state(tbnn_handle h, float* theta);
int tbnn_set_hypers(tbnn_handle h, const float* eta);
int tbnn_get_hypers(tbnn_handle h, float* eta);

/* the target closure calculateProbs (network.py:370-392) and its gradient
 * (TF autodiff inside TFP).  theta/eta may be NULL = use the
 * handle's current state.  stat (optional) receives the data-term statistic:
 * sum((y-f)^2) for the Gaussian likelihoods, the log-likelihood for Bernoulli, categorical and Poisson (logp and stat are the true
 * log-density there: Poisson's include the constant -C, TBNN_LIK_POISSON above). */
int tbnn_logp_grad(tbnn_handle h, const float* theta, const float* eta, double* logp,
                   float* grad, double* stat);

/* network.predict, network.py:141-171: out is [d_out, n] like the reference. */
int tbnn_forward(tbnn_handle h, const float* theta, const float* X, int64_t n, float* out);

/* One weight transition = InnerStepMain (network.py:368-412):
 * tfp.mcmc.HamiltonianMonteCarlo + sample_chain(num_results=1), call sites
 * network.py:394-408.  p0 (P floats) / log_u (1 float) may be NULL (device
 * Philox draw) or injected for parity tests.  trace_logp (optional, L+1
 * doubles) receives the target log-prob at q_0..q_L. */
int tbnn_hmc_step(tbnn_handle h, float eps, int32_t L, const float* p0, const float* log_u,
                  tbnn_step_out* out, double* trace_logp);

/* n_epochs transitions back to back with fixed (eps, L) and no host
 * round-trip in between (adapter bypassed).  outs: n_epochs records. */
int tbnn_hmc_run(tbnn_handle h, float eps, int32_t L, int32_t n_epochs, tbnn_step_out* outs);

/* Multi-chain handles with EVERY chain at its own step size and leapfrog count -- the reference runs one paramAdapter per chain
 * (network.py:221-235, :603-607), so C chains of it are C schedules.  eps, L: n_chains values.  The chains advance in lockstep for
 * max_c L[c] steps; chain c takes its closing half kick at step L[c] and is skipped from then on (its blocks of the fused pass exit
 * at once), so chain c is bit for bit tbnn_create(.., chain_id + c) driven with (eps[c], L[c]).  out[c].n_leapfrog = L[c].
 * tbnn_hmc_run_each: n_epochs such transitions back to back, outs[chain][epoch].  (On a one-chain handle: arrays of one.) */
int tbnn_hmc_step_each(tbnn_handle h, const float* eps, const int32_t* L, tbnn_step_out* out);
int tbnn_hmc_run_each(tbnn_handle h, const float* eps, const int32_t* L, int32_t n_epochs, tbnn_step_out* outs);
/* the hyper transition of every chain at its own step size eps_h[c] (one dual averaging per chain, network.py:457-469) */
int tbnn_hyper_step_each(tbnn_handle h, const float* eps_h, int32_t L_h, tbnn_step_out* out);

/* One hyper-parameter transition = the HMC part of InnerStepHyper
 * (network.py:414-456); dual averaging (:457-469) stays with the caller. */
int tbnn_hyper_step(tbnn_handle h, float eps_h, int32_t L_h, const float* p0, const float* log_u,
                    tbnn_step_out* out);
/* the hyper target (network.py:416-440) and its gradient w.r.t. eta */
int tbnn_hyper_logp_grad(tbnn_handle h, const float* eta, double* logp, float* grad);

/* checkpoint export: writes theta (P floats) then eta (H floats) to a device
 * buffer of P+H floats (feeds the RCCL all-gather at sample time). */
int tbnn_export_sample_device(tbnn_handle h, float* d_out);

/* the chain RNG, exposed for tests: n standard normals / one log-uniform for
 * (epoch, purpose) exactly as tbnn_hmc_step would draw them. */
int tbnn_debug_draw(tbnn_handle h, uint32_t epoch, uint32_t purpose, int32_t n, float* out_normals,
                    float* out_log_u);
/* diagnostic (tests/test_gpu_properties.py): the momentum the last trajectory of tbnn_hmc_step ended with (P floats: p_L after the
 * closing half kick, kept whether or not the proposal was accepted).  With it a test can run the integrator backwards: from q_L
 * with p0 = -p_L the same L steps must return to q_0 (tfp's leapfrog is time-reversible; call sites network.py:394-408). */
int tbnn_debug_momentum(tbnn_handle h, float* p_out);
/* diagnostic (tests/test_gpu_many_tiles.py): how many statistic partials a fused pass of the staged rows writes and tbnn_logp_grad sums --
 * on the one-kernel families the workgroups of the launch (with the test hook TBNN_FAST_GRID: the small grid); 0 before tbnn_set_data.
 * Read only. */
int tbnn_debug_stat_partials(tbnn_handle h);
/* epoch counter that keys the RNG (incremented by every tbnn_hmc_step) */
int tbnn_set_epoch(tbnn_handle h, uint32_t epoch);
/* record a hipEvent pair around every stride-th fused fwd+bwd launch on the
 * chain's stream (fills fwdbwd_us); stride <= 0 turns it off */
int tbnn_set_profiling(tbnn_handle h, int stride);
/* diagnostic (tools/stamps.py): launches the narrow fused kernel three times at the current state and returns the
 * in-kernel stamps of workgroup 0 of the last launch: out16[0..7] = 100 MHz wall clock at start, prologue done, first
 * tile done, tile loop done, end, cooperative tail done, staging done, tile slabs done; out16[8..15] = the shader clock at
 * the same points.  Narrow ahead-of-time kernels only; the chain state is not touched. */
int tbnn_debug_stamps(tbnn_handle h, uint64_t* out16);
/* measurement (bench.py's roofline): `reps` fused forward+backward passes of the CURRENT state back to back on the chain's stream between ONE
 * pair of events; *us_per_pass = elapsed / reps.  (An event pair around a single launch, tbnn_set_profiling, carries ~3 us of the pair's own
 * cost: 45.4 us where rocprofv3 sees 42.6 at configs[1].)  The chain state is not touched.  Reference: the gradient evaluation of one leapfrog
 * step, network.py:394-408. */
int tbnn_debug_fused_burst(tbnn_handle h, int32_t reps, float* us_per_pass);

/* ---- predictions and metrics over the staged rows: no host traffic but the result.
 * network.__init__ stages the validation set next to the training set (network.py:47-51). ---- */
int tbnn_set_validation(tbnn_handle h, const float* X, const float* Y, int64_t n);
/* network.predict(train=True/False) (network.py:141-171): which = 0 training rows, 1 validation rows;
 * theta NULL = current state; out: host [d_out, n] or NULL (predictions stay on the device). */
int tbnn_predict(tbnn_handle h, int which, const float* theta, float* out);
/* Ensemble prediction, predictor.predict (predictor.py:132-155): the forward pass of m saved
 * networks, theta_i = thetas + i * theta_stride (theta_stride >= P floats), over the same rows.  X NULL: the staged
 * rows selected by `which` (0 training, 1 validation); else n host rows [n, d_in].  out: host [m][d_out][n].
 * Narrow shapes run one batched launch of the forward-only MFMA kernel (grid.y = network). */
int tbnn_forward_many(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int which, const float* X,
                      int64_t n, float* out);
/* ---- reductions over the network axis of an ensemble, on the device chunk tbnn_forward_many holds: the forward passes are the very
 * kernels of tbnn_forward_many (every kernel family, one-chain and multi-chain handles); no host traffic but the result.  Arguments up
 * to `n` as tbnn_forward_many's.  net_w: m importance weights (predictor.reweight) or NULL = equal; finite and >= 0 with at least one
 * > 0, refused otherwise (the rules of tbnn_set_row_weights).  Row weights (tbnn_set_row_weights) do not enter, as in tbnn_metrics. ---- */
enum { TBNN_XFORM_NONE = 0, TBNN_XFORM_EXP = 1, TBNN_XFORM_SIGMOID = 2, TBNN_XFORM_SOFTMAX = 3 };
/* Posterior-predictive moments.  Per (output, row): t_i = xform(f_i) * scale + shift in fp32 (the de-normalisation of tbnn_metrics;
 * SOFTMAX: across the row's d_out >= 2 outputs, the row maximum subtracted first); with W = sum_i w_i
 *   mean = sum_i w_i t_i / W,  var = sum_i w_i (t_i - mean)^2 / W   (population form: np.average with weights, np.var)
 * summed in fp64 in network order.  mean_out, var_out: host [d_out][n] doubles; var_out may be NULL. */
int tbnn_ensemble_moments(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, const float* net_w, int xform,
                          float scale, float shift, int which, const float* X, int64_t n, double* mean_out, double* var_out);
/* Data log-likelihood of the rows under each of the m networks, reduced both ways.  likelihood: the TBNN_LIK_* to judge under,
 * independent of the handle's own; sd: m per-network standard deviations for the Gaussian kinds, or NULL = the descriptor's fixed_sd
 * (clipped to [1e-8, 1e8], layer.py:60-64).  Y: host targets [n, d_out] of the rows; NULL with X NULL = the staged targets of `which`
 * (Y with X NULL: targets for the staged rows, n must match); X without Y is refused.  Terms: the Gaussian log density per output;
 * Bernoulli with p clipped to [1e-8, 1 - 1e-7] (likelihood.py:78-80); categorical sum_k y_k log softmax_k(f) (likelihood.py:86-107);
 * Poisson y f - exp(f) - lgamma(y + 1) per output in fp64, f the log-rate (the posterior mean and variance of the rate itself:
 * tbnn_ensemble_moments with TBNN_XFORM_EXP); Student-t: the density of TBNN_LIK_STUDENT_T per output in fp64, its scale s_i = sd[i] or
 * NULL = fixed_sd, clipped as the Gaussian kinds', its nu the handle's lik_df -- the descriptor's on a Student-t handle, what
 * tbnn_set_lik_df set on any other (0, never set: refused); negative binomial: the density of TBNN_LIK_NEG_BINOMIAL per output in fp64 in
 * its stable form, its dispersion r the handle's lik_df by the same rule; Gamma: the density of TBNN_LIK_GAMMA per output in fp64, its
 * shape a the handle's lik_df by the same rule; Weibull: per output the log density of TBNN_LIK_WEIBULL on an event row (y > 0) and the log
 * survival function -u on a right-censored one (y < 0), in fp64, its shape k the handle's lik_df by the same rule.
 *   per_net[i]   = sum over rows and outputs of the terms under network i          (m doubles, or NULL)
 *   lppd_rows[r] = log sum_i w_i p(y_r | theta_i) - log W, p the product over the row's outputs   (n doubles, or NULL)
 * Both are the same bits from run to run. */
int tbnn_ensemble_loglik(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int likelihood, const float* sd,
                         const float* net_w, int which, const float* X, const float* Y, int64_t n, double* per_net,
                         double* lppd_rows);
/* Classification uncertainty: how sure is the ensemble of a label, and is that sureness noise in the data or disagreement between the
 * networks?  Arguments up to `n` as tbnn_ensemble_moments'; likelihood: TBNN_LIK_BERNOULLI or TBNN_LIK_CATEGORICAL, the kind to read the
 * outputs under, independent of the handle's own (as tbnn_ensemble_loglik's).  Per network i and row r, from the fp32 forward output f:
 *   categorical  (K = d_out >= 2 logits per row)  p_ik = exp(f_k - max_j f_j) / sum_j exp(f_j - max_j f_j) in fp32, the very values
 *                tbnn_ensemble_moments forms under TBNN_XFORM_SOFTMAX; H_i = -sum_k p_ik log p_ik, the log and the sum in fp64 from the
 *                fp32 p_ik, classes in index order, 0 log 0 = 0; the vote a_i = the smallest k with p_ik maximal (ties go to the lowest
 *                class).  One entropy per row.
 *   Bernoulli    (every output a label of its own: an element is an (output, row) pair)  p_i = f clipped to [1e-8, 1 - 1e-7] in fp32,
 *                the clip of the likelihood and of tbnn_ensemble_loglik; H_i = -(p_i log p_i + (1 - p_i) log1p(-p_i)) in fp64; the vote
 *                is p_i >= 1/2.  One entropy per element.
 * With W = sum_i w_i (net_w NULL: every w_i = 1), all sums fp64 in network order, not contracted:
 *   prob_out      pbar_k = sum_i w_i p_ik / W        the posterior-mean probability (Bernoulli: of the label 1)
 *   vote_out      sum_i w_i [a_i == k] / W           the share of the posterior that votes for class k (Bernoulli: for the label 1); the
 *                                                   variation ratio is 1 - max_k of it (Bernoulli: 1 - max(vote, 1 - vote))
 *   total_out     H[pbar], the same formula in fp64  the entropy of the predictive distribution
 *   aleatoric_out sum_i w_i H_i / W                  the expected entropy under the posterior: noise in the data
 *   epistemic_out max(total - aleatoric, 0)          the mutual information of label and network ("BALD"): model disagreement.  By
 *                                                   Jensen's inequality the difference is >= 0; only rounding can take it below
 * prob_out, vote_out: host [d_out][n] doubles; total_out, aleatoric_out, epistemic_out: host [n] doubles categorical, [d_out][n] Bernoulli.
 * Any of the five may be NULL, not all.  NaN: a NaN among a row's values (Bernoulli: an element's) under ANY network, whatever its weight,
 * gives NaN in every output of that row (element); infinite logits go through the softmax as under tbnn_ensemble_moments (f - max is NaN
 * at +inf, the row NaN).  A thread owns its row or element and walks the networks in order; the sums cross the chunks of networks
 * (2^28 floats of predictions each) in one device buffer: the same bits from run to run, whatever the grid and the chunking.
 * Refused, with nothing written: every output NULL, a likelihood other than the two label kinds (regression and count kinds:
 * tbnn_ensemble_predictive and tbnn_ensemble_moments answer there), TBNN_LIK_CATEGORICAL with d_out < 2, weights breaking the rules above,
 * and what tbnn_ensemble_moments refuses of m, theta_stride, which and n. */
int tbnn_ensemble_uncertainty(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int likelihood, const float* net_w,
                              int which, const float* X, int64_t n, double* prob_out, double* vote_out, double* total_out,
                              double* aleatoric_out, double* epistemic_out);
/* Posterior-predictive quantiles (credible intervals) over the network axis.  Arguments up to `n` as tbnn_ensemble_moments'; the values
 * ranked per (output, row) are the m values t_i = xform(f_i) * scale + shift, formed in fp32 BEFORE the ranking (a negative scale or the
 * softmax need no special case).  probs: n_probs probabilities in [0, 1], 1 <= n_probs <= 64; out: host [n_probs][d_out][n] doubles.
 *   TBNN_QUANT_LINEAR        NumPy's default: h = (m - 1) p, lo = floor(h), g = h - lo; t_(lo) + g (t_(lo+1) - t_(lo)) in fp64 from the two
 *                            fp32 order statistics (g = 0: t_(lo) itself).  net_w must be NULL.
 *   TBNN_QUANT_INVERTED_CDF  the smallest value v among the networks with w_i > 0 such that sum_{i: t_i <= v} w_i >= p W, W = sum_i w_i,
 *                            both sums fp64 in network order (net_w NULL: every w_i = 1): one of the t_i, converted exactly --
 *                            np.quantile(..., method="inverted_cdf", weights=w).  p W is one rounded fp64 product.  Without weights
 *                            (W = m) that is NumPy's own index arithmetic at any p; with weights NumPy compares the partial sums
 *                            divided by W with p instead, which is the same decision wherever p W is exact (dyadic p, integer
 *                            weights) and may differ in the last bit of a tie between a partial sum and p W otherwise.
 * An element with a NaN among its t_i gives NaN at every probability; +-inf rank as numbers.  The selection is exact (no sort: bisection on
 * the order-preserving 32-bit key of an fp32 value, 32 passes over the element's m values) and the same bits from run to run.  All m
 * networks of a row are needed at once, so the ROWS are cut into blocks (multiples of 64 rows whose m d_out rb predictions fit 2^28 floats;
 * a block's n_probs d_out rb results are held beside them).
 * Refused, with nothing written: NULL probs / out, n_probs outside 1 .. 64, a probability outside [0, 1] or NaN, an unknown method or
 * transform, SOFTMAX with d_out < 2, weights breaking the rules above, weights with TBNN_QUANT_LINEAR, m d_out 64 > 2^28. */
enum { TBNN_QUANT_LINEAR = 0, TBNN_QUANT_INVERTED_CDF = 1 };
int tbnn_ensemble_quantiles(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, const float* net_w, int method,
                            int xform, float scale, float shift, int which, const float* X, int64_t n, const double* probs,
                            int32_t n_probs, double* out);
/* Convergence diagnostics over the network axis read as chains x draws: split-R-hat (Gelman-Rubin on split chains) and the effective
 * sample size by Geyer's initial monotone sequence, the estimators Stan and ArviZ report (BDA3 section 11.4-11.5; Stan's ESS without its
 * last-odd-lag correction).  Arguments as tbnn_ensemble_quantiles' without weights and probabilities; n_chains = C, 1 <= C <= 64, m = C S
 * networks in chain-major order (network i = c S + s), S >= 8.  Per (output, row) the m values t[c][s] = xform(f) * scale + shift are formed
 * in fp32 as the quantiles form them; everything below is fp64.
 *   split     N = floor(S / 2); chain c gives split chains 2 c (draws 0 .. N-1) and 2 c + 1 (draws S-N .. S-1; an odd S drops the middle
 *             draw): K = 2 C split chains x[k][0 .. N-1]
 *   means     mu_k = mean of x[k], d[k][s] = x[k][s] - mu_k
 *   autocov   a_k(l) = (1/N) sum_{s=0}^{N-1-l} d[k][s] d[k][s+l]  (biased; summed in s order; centred products, not raw second moments);
 *             A(l) = mean over k of a_k(l), in k order
 *   variances Wv = A(0) N / (N-1);  Bn = sample variance (ddof 1) of the K means;  Vp = Wv (N-1) / N + Bn
 *   rhat      sqrt(Vp / Wv)
 *   rho(l)    1 - (Wv - A(l)) / Vp, rho(0) = 1
 *   ess       P_0 = 1 + rho(1); for k = 1, 2, ... while 2k+1 <= N-1: P_k = rho(2k) + rho(2k+1), stopping at the first P_k that is not > 0
 *             (not used), else P'_k = min(P'_{k-1}, P_k);  tau = max(-1 + 2 sum P'_k, 1 / log10(K N));  ess = K N / tau
 * An element with a NaN among its t, or with Wv not > 0 (every split chain constant), gives rhat = ess = NaN; +-inf among the t reach NaN
 * through the arithmetic.  The same bits from run to run.  The autocovariances are computed 8 lags at a time from one read of the chain, and
 * an element leaves the lag loop after the batch that holds its stop; the rows are cut into blocks as for the quantiles (the K means per
 * element, 2 C d_out rb doubles, are held beside a block).  There is no importance-weight argument: the autocorrelation of a reweighted
 * ensemble is not defined here.  rhat_out, ess_out: host [d_out][n] doubles; either may be NULL, not both (rhat alone stops after lag 0).
 * Refused, with nothing written: both outputs NULL, n_chains outside 1 .. 64, m not divisible by n_chains, m / n_chains < 8, an unknown
 * transform, SOFTMAX with d_out < 2, m d_out 64 > 2^28. */
int tbnn_ensemble_diagnostics(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int32_t n_chains, int xform,
                              float scale, float shift, int which, const float* X, int64_t n, double* rhat_out, double* ess_out);
/* The same estimator over a caller's series, host [m][tot] floats in the same chain-major order (weights, hypers, any scalar per draw):
 * rhat_out, ess_out host [tot] doubles, either may be NULL, not both.  No forward pass; nothing staged on the handle is read.  The columns
 * are uploaded in blocks under the same budget.  Refused as above, and a NULL series, tot < 1 or m 64 > 2^28. */
int tbnn_series_diagnostics(tbnn_handle h, const float* series, int32_t m, int64_t tot, int32_t n_chains, double* rhat_out,
                            double* ess_out);
/* Posterior-predictive distribution of a NEW observation: the mixture over the networks of the observation model around each network's
 * prediction -- what tbnn_ensemble_quantiles leaves out (it ranks the networks' outputs: credible intervals).  Its quantiles are predictive
 * intervals, its CDF at an observed target is the PIT value that checks them against held-out data.  Arguments up to `n` as
 * tbnn_ensemble_loglik's (likelihood, sd, net_w, rows, targets), probs and the [n_probs][d_out][n] layout as tbnn_ensemble_quantiles'.
 * Per (output j, row r), over the m networks with weights w_i (NULL: 1), W = sum_i w_i; f_i is the fp32 forward output promoted exactly to
 * fp64 and everything below is fp64; no transform is applied.
 *   Gaussian kinds   s_i = sd[i], or NULL = the descriptor's fixed_sd, clipped to [1e-8, 1e8] as tbnn_ensemble_loglik clips it.
 *                    F(y) = (1/W) sum_i w_i Phi((y - f_i) / s_i), Phi(z) = erfc(-z / sqrt 2) / 2, summed in network order (the host stages
 *                    w_i / W and 1 / (s_i sqrt 2) once per call).  Quantile at p: a point q where F crosses p -- the device returns the upper
 *                    end b of a bracket a < b at most 2 ulp64 wide with F(a) < p <= F(b) AS EVALUATED (or a point with F == p), so q is a
 *                    crossing within the evaluation error of F whatever the slope there, also where the mixture is flat between separated
 *                    modes.  Found from the bracket [min_i, max_i] of f_i + s_i Phi^-1(p) (Phi^-1 on the host: Wichura's AS 241), widened,
 *                    verified on the device and pushed outward where F does not straddle p, by Newton steps (F' is the mixture density)
 *                    that fall back to bisection whenever a step leaves the bracket or fails to shrink it.
 *   TBNN_LIK_POISSON lambda_i = exp((double)f_i).  For an integer k >= 0, F(k) = (1/W) sum_i w_i Q(k + 1, lambda_i), Q the regularised upper
 *                    incomplete gamma function (k + 1 < 2^16: series below lambda < k + 2, continued fraction above, the prefactor formed
 *                    around the peak from k + 1 = 32 on so that it does not cancel; from 2^16 on Temme's uniform expansion); F(k) = 0 for k < 0.  Quantile at p: the smallest
 *                    integer k >= 0 with F(k) >= p, as a double (searched outward from the weighted mean rate, then by bisection).  The CDF
 *                    at a target y is taken at floor(y).  One evaluation of Q costs a few sqrt(k) terms near k = lambda, 2,660 at the most
 *                    (k just below 2^16), and no loop beyond: the cost does not grow with the rate up to the ceiling of 2^30.
 *   TBNN_LIK_NEG_BINOMIAL   r = the handle's dispersion (the descriptor's lik_df on a negative-binomial handle, else what tbnn_set_lik_df set;
 *                    never set: refused), q_i = r / (r + exp(f_i)) = sigmoid(log r - (double)f_i), formed directly and not as 1 - p_i.  For an
 *                    integer k >= 0, F(k) = (1/W) sum_i w_i I_{q_i}(r, k + 1), I the regularised incomplete beta function: its continued
 *                    fraction by the modified Lentz recurrence, the side I_x(a, b) / 1 - I_{1-x}(b, a) by x < (a + 1) / (a + b + 2), the
 *                    prefactor formed around the peak (Stirling's series for every argument from 16 on) so that it does not cancel for large
 *                    k, never more than 10 sqrt(max(r, k + 1)) + 100 double steps; F(k) = 0 for k < 0.  Quantile at p: the smallest integer
 *                    k >= 0 with F(k) >= p, searched as Poisson's from the weighted mean rate, the first step floor(sqrt(mean + mean^2 / r))
 *                    + 1.  The CDF at a target y is taken at floor(y).  Ceilings: 2^20 on the rate exp(f_i) and on k (below).
 *   TBNN_LIK_GAMMA   a = the handle's shape (the descriptor's lik_df on a Gamma handle, else what tbnn_set_lik_df set; never set: refused).
 *                    F(y) = (1/W) sum_i w_i P(a, a y exp(-f_i)), P the regularised lower incomplete gamma function in fp64: for x < a + 1 its
 *                    series, returned as P (a small lower tail is not formed as 1 - (1 - P)), else 1 - Q from the continued fraction or,
 *                    from a = 2^16 on, Temme's expansion; never more than 10 sqrt(max(a, x)) + 100 terms.  F = 0 for y <= 0.  Quantile at p:
 *                    the Gaussian scheme on the positive axis -- the bracket [min_i, max_i] of the components' own quantiles
 *                    exp(f_i) g_p / a (g_p the standard Gamma(a, 1) quantile, staged by the host), widened relatively and VERIFIED with
 *                    multiplicative pushes until F(lo) < p <= F(hi) as evaluated, then Newton steps on the mixture density safeguarded by
 *                    the midpoint: the upper end hi of a bracket of at most 2 ulp64(hi) with F(lo) < p <= F(hi), or a point with F == p.
 *                    cdf_below_out is refused (a continuous CDF has no step).  A network of weight 0 is not looked at, whatever it holds.
 *   TBNN_LIK_WEIBULL k = the handle's shape (the descriptor's lik_df on a Weibull handle, else what tbnn_set_lik_df set; never set: refused).
 *                    F(t) = (1/W) sum_i w_i (-expm1(-u_i)), u_i = exp(k (log t - f_i)), read at t = |y|: the sign of a target is its
 *                    censoring flag, and on a censored row the PIT lies in [F, 1] (the caller knows which rows those are).  F = 0 for
 *                    t = 0.  Quantile at p: Gamma's scheme -- the host stages g_p = (-log1p(-p))^(1/k), exp(f_i) g_p is component i's own
 *                    quantile, the bracket is multiplicative, widened and VERIFIED, the search the safeguarded Newton search with the
 *                    closed-form density (k / t) u_i exp(-u_i), the same stopping rule, the result the upper end.  cdf_below_out is
 *                    refused; NaN rules as Gamma's, with the scale exp(f_i) for the mean.
 * q_out: host [n_probs][d_out][n] doubles, or NULL (then probs may be NULL too); probs: n_probs probabilities in the OPEN interval (0, 1)
 * (the Gaussian quantile at 0 or 1 is infinite), 1 <= n_probs <= 64.  cdf_out: host [d_out][n] doubles = F(y) at the targets, or NULL; Y is
 * then needed by tbnn_ensemble_loglik's rules (host targets [n, d_out]; NULL with X NULL = the staged targets of `which`; X without Y is
 * refused).  cdf_below_out (TBNN_LIK_POISSON and TBNN_LIK_NEG_BINOMIAL only, with cdf_out; or NULL): [d_out][n] doubles = F(y - 1), the lower end of the target's step
 * (a discrete PIT value lies anywhere in [F(y - 1), F(y)]).  At least one of q_out and cdf_out must be given.
 * NaN: an element with a NaN among its f_i (any weight) gives NaN in every output; so does, among the networks with w_i > 0, a lambda_i
 * that is not finite or exceeds 2^30 (Poisson; negative binomial: 2^20), a Gamma mean exp(f_i) that is 0 or not finite or, for the quantiles alone, an infinite f_i (Gaussian).  A NaN
 * target gives a NaN CDF; under Poisson and the negative binomial so does any target that is not finite, and a negative one gives 0.  Under
 * the negative binomial a target with floor(y) > 2^20 gives a NaN CDF too, no trial of the quantile search goes past k = 2^20, and a
 * probability whose F(2^20) is still below it gives NaN for that probability alone.  Networks of weight 0 add nothing.  The results are the
 * same bits from run to run, and a probability's result does not depend on the others asked with it.  The rows are cut into blocks as for
 * tbnn_ensemble_quantiles (a block's (n_probs + 2) d_out rb results are held beside it).
 * Refused, with nothing written: q_out and cdf_out both NULL, q_out without probs, cdf_below_out without cdf_out or with a Gaussian kind,
 * X without Y when cdf_out is given, n not matching the staged rows, n_probs outside 1 .. 64, a probability outside (0, 1) or NaN,
 * TBNN_LIK_BERNOULLI / TBNN_LIK_CATEGORICAL (the predictive distribution of a label is its posterior-mean probability:
 * tbnn_ensemble_moments returns it), TBNN_LIK_STUDENT_T (the mixture of t CDFs needs the regularised incomplete beta function on the
 * device: not built), any other likelihood code, a NaN sd, weights breaking the rules above, m d_out 64 > 2^28. */
int tbnn_ensemble_predictive(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int likelihood, const float* sd,
                             const float* net_w, int which, const float* X, const float* Y, int64_t n, const double* probs,
                             int32_t n_probs, double* q_out, double* cdf_out, double* cdf_below_out);
/* The continuous ranked probability score (CRPS) of the predictive mixture at the targets: a proper score in the units of the target that
 * rewards calibration and sharpness together, from the closed form for a mixture of Gaussians (Grimit, Gneiting, Berrocal, Johnson 2006) --
 * no quadrature.  Arguments up to `n` as tbnn_ensemble_predictive's (likelihood, sd, net_w, rows, targets).
 * An element is an (output, row) pair.  Under TBNN_LIK_HETERO_GAUSSIAN an element is a row, giving one result plane (od = 1; else
 * od = d_out), as in tbnn_ensemble_predictive.
 *   Network weights are w_i (NULL: all 1), with W = sum_i w_i and omega_i = w_i / W (one rounded fp64 quotient per network, from the host).
 *   Network i predicts f_i, formed in fp32 and widened to fp64.
 *   The scale s_i is sd[i], or fixed_sd when sd is NULL, clipped to [1e-8, 1e8] in fp32 as tbnn_ensemble_loglik clips it.
 *   Under the heteroscedastic kind, s_i = exp(gc_i) per (network, row), gc_i the log-sd output clipped to +-log(1e8).
 *   The target is y.
 * The pair term is
 *   A(mu, sigma) = E|N(mu, sigma^2)| = sigma [2 phi(mu / sigma) + (mu / sigma) erf(mu / (sigma sqrt 2))].
 * Both terms of A are >= 0, so nothing cancels inside it.  The three outputs are
 *   error  = sum_i omega_i A(y - f_i, s_i)                                          = E|Y - y|
 *   spread = 1/2 sum_i sum_j omega_i omega_j A(f_i - f_j, sqrt(s_i^2 + s_j^2))      = 1/2 E|Y - Y'|, the diagonal included, where
 *            A(0, s_i sqrt 2) = 2 s_i / sqrt pi
 *   crps   = error - spread.
 * noise = 0 selects the ensemble CRPS of the networks' outputs alone, the limit s -> 0, where A(mu, 0) = |mu|.  In that mode sd is not
 * read and the heteroscedastic kind reads its mean plane only.  noise = 1: the predictive mixture above.
 * Everything is fp64 and not contracted.  The order of every sum is fixed: the networks are cut into tiles of 8, network i belongs to lane
 * g = i mod 8 of its element's eight; a lane adds its error terms in ascending i, and its pair terms (omega_i omega_j) A_ij for j <= i
 * (the term j = i at half weight, which with the symmetry of A gives the double sum above) over its networks i ascending, for each i the
 * tiles of j ascending and j ascending within a tile; the eight lanes' sums are then added in lane order.  Every one of these sums is
 * compensated (Kahan).  Networks of weight 0 are left out of every sum.  The result is the same bits from run to run, whatever the grid and
 * whatever the row blocks.
 * NaN: a NaN target makes the element NaN.  Gaussian kinds: a NaN f_i under any network, whatever its weight, makes the element NaN.
 * Heteroscedastic kind: a NaN f_i or (noise = 1) g_i of a network that counts makes the element NaN; a network of weight 0 is not looked
 * at.  An infinite f_i among the networks that count makes the element NaN.  All three outputs of such an element are NaN.
 * crps_out, error_out, spread_out: host [od][n] doubles each, or NULL; at least one of the three.  The rows are cut into blocks as for
 * tbnn_ensemble_quantiles (a block's 3 od rb results are held beside it).  The work is m (m + 1) / 2 pair terms per element, an erf and an
 * exp each.
 * Refused, with nothing written: every output NULL, X without Y, noise not 0 or 1, TBNN_LIK_BERNOULLI / TBNN_LIK_CATEGORICAL (a label:
 * tbnn_ensemble_uncertainty), TBNN_LIK_POISSON / TBNN_LIK_NEG_BINOMIAL (the pair term of two count distributions has no closed form: not
 * built), TBNN_LIK_STUDENT_T (no closed form either, and its predictive distribution is not built), any other likelihood code,
 * TBNN_LIK_HETERO_GAUSSIAN with d_out != 2, m > 4096 (a launch is quadratic in m: a limit of the interface), n not matching the staged
 * rows, a NaN sd (noise = 1), weights breaking the rules above, m d_out 64 > 2^28. */
int tbnn_ensemble_crps(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int likelihood, const float* sd,
                       const float* net_w, int which, const float* X, const float* Y, int64_t n, int noise,
                       double* crps_out, double* error_out, double* spread_out);
/* Out-of-sample model comparison: Pareto-smoothed importance-sampling leave-one-out cross-validation (Vehtari, Gelman, Gabry 2017; Vehtari,
 * Simpson, Gelman, Yao, Gabry 2024) and WAIC, from the m x n matrix of per-network, per-row log-likelihoods, which is formed and reduced on the
 * device.  The algorithm is the R package loo's, continuous in its inputs (not ArviZ's variant, which drops fit weights below 10 eps).
 * Arguments up to `n` as tbnn_ensemble_loglik's (likelihood, sd, rows, targets), without net_w: smoothing the ratios of an ensemble that is
 * already importance-weighted is not defined here.  r_eff: the relative efficiency of the draws (1: independent), one number for all rows.
 * l_i is the row's log-likelihood under network i, summed over its outputs: the terms of tbnn_ensemble_loglik, the same bits.  Everything
 * after l_i is fp64, not contracted.  Per row:
 *   lppd      logsumexp_i(l_i) - log m                                  (the bits of tbnn_ensemble_loglik's lppd_rows without weights)
 *   p_waic    sum_i (l_i - mean l)^2 / (m - 1), centred; elpd_waic = lppd - p_waic is left to the caller
 *   ratios    x_i = -l_i - max_j(-l_j): the largest is exactly 0
 *   tail      M = ceil(min(0.2 m, 3 sqrt(m / r_eff))); with v_(1) <= ... <= v_(m) the sorted x, the tail is v_(m-M+1 .. m) and the cutoff
 *             c = v_(m-M).  Only the multiset of values counts, so ties need no rule
 *   no smoothing if M < 5, or the tail's range v_(m) - v_(m-M+1) is 0, or y_(q) below is not > 0: k = +inf and the raw x_i are used
 *   fit       (Zhang and Stephens 2009, with loo's priors)  y_j = exp(v_(m-M+j)) - exp(c), j = 1 .. M; q = floor(M / 4 + 1/2),
 *             G = 30 + floor(sqrt M); for g = 1 .. G: b_g = 1 / y_(M) + (1 - sqrt(G / (g - 1/2))) / (3 y_(q)),
 *             kappa_g = (1/M) sum_j log1p(-b_g y_j), L_g = M (log(-b_g / kappa_g) - kappa_g - 1), w_g = exp(L_g - logsumexp_g L), all G kept;
 *             b = sum_g b_g w_g, kappa = (1/M) sum_j log1p(-b y_j), sigma = -kappa / b, k = (M kappa + 5) / (M + 10)
 *   smoothing the j-th smallest tail value becomes log(exp(c) + sigma expm1(-k log1p(-p_j)) / k), p_j = (j - 1/2) / M (|k| < 2^-52:
 *             -sigma log1p(-p_j) for the quotient), then at most 0.  A k or sigma that is not finite: the raw x_i, and the k obtained
 *   loo       with the final lw_i: elpd_loo = logsumexp_i(lw_i + l_i) - logsumexp_i(lw_i)
 * A NaN or infinity among a row's l_i gives NaN in every row output of that row; its neighbours are unaffected.  pareto_k says where
 * elpd_loo can be trusted (below min(1 - 1 / log10 m, 0.7)).  elpd_loo_rows, pareto_k_rows, lppd_rows, p_waic_rows: n doubles each, or
 * NULL; pointwise: host [m][n] doubles = l_i per row (ArviZ's log_likelihood group), or NULL; at least one of the five.  Without
 * elpd_loo_rows and pareto_k_rows the smoothing kernel is not launched.  The device finds c without a sort (bisection on the order-preserving
 * 64-bit key of an fp64 value, 64 passes over the row's m values), ranks the tail by counting and carries the fit's weights as running sums;
 * one thread per row, the same bits from run to run and whatever the blocks.  The rows are cut into blocks as for tbnn_ensemble_quantiles,
 * the matrix column and the tail, 8 m + 16 M bytes per row, counted into the same budget beside the 4 m d_out of the predictions.
 * Refused, with nothing written: every output NULL, r_eff not finite or not > 0, m < 2, X without Y, n not matching the staged rows, an
 * unknown likelihood code, TBNN_LIK_CATEGORICAL with d_out < 2, a NaN sd, (m d_out + 2 m + 4 M) 64 > 2^28. */
int tbnn_ensemble_loo(tbnn_handle h, const float* thetas, int32_t m, int64_t theta_stride, int likelihood, const float* sd,
                      int which, const float* X, const float* Y, int64_t n, double r_eff, double* elpd_loo_rows, double* pareto_k_rows,
                      double* lppd_rows, double* p_waic_rows, double* pointwise);
/* The degrees of freedom nu that tbnn_ensemble_loglik and tbnn_ensemble_loo use when they judge under TBNN_LIK_STUDENT_T on a handle whose
 * OWN likelihood is another one (a forward handle for saved networks is usually a fixed-sd Gaussian one).  Nothing else reads it.  Refused
 * (-1): a TBNN_LIK_STUDENT_T handle (its nu is the descriptor's lik_df), a df that is not finite and > 0.  The same value is the dispersion r
 * when they judge under TBNN_LIK_NEG_BINOMIAL; a TBNN_LIK_NEG_BINOMIAL handle (its r is the descriptor's lik_df) is refused too.  And the
 * shape a when they -- and tbnn_ensemble_predictive -- judge under TBNN_LIK_GAMMA; a TBNN_LIK_GAMMA handle is refused likewise.  And the
 * shape k under TBNN_LIK_WEIBULL; a TBNN_LIK_WEIBULL handle is refused likewise. */
int tbnn_set_lik_df(tbnn_handle h, float df);
/* metrics.py:30-141 in one pass over the predictions: with p = f*sd+mean, r = y*sd+mean (exp() of either on
 * request: scaleExp; SquaredError leaves the validation predictions un-exponentiated, metrics.py:44-47)
 *   out3[0] = mean (p-r)^2            SquaredError
 *   out3[1] = mean 100*|(p-r)/r|      PercentError
 *   out3[2] = mean |r - round(p)|     1 - Accuracy */
int tbnn_metrics(tbnn_handle h, int which, const float* theta, float mean, float sd, int exp_pred, int exp_real,
                 double out3[3]);

/* predictor.trainProbs / reweight (predictor.py:157-273): for m saved networks, the sum over the dense
 * layers of calculateHyperProbs(hypers, tensors) (layer.py:199-242, :379-422) in ONE launch (one workgroup per network).
 * theta_i = thetas + i * theta_stride (>= P floats), eta_i = etas + i * eta_stride (>= 4 * layers floats: loc_w, g_w, loc_b,
 * g_b per dense layer); priors: `layers` TBNN_PRIOR_* values to judge the layers under (reweight loads another architecture)
 * or NULL = the chain's own.  out: m doubles (sums in fp64). */
int tbnn_hyper_probs_many(tbnn_handle h, const int32_t* priors, const float* thetas, int64_t theta_stride,
                          const float* etas, int64_t eta_stride, int32_t m, double* out);

/* ---- kernels for shapes outside the ahead-of-time registries.  The shape-specialised MFMA kernels are
 * C++ templates; tensorbnn_amd/jit.py instantiates them for a given network with hipcc at run time
 * (cached .so), and this call hands the result to the library: later tbnn_create calls with
 * TBNN_KERNEL_AUTO / _FAST for that shape use it.  (The reference gets the same effect from
 * tf.function tracing + XLA, network.py:359-362.) ---- */
int tbnn_register_kernel_lib(const char* path);
/* 0: no fused kernel covers the shape (KERNEL_AUTO then runs the layered run-time-shape MFMA kernels); 1 / 2: ahead-of-time narrow / wide MFMA kernels; 3: a registered library */
int tbnn_fused_kernel_available(const tbnn_net_desc* desc);

/* ---- RCCL over xGMI.  librccl.so is resolved with dlopen on the first
 * tbnn_comm_* call: single-GPU use never loads it.  One communicator per chain handle; every
 * collective is enqueued on the chain's own stream (no host sync inside a transition). ---- */
#define TBNN_COMM_ID_BYTES 128
typedef struct tbnn_comm* tbnn_comm_handle;
/* rank 0 draws the id (ncclGetUniqueId); the host hands it to the other ranks (torch.distributed
 * broadcast, MPI, a file ...) */
int tbnn_comm_unique_id(unsigned char id[TBNN_COMM_ID_BYTES]);
/* ncclCommInitRank on the chain's device; collective over all `world` ranks */
int tbnn_comm_create(tbnn_handle h, int world, int rank, const unsigned char id[TBNN_COMM_ID_BYTES],
                     tbnn_comm_handle* out);
/* ranks in the communicator as the collective library reports them (ncclCommCount); < 0: error */
int tbnn_comm_count(tbnn_comm_handle c);
int tbnn_comm_destroy(tbnn_comm_handle c);
/* checkpoint-time gather (network.py:610-663 writes one chain; with N chains every rank ends up
 * with all N samples): all-gather of (theta, eta) = P+H floats per rank.  d_out: device buffer of
 * world*(P+H) floats or NULL (library-owned buffer); host_out: world*(P+H) floats or NULL. */
int tbnn_gather_samples(tbnn_handle h, tbnn_comm_handle c, float* d_out, float* host_out);
/* row-sharded single chain: the ranks of `c` hold disjoint row blocks of (X, Y) and identical
 * theta / eta / seed / chain_id; the data-term gradient (P floats) and the likelihood statistic are
 * all-reduced after every fused pass, so every rank takes the same leapfrog trajectory and the same
 * Metropolis decision.  n_total = rows over all ranks (normaliser of the Gaussian likelihood).
 * c == NULL switches back to the unsharded chain.  Refused on a handle with row weights (tbnn_set_row_weights). */
int tbnn_set_row_shard(tbnn_handle h, tbnn_comm_handle c, int64_t n_total);

/* ---- (eps, L) adapter: paramAdapter (tensorBNN/paramAdapter.py:11-292), host C++ ---- */
typedef struct tbnn_adapter* tbnn_adapter_handle;
/* paramAdapter.__init__ :39-93 (k = burnin/averagingSteps, network.py:229-230) */
int tbnn_adapter_create(float e1, int32_t L1, float el, float eu, int32_t eNumber, int32_t Ll,
                        int32_t Lu, int32_t lStep, int32_t m, double k, float a, float delta,
                        int32_t randomSteps, uint64_t seed, tbnn_adapter_handle* out);
int tbnn_adapter_destroy(tbnn_adapter_handle a);
/* paramAdapter.update :199-292.  state: P floats (the new theta).  inject_u
 * (<0: draw) replaces tf.random.uniform :232; inject_e/inject_l (<0: draw)
 * replace random.choice :283-284 with grid indices.  Outputs next (eps, L). */
int tbnn_adapter_update(tbnn_adapter_handle a, const float* state, int32_t P, float inject_u,
                        int32_t inject_e, int32_t inject_l, float* eps_out, int32_t* L_out,
                        float* sjd_out);

/* ---- pre-training on the device: BNN_functions.trainBasicRegression / trainBasicClassification (BNN_functions.py:60-180, :183-297;
 * docs/ClassificationExample.md, Examples/extendedRegression.py start every chain from their result) are Keras Adam with amsgrad=True;
 * here the same update rule ascends the chain's OWN target -- its activations, priors, likelihood, row weights -- with the fused
 * forward+backward pass of whichever kernel family the handle runs.  Added without a new ABI version: the symbols are additions. ----
 *
 * tbnn_optimize runs n_steps >= 0 full-batch steps back to back on the chain's stream (no host round trip), from theta_0 = the
 * chain's state.  With g_t the gradient at theta_t of the objective (TBNN_OPT_POSTERIOR: the target log-probability tbnn_logp_grad
 * returns, priors included; TBNN_OPT_LIKELIHOOD: the data log-likelihood alone, row weights included) and t counting from 1 since the
 * last reset, one step is torch.optim.Adam(lr, betas, eps, amsgrad, maximize=True)'s, in fp32:
 *   m = beta1 m + (1 - beta1) g_t ;  v = beta2 v + (1 - beta2) g_t^2 ;  vhat = amsgrad ? max(vhat, v) : v
 *   theta_{t+1} = theta_t + a_t m / (sqrt(vhat) r_t + epsilon),   a_t = lr / (1 - beta1^t),   r_t = 1 / sqrt(1 - beta2^t)
 * (a_t, r_t and 1 - beta formed in fp64 from the fp32 arguments and rounded once).
 * Checks: the objective is evaluated at theta_t for the call's steps t = 0, k, 2k, .. < n_steps (k = check_every) and once more at
 * theta_{n_steps}: n_checks = ceil(n_steps / k) + 1 values per chain, in step order (n_steps = 0: one evaluation, no step).  The value is
 * the true log-density (Poisson with its constant), summed in fp64.  A check whose value is finite and above every earlier one since the
 * last reset records theta_t as the best weights; a check whose value is NOT finite freezes the chain: it makes no further update, in this
 * call or a later one without reset (diverged = 1).  Between two checks nothing is judged.
 * After the call the chain's state is the best weights when keep_best is set or the chain froze, else theta_{n_steps}; the cached
 * (log-prob, gradient) of the state is dropped, so the next transition or tbnn_logp_grad evaluates afresh.  Hypers, the epoch counter
 * and the random stream are untouched: the call draws nothing.
 * reset != 0 zeroes m, v, vhat, t and the best record (best weights = the start state) first; reset == 0 continues them, so that a run
 * cut into blocks with keep_best = 0 takes the same steps as one call (the first call on a handle always resets).
 * Multi-chain handle: every chain is optimised from its own state in the same launches; out[chains], trace[chains][n_checks]; a frozen
 * chain does not hold up the others.
 * out (per chain): steps_done = n_steps, or for a chain that froze the step of the check that froze it (0: frozen before the call);
 * diverged; best_step: the step counter t (since the last reset) of the best check; n_checks; obj_first / obj_last: the first and last
 * check of this call; obj_best: the best since the last reset (-inf: none was finite); device_us: hipEvent time of the whole run.
 * Errors (the handle is left as it was): no data staged; a row-sharded handle (tbnn_set_row_shard); NULL cfg or out; n_steps < 0;
 * check_every < 1; lr or epsilon not finite or not > 0; a beta outside [0, 1); an unknown objective. */
enum { TBNN_OPT_POSTERIOR = 0, TBNN_OPT_LIKELIHOOD = 1 };
typedef struct tbnn_optim_cfg { float lr, beta1, beta2, epsilon; int32_t amsgrad, objective, check_every, keep_best; } tbnn_optim_cfg;
typedef struct tbnn_optim_out { int32_t steps_done, diverged, best_step, n_checks; double obj_first, obj_last, obj_best; float device_us; } tbnn_optim_out;
int tbnn_optimize(tbnn_handle h, const tbnn_optim_cfg* cfg, int32_t n_steps, int32_t reset, tbnn_optim_out* out /* [chains] */,
                  double* trace /* [chains][n_checks] or NULL */);
/* diagnostic: the optimiser's moments, the total gradient g of its last step ([chains][P] floats each) and its step counter t; any
 * pointer may be NULL.  An error before the first tbnn_optimize. */
int tbnn_optim_state(tbnn_handle h, float* m, float* v, float* vhat, float* g, int32_t* t);

#ifdef __cplusplus
}
#endif
#endif /* TBNN_H */
