/*
 * vjf_hip.h -- C ABI of the MI355X (gfx950) implementation of VJF's online filtering step.
 *
 * This is the drop-in boundary for ONE hot path of catniplab/vjf: `VJF.filter`
 * (vjf/model.py:179-221) batched over independent trials, plus the stand-alone operators it is
 * built from.  The reference has no FFI (it is pure Python on torch-CPU); the entry points below
 * are what a binding for that path calls -- the Python side (vjf_amd/_native.py, ctypes) is the
 * reference-shaped host code, see INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (never throws); vjf_last_error() gives text;
 *   - all tensor pointers are DEVICE pointers to row-major contiguous fp32 unless stated;
 *   - the library never allocates device memory: the caller owns `state` and `workspace`
 *     (sizes from vjf_state_size / vjf_workspace_size) and may alias `state` as tensors;
 *   - calls are asynchronous on the context's HIP stream and ordered on it; one context is not
 *     re-entrant, several contexts may coexist (SURVEY.md 8b "Threading"): the launches of the one-launch route -- a grid that
 *     must be resident as a whole -- are chained across the contexts of a process (each waits for the completion of the
 *     previous one, whichever context and stream it came from), and a grid that shares the device with ANOTHER process's
 *     ends within a quarter of a second with VJF_STATUS_NOT_RESIDENT, the state untouched;
 *   - besides the caller's `state` and `workspace` the library holds one page of pinned HOST memory per process and device:
 *     the words through which a launch that has given up a wait tells the host (read at the start of the next call).
 */
#ifndef VJF_HIP_H
#define VJF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VJF_ABI_VERSION 1
#define VJF_MAX_HIDDEN 8

/* likelihood kinds (vjf/likelihood.py:9, :43) */
#define VJF_LIK_GAUSSIAN 0
#define VJF_LIK_POISSON 1

/* per-call flags of VJF.filter (vjf/model.py:180) */
#define VJF_FLAG_SGD 1u      /* sgd=True    : backward, clip to +-1, SGD step (model.py:206-214) */
#define VJF_FLAG_UPDATE 2u   /* update=True : closed-form updates (model.py:215-216, 156-177)   */
#define VJF_FLAG_WARM_UP 4u  /* warm_up=True: no dynamics term / no RLS (model.py:148, 370)     */
#define VJF_FLAG_EXACT_NONFINITE 8u   /* trials sharded over ranks (communicators in the context): a step whose loss has a non-finite
                                       * component is REPLAYED as on one rank (model.py:138-149: the component becomes the constant 0,
                                       * the gradient is that of the others) -- at the price of a second sum over ranks in EVERY step
                                       * (its launches return at once on ordinary steps, the collective itself cannot be skipped:
                                       * every rank must enter it).  Without the flag such a step's SGD update is skipped and
                                       * VJF_STATUS_NONFINITE_* raised.  No effect on one rank (always replayed there). */

/* sticky status bits, read with vjf_get_status */
#define VJF_STATUS_NONFINITE_RECON 1u   /* l_recon non-finite -> replaced by 0 (model.py:138-139) */
#define VJF_STATUS_NONFINITE_DYN 2u     /* l_dynamics non-finite (model.py:141-142)               */
#define VJF_STATUS_NONFINITE_ENT 4u     /* entropy non-finite (model.py:144-145)                  */
#define VJF_STATUS_RLS_FAILED 8u        /* Cholesky pivot <= 0 in rls: RLS state left unchanged   */
/* detail bits beside VJF_STATUS_RLS_FAILED: which bounded in-kernel wait of vjf_filter_seq / vjf_filter_step ran out (a role or
   kernel waited for another one that did not deliver in time; results of the call are then not to be used) */
#define VJF_STATUS_WAIT_RESIDENT 0x100u  /* SGD role / kernel: the trial role's late slabs                         */
#define VJF_STATUS_WAIT_OPERAND 0x200u   /* operand role / kernel: its inputs (early slabs, statistics, previous RLS update) */
#define VJF_STATUS_WAIT_STATS 0x400u     /* Cholesky loop: statistics reduced                                      */
#define VJF_STATUS_WAIT_SIGMA 0x800u     /* Cholesky loop: previous step's sigma / RLS update                      */
#define VJF_STATUS_WAIT_GATE 0x1000u     /* trial role: parameters of the previous step; a gate kernel of the per-step route */
#define VJF_STATUS_WAIT_GATE2 0x2000u    /* Gram role: posterior, previous slab sum                                */
#define VJF_STATUS_WAIT_G 0x4000u        /* y / W loop: operands (g)                                               */
#define VJF_STATUS_WAIT_COLUMN 0x8000u   /* y / W and inverse loops: a column of L, or the trial role's readers    */
#define VJF_STATUS_WAIT_K1 0x10000u      /* trial role / kernel: previous step's RLS update                        */
#define VJF_STATUS_NOT_RESIDENT 0x20000u /* one-launch route: not every workgroup of the grid was placed on the device in time (another
                                          * process's kernels hold compute units): the launch ended before it touched the state; the
                                          * context leaves the one-launch route */
#define VJF_STATUS_WAIT_MASK 0x3ff00u    /* any of the above: the outputs of the call that raised it are not to be used.  The NEXT
                                          * vjf_filter_* call of the context fails (it would chain invalid results) until
                                          * vjf_get_status has been called. */

/* Slots of the state blob, in the reference's state_dict order followed by the plain-attribute
 * RLS tensors and the scalars the reference keeps as Python numbers. */
enum vjf_slot {
    VJF_SLOT_PRIOR_MEAN = 0,   /* (xdim)            VJF.mean            model.py:66  */
    VJF_SLOT_PRIOR_LOGVAR = 1, /* (xdim)            VJF.logvar          model.py:67  */
    VJF_SLOT_LIK_LOGVAR = 2,   /* (1) Gaussian only likelihood.logvar   likelihood.py:16 */
    VJF_SLOT_TR_LOGVAR = 3,    /* (1)               transition.logvar   model.py:331 */
    VJF_SLOT_CENTROID = 4,     /* (n_rbf, xdim+udim) feature.centroid   module.py:20 */
    VJF_SLOT_LOGWIDTH = 5,     /* (n_rbf)           feature.logwidth    module.py:21 */
    VJF_SLOT_REC_W0 = 6,       /* +2k: (h_k, h_{k-1}) recognition.mlp.{2k}.weight  recognition.py:20-26 */
    VJF_SLOT_REC_B0 = 7,       /* +2k: (h_k)          recognition.mlp.{2k}.bias    */
    VJF_SLOT_MEAN_W = 22,      /* (xdim, h_L)  recognition.mean.weight    recognition.py:27 */
    VJF_SLOT_LV_W = 23,        /* (xdim, h_L)  recognition.logvar.weight  recognition.py:28 */
    VJF_SLOT_LV_B = 24,        /* (xdim)       recognition.logvar.bias    */
    VJF_SLOT_DEC_W = 25,       /* (ydim, xdim) decoder.decode.weight      model.py:24 */
    VJF_SLOT_DEC_B = 26,       /* (ydim)       decoder.decode.bias        */
    VJF_SLOT_W_MEAN = 27,      /* (n_rbf, xdim)  velocity.w_mean       module.py:50  */
    VJF_SLOT_W_CHOL = 28,      /* (n_rbf, n_rbf) velocity.w_chol       module.py:52  (upper: inv(L^T)) */
    VJF_SLOT_W_PREC = 29,      /* (n_rbf, n_rbf) velocity.w_precision  module.py:53  */
    VJF_SLOT_W_PCHOL = 30,     /* (n_rbf, n_rbf) velocity.w_pchol      module.py:54  (lower L) */
    VJF_SLOT_SCALARS = 31,     /* (16) see vjf_scalar */
    VJF_N_SLOTS = 32
};

/* indices into the SCALARS slot (all stored as fp32; the counters are exact integers < 2^24) */
enum vjf_scalar {
    VJF_SC_N_LIK = 0,   /* likelihood.n_sample  likelihood.py:17 */
    VJF_SC_N_TR = 1,    /* transition.n_sample  model.py:332     */
    VJF_SC_LR_LIK = 2,  /* optimizer.param_groups[0..3]['lr']  model.py:69-77 */
    VJF_SC_LR_DEC = 3,
    VJF_SC_LR_TR = 4,
    VJF_SC_LR_REC = 5,
    VJF_SC_FREEZE_DEC = 6, /* 1.0 after decoder.requires_grad_(False)  model.py:283 */
    VJF_SC_STATUS = 7,     /* status bits as an integer-valued float */
    VJF_SC_TRI_CLEAN = 8,  /* device-internal: 1 once the zero halves of w_chol / w_pchol have been cleared;
                              write 0 after storing a dense matrix into either tensor from the host */
    VJF_SC_SHRINK = 9,     /* velocity.rls forgetting factor  module.py:80-96; a stored 0 reads as 1 (every state written
                              before the slot had a meaning is zero there) */
    VJF_N_SCALARS = 16
};

typedef struct vjf_config {
    int32_t ydim, xdim, udim, n_rbf;
    int32_t n_hidden;                /* 1..VJF_MAX_HIDDEN */
    int32_t hidden[VJF_MAX_HIDDEN];  /* hidden_sizes of Recognition (recognition.py:17) */
    int32_t likelihood;              /* VJF_LIK_* */
    int32_t max_batch;               /* largest B (trials per call on this device) the workspace serves */
    int32_t device;                  /* HIP device ordinal */
} vjf_config;

/* Activation of the recognition layers (vjf/recognition.py:17-24: `activation`, one class for every layer; default Tanh).
 * Supported: the activations whose derivative follows from the layer's output (the routes keep no pre-activation). */
#define VJF_ACT_TANH 0
#define VJF_ACT_RELU 1
#define VJF_ACT_LEAKY_RELU 2   /* p0 = negative_slope >= 0 */
#define VJF_ACT_ELU 3          /* p0 = alpha > 0 */
#define VJF_ACT_SOFTPLUS 4     /* p0 = beta > 0, p1 = threshold >= 20 */
#define VJF_ACT_SIGMOID 5
#define VJF_ACT_HARDTANH 6     /* p0 = min_val < p1 = max_val (ReLU6: 0, 6) */
typedef struct vjf_activation { int32_t kind; float p0, p1; } vjf_activation;

typedef struct vjf_ctx vjf_ctx;

int vjf_abi_version(void);
/* Text of the last error raised on the calling thread ("" if none). */
const char* vjf_last_error(void);

/* ---- memory plan ------------------------------------------------------------------------- */
/* Number of fp32 elements of the state blob for `cfg`. */
int vjf_state_size(const vjf_config* cfg, int64_t* n_floats);
/* offsets[slot], sizes[slot] (fp32 elements) for the VJF_N_SLOTS slots; unused slots have size 0. */
int vjf_state_layout(const vjf_config* cfg, int64_t* offsets, int64_t* sizes);
/* Bytes of scratch the context needs for cfg->max_batch trials. */
int vjf_workspace_size(const vjf_config* cfg, int64_t* bytes);
/* The gradient-tile table of the one-launch route's training kernel for `cfg` (pure arithmetic, callable without a GPU): 16 header
 * words -- [0] tiles, [1] segments, [2 + s] end of segment s -- then 8 words per 16x16 tile: {LDS float of the tile's first delta row,
 * delta rows from there, LDS float of its first input row, input rows from there (the row AT that count is the ones row), first
 * float of the tile in the late slab, the slab block's row length, slab rows stored, slab columns stored}.  `n_words` (may be null)
 * gets the table's length; `table` (may be null) is filled when `capacity` >= that length, else -7. */
int vjf_mega_grad_tile_table(const vjf_config* cfg, int32_t* table, int32_t capacity, int32_t* n_words);

/* ---- context ------------------------------------------------------------------------------ */
/* `state` (fp32, vjf_state_size floats) and `workspace` stay owned by the caller and must outlive
 * the context.  `stream` is a hipStream_t (NULL = the null stream). */
int vjf_ctx_create(const vjf_config* cfg, float* state, void* workspace, int64_t workspace_bytes,
                   void* stream, vjf_ctx** out);
int vjf_ctx_destroy(vjf_ctx* ctx);
/* Activation of the recognition layers (vjf/recognition.py:17-24; a new context has VJF_ACT_TANH).  Valid on a context that has
 * not yet run a vjf_filter_* call (else an error); re-runs the one-launch residency check for the kernels it selects (when they
 * cannot be resident the context takes the per-step route, and vjf_route says so).  Invalid kinds or parameters: < 0. */
int vjf_set_activation(vjf_ctx* ctx, const vjf_activation* act);
int vjf_set_stream(vjf_ctx* ctx, void* stream);
/* Synchronises the stream, returns and clears the sticky status bits. */
int vjf_get_status(vjf_ctx* ctx, uint32_t* status);

/* Which schedule vjf_filter_seq / vjf_filter_step use on a single rank (results agree to summation order; the one-launch and
 * three-stream routes are bit-identical to each other):
 *   1 (default)  the one-launch route: ONE launch carries the whole call; the trial, Gram, operand, SGD and RLS roles are
 *                workgroups of one grid, resident as a whole (checked against the occupancy query before it is launched), that
 *                hand over through counters in memory (plans it serves: see vjf_route);
 *                plans whose RLS update is a sequence of launches (n_rbf > 224) run that update on a second internal stream,
 *                beside the backward half of its step and the forward half of the next (bit-identical to the one-stream order);
 *   3            the per-step route on three internal streams (the route the RCCL path uses), for A/B measurements;
 *   0            the per-step kernels in the one-stream order (also what tools that serialise kernels need).
 * Returns the resulting setting, or a negative error code. */
int vjf_set_overlap(vjf_ctx* ctx, int enable);

/* The route a vjf_filter_seq call with these flags would take now: 1 one-launch, 3 three-stream per-step (with communicators:
 * the RCCL route), 2 per-step with the multi-launch RLS update on a second stream (T > 1), 4 per-step with ONE all-reduce per
 * step (vjf_set_collectives), 0 one-stream per-step.
 * Negative on error. */
int vjf_route(vjf_ctx* ctx, uint32_t flags);

/* Trials sharded over ranks, one process per GPU: with communicators attached, vjf_filter_seq sums the RLS statistics and
 * the gradients over ranks itself (two RCCL all-reduces per step, one on each chain of its schedule) and B in its
 * arguments is the LOCAL batch.  RCCL is resolved at run time from the process (torch's copy) or librccl.so.
 * vjf_comm_unique_id: rank 0 fills 256 bytes (two ncclUniqueId) that the caller broadcasts to every rank;
 * vjf_comm_init: every rank, collectively.  Replaces the caller-side all-reduce between vjf_filter_local and
 * vjf_filter_global (vjf/model.py has no multi-GPU path: SURVEY 8e). */
int vjf_comm_unique_id(void* ids256);
int vjf_comm_init(vjf_ctx* ctx, const void* ids256, int32_t rank, int32_t world);
/* How many sums over ranks a step of vjf_filter_seq makes on the in-library route: 2 (default) -- [gradients | loss sums] on the
 * trial chain and [Phi^T Phi | Phi^T dx | sum |dx|^2] on the statistics chain of the three-stream schedule, overlapping each other
 * and the other chain's kernels -- or 1: the whole reduce buffer in ONE all-reduce between the trial-parallel and the serial half
 * of the step (SURVEY.md 8e's packed layout; any flags, one stream, no overlap of the two chains).  Same results to summation
 * order.  Also: VJF_COLLECTIVES=1 in the environment when the context is created. */
int vjf_set_collectives(vjf_ctx* ctx, int32_t per_step);
/* What RCCL itself says about the context's two communicators: ranks[0], ranks[1] = ncclCommCount of the gradient chain's and of
 * the statistics chain's communicator (0, 0 without communicators).  A benchmark line quotes these, not the launcher's
 * environment. */
int vjf_comm_ranks(vjf_ctx* ctx, int32_t* ranks2);

/* Diagnostic: enable/disable s_memtime phase stamps in the serial kernel and (out32 != NULL) copy the
 * 32 stamp words of the last step to the host.  Not part of the reference surface. */
int vjf_debug_stamps(vjf_ctx* ctx, int enable, uint64_t* out32);

/* ---- the hot path: VJF.filter (vjf/model.py:179-221) ---------------------------------------- */
/* One filtering step on B trials.
 *   y (B,ydim); u (B,udim) or NULL; mu_s, lv_s (B,xdim) previous posterior, both NULL => prior
 *   (model.py:107-108); eps_s, eps_t (B,xdim) the two reparametrisation draws in the reference's
 *   order xs then xt (util.py:11-13); outputs mu_t, lv_t (B,xdim) = qt, loss4 (4) =
 *   {loss, -l_recon, -l_dynamics, entropy} (model.py:152).  Equivalent to
 *   vjf_filter_local + vjf_filter_global with B_total = B. */
int vjf_filter_step(vjf_ctx* ctx, int32_t B, const float* y, const float* u, const float* mu_s,
                    const float* lv_s, const float* eps_s, const float* eps_t, float* mu_t, float* lv_t,
                    float* loss4, uint32_t flags);

/* Trial-parallel half of a step: everything per trial plus this device's partial sums, written
 * to the reduce buffer (gradient sums, RLS statistics Phi^T Phi, Phi^T dx, loss sums).  With
 * trials sharded over devices the caller all-reduces (sum) that buffer between the two halves. */
int vjf_filter_local(vjf_ctx* ctx, int32_t B, const float* y, const float* u, const float* mu_s,
                     const float* lv_s, const float* eps_s, const float* eps_t, float* mu_t, float* lv_t,
                     uint32_t flags);
/* Device pointer / length (fp32 elements) of the reduce buffer (lives inside `workspace`). */
int vjf_reduce_buffer(vjf_ctx* ctx, float** ptr, int64_t* n_floats);
/* Serial half: finite guards, clip, SGD, likelihood running variance, RLS (Cholesky, solve,
 * triangular inverse), state-noise running variance, from the (all-reduced) buffer.
 * B_total = trials summed over all devices.  (A step with a non-finite loss component: this half alone cannot re-form the
 * gradient without the dropped component -- the SGD step is skipped, the status bit raised; vjf_filter_step / vjf_filter_seq
 * on one rank replay the backward half, see vjf_filter_seq.) */
int vjf_filter_global(vjf_ctx* ctx, int32_t B_total, float* loss4, uint32_t flags);

/* T successive steps, each fed the previous posterior: the inner loop of VJF.fit
 * (model.py:252-261).  y (T,B,ydim); u (T,B,udim) or NULL; eps (T,2,B,xdim);
 * mu0/lv0 (B,xdim) or NULL => prior; outputs mu, lv (T,B,xdim), loss (T,4).
 * On a single rank with sgd + update and no warm-up (plans the one-launch route serves: see vjf_route) the whole call -- per
 * chunk of 16384 steps -- is ONE kernel launch (a grid resident as a whole); the call stays asynchronous.  With communicators (vjf_comm_init)
 * the steps run as per-step kernels on three internal streams with the sums over ranks done by RCCL; otherwise step by step
 * on the caller's stream.  Every in-kernel wait is bounded: one that runs out raises VJF_STATUS_RLS_FAILED plus a
 * VJF_STATUS_WAIT_* detail bit (vjf_get_status), ends the other waits of the call at once, and the outputs of the call are
 * not to be used.  A loss component that is not finite (VJF_STATUS_NONFINITE_*) is handled as vjf/model.py:138-149 does
 * (the component becomes 0 and the step's gradient is that of the others) on the one-launch route and on the one-stream
 * per-step route of a single rank (there the backward half, the gradient sums and the SGD pass are launched again behind the
 * first SGD pass; they return at once on ordinary steps).  Where trials are sharded over ranks (communicators, or
 * vjf_filter_local / vjf_filter_global around the caller's all-reduce: a replay would need a second sum over ranks), on the
 * three-stream route of one rank and on plans served by the generic single-workgroup serial kernel the SGD step of such a
 * step is skipped. */
int vjf_filter_seq(vjf_ctx* ctx, int32_t T, int32_t B, const float* y, const float* u, const float* eps,
                   const float* mu0, const float* lv0, float* mu, float* lv, float* loss, uint32_t flags);

/* ---- stand-alone operators (the reference's vjf.module / vjf.functional surface) ------------ */
/* functional.rbf (vjf/functional.py:11-22): out(B,n) = exp(-1/2 |x-c|^2 / exp(logw)^2). */
int vjf_rbf_forward(const float* x, const float* centroid, const float* logwidth, float* out,
                    int32_t B, int32_t n, int32_t d, void* stream);
/* LinearRegression.forward(sampling=False) (vjf/module.py:64-77): mean(B,dout), logvar(B,dout). */
int vjf_blr_predict(const float* x, const float* centroid, const float* logwidth, const float* w_mean,
                    const float* w_chol, float* mean, float* logvar, int32_t B, int32_t n, int32_t d,
                    int32_t dout, void* stream);
/* LinearRegression.forward(sampling=True) (vjf/module.py:70-73): out = feat @ (w_mean + w_chol @ noise). */
int vjf_blr_sample(const float* x, const float* centroid, const float* logwidth, const float* w_mean,
                   const float* w_chol, const float* noise, float* out, float* w_scratch, int32_t B,
                   int32_t n, int32_t d, int32_t dout, void* stream);
/* RBFDS.forecast (vjf/model.py:342-361) with the sampling branch of LinearRegression.forward (vjf/module.py:70-73) for every
 * step, as one call:  x[0] = x0;  x[t+1] = x[t] + Phi([x[t], u[t]]) (w_mean + w_chol @ w_noise[t])  (+ s_noise[t] exp(tr_logvar / 2)).
 * x (T+1,B,dout) out; u (T,B,du) or NULL (du = d - dout); w_noise (T,n,dout); s_noise (T,B,dout) or NULL; tr_logvar: device
 * scalar (read only when s_noise is given).  w_chol is read as a dense matrix.  Asynchronous on `stream`, no host synchronisation;
 * reads the state tensors, writes none.  Steps run in chunks (two launches each) whose weight samples live in `scratch`:
 * >= vjf_forecast_scratch_size(T,n,dout) bytes, at most 8 MiB (+ four rows of padding) whatever T is, or one step's n dout floats where that is
 * more; a chunk is at most 4096 steps.  -1 null tensor, -20 bad shape, -21 u missing with d > dout, -11 n (d) beyond one
 * workgroup's LDS. */
int vjf_forecast_scratch_size(int32_t T, int32_t n, int32_t dout, int64_t* bytes);
int vjf_forecast_seq(const float* x0, const float* u, const float* w_noise, const float* s_noise, const float* centroid,
                     const float* logwidth, const float* w_mean, const float* w_chol, const float* tr_logvar, float* x,
                     void* scratch, int32_t T, int32_t B, int32_t n, int32_t d, int32_t dout, void* stream);
/* An ensemble of S roll-outs of RBFDS.forecast (vjf/model.py:342-361; every step draws its own weights, vjf/module.py:70-73, so
 * one roll-out is one draw of the predictive distribution) and VJF.forecast's decoding of each (vjf/model.py:321-324), reduced to
 * the per-step mean and population variance over the members, as one call.  Member s is vjf_forecast_seq on
 * x0 + s * x0_member_stride, w_noise[s], s_noise[s], bit for bit; x0_member_stride (floats) is 0 for one start (B,dout) shared by
 * the members or B * dout for x0 (S,B,dout).  w_noise (S,T,n,dout); s_noise (S,T,B,dout) or NULL; u (T,B,du) or NULL, shared.
 * Out: x_mean, x_var (T+1,B,dout); y_mean, y_var (T+1,B,dy) of y = x dec_W^T + dec_b, dec_W (dy,dout) -- dec_W == NULL: no y
 * outputs (dec_b, y_mean, y_var, dy are ignored); x_members (S,T+1,B,dout) or NULL: the members are not kept.  The decoded members
 * never reach memory.  Every output element is folded over the members in member order (Welford, fp32) by one lane, so its bits
 * depend on that trial's inputs alone; S = 1 gives the roll-out itself and variances of exactly 0.  T = 0: the moments of the starts
 * (x_members is not written).  Asynchronous on `stream`, no host synchronisation; reads the state tensors, writes none.
 * Members and steps run in chunks (three launches each) whose weight samples and states live in `scratch`:
 * >= vjf_forecast_ens_scratch_size(T,S,B,n,dout) bytes, whatever T and S are at most 8 MiB of weight samples (+ four rows of
 * padding; or one sample's n dout floats where that is more) + 32 MiB of member states (or two rows of B dout floats where that is
 * more); a chunk is at most 4096 steps and 4096 members.  -1 null tensor, -20 bad shape, -21 u missing with d > dout, -11 n (d,
 * dout) beyond one workgroup's LDS: all before the first launch. */
int vjf_forecast_ens_scratch_size(int32_t T, int32_t S, int32_t B, int32_t n, int32_t dout, int64_t* bytes);
/* The chunking vjf_forecast_ens takes for these sizes (VJF_FE_MEMBERS / VJF_FC_CHUNK included): members and steps per chunk.  A chunk
 * needs members * steps * n * dout * 4 bytes of weight samples and members * (steps + 1) * B * dout * 4 bytes of states, both inside
 * vjf_forecast_ens_scratch_size's bound for every T >= 1 and S (tests sweep it; the call checks it before its first launch). */
int vjf_forecast_ens_chunks(int32_t T, int32_t S, int32_t B, int32_t n, int32_t dout, int32_t* members, int32_t* steps);
int vjf_forecast_ens(const float* x0, int64_t x0_member_stride, const float* u, const float* w_noise, const float* s_noise,
                     const float* centroid, const float* logwidth, const float* w_mean, const float* w_chol,
                     const float* tr_logvar, const float* dec_W, const float* dec_b, float* x_mean, float* x_var,
                     float* y_mean, float* y_var, float* x_members, void* scratch, int32_t T, int32_t S, int32_t B,
                     int32_t n, int32_t d, int32_t dout, int32_t dy, void* stream);
/* Tangent dynamics of the mean map of RBFDS.forward(sampling=False) (vjf/model.py:334-340 over vjf/module.py:64-77),
 *   f(x, u) = x + Phi([x, u]) w_mean,   J(x, u) = df/dx = I - w_mean^T G,   G[k][j] = phi_k (x_j - c_kj) / exp(logwidth_k)^2,
 * as one call: T steps of x[t+1] = f(x[t], u[t]), Q <- J(x[t], u[t]) Q for a frame Q (dout x m per trial), and every qr_every steps
 * (and behind the last step) one pass of modified Gram-Schmidt in column order on every trial's frame, fp32, R_vv > 0, log R_vv added
 * to lsum[b][v] in interval order and stored to lhist[interval][b][v] if given.  lsum / (T dt) are the m leading Lyapunov exponents
 * in Gram-Schmidt column order.  qr_every = 0: the frame is never normalised and q_out is the raw product -- one step from Q = I with
 * m = dout is J itself, q_out[b][i][j] = df_i/dx_j (lsum may be NULL, lhist must be).
 * x0 (B,dout); u (T,B,du) or NULL (du = d - dout); q0 (B,dout,m) or NULL: the first m columns of I; x_out (B,dout), q_out (B,dout,m):
 * the final state and frame, from which a further call continues the run bit for bit when the cut is at an interval boundary; lsum
 * (B,m) in/out (accumulate = 0: the sums start from 0 and lsum is only written); lhist (ceil(T / qr_every),B,m) or NULL.
 * T = 0: x_out = x0, q0 is orthonormalised once and its log R_vv are added (qr_every > 0).  A trial's outputs depend on that trial's
 * inputs alone, bit for bit.  Asynchronous on `stream`, no host synchronisation, no scratch; reads the state tensors, writes none.
 * Steps run in launches of at most 4096 (VJF_FC_CHUNK: fewer), the state carried through the output buffers.
 * -1 null tensor, -20 bad shape (also m < 1, m > dout, qr_every < 0, lhist with qr_every = 0), -21 u missing with d > dout, -11 the
 * shape is beyond one workgroup's LDS or dout > 64: all before the first launch.
 * vjf_tangent_plan: what the call takes for these sizes -- tangent vectors per pass over the features (m wherever it fits; the
 * results do not depend on it) and the dynamic LDS of a workgroup; -11 / -20 as the call. */
int vjf_tangent_plan(int32_t n, int32_t d, int32_t dout, int32_t m, int32_t* vectors_per_pass, int64_t* lds_bytes);
int vjf_tangent_rollout(const float* x0, const float* u, const float* q0, const float* centroid, const float* logwidth,
                        const float* w_mean, float* x_out, float* q_out, float* lsum, float* lhist, int32_t T, int32_t B,
                        int32_t n, int32_t d, int32_t dout, int32_t m, int32_t qr_every, int32_t accumulate, void* stream);
/* Fixed points of the same mean map: for each start x0[b] and constant input u[b] (a parameter of the map), x with
 *   g(x, u) = Phi([x, u]) w_mean = 0,   A = dg/dx = -w_mean^T G  (J = I + A),
 * by a damped Newton (Levenberg-Marquardt) search on |g|^2, the whole search as one call, fp32.  Per trial: x = xc = x0, r2 = +inf,
 * lam = lam0, M = 0 (dout x dout), b = 0 (dout), done = false, n_iter = 0.  For k = 0 .. max_iter, for every trial not done:
 *   1. g = g(xc, u), A = A(xc, u), r2c = sum_i g_i^2;
 *   2. r2c < r2 (a NaN compares false): accept -- x = xc, r2 = r2c, M = A^T A, b = A^T g, and with k > 0 lam = max(lam / 10, 1e-7);
 *   3. else reject -- lam = min(lam * 10, 1e7);
 *   4. done = (r2 <= tol^2);   5. k == max_iter: stop;
 *   6. not done: n_iter += 1, mu = trace(M) / dout, K = M + (lam mu) I = L L^T (Cholesky), K delta = -b, xc = x + delta; a pivot that
 *      is not positive and finite: xc = x (the next comparison rejects it).
 * A trial that is done is frozen.  So r2 never increases, max_iter = 0 returns x0 and its residual, a non-finite start returns x0,
 * residual = inf, converged = 0, and a trial's outputs depend on that trial's inputs alone, bit for bit (not on its row, the batch, the
 * other trials of its tile or the stream).
 * x0 (B,dout); u (B,du) or NULL (du = d - dout); x (B,dout); residual (B) = sqrt(r2); n_iter (B), converged (B): int32; jac (B,dout,dout)
 * or NULL: J = I + A at the returned x, jac[b][i][j] = df_i/dx_j.  Asynchronous on `stream`, no host synchronisation, no scratch; reads
 * the state tensors, writes none.
 * -1 null tensor, -20 bad shape (also max_iter < 0, tol or lam0 not positive and finite), -21 u missing with d > dout, -11 dout > 32 or
 * the shape is beyond one workgroup's LDS: all before the first launch.
 * vjf_fixed_points_plan: the dynamic LDS of a workgroup for these sizes; -11 / -20 as the call. */
int vjf_fixed_points_plan(int32_t n, int32_t d, int32_t dout, int64_t* lds_bytes);
int vjf_fixed_points(const float* x0, const float* u, const float* centroid, const float* logwidth, const float* w_mean,
                     float* x, float* residual, int32_t* n_iter, int32_t* converged, float* jac,
                     int32_t B, int32_t n, int32_t d, int32_t dout, int32_t max_iter, float tol, float lam0, void* stream);
/* Smoothing: the extended Rauch-Tung-Striebel pass over a filtered sequence q(x_t | y_1..t) = N(mu_t, D_t), D_t = diag(exp(logvar_t)),
 * with the same mean map f(x, u) = x + Phi([x, u]) w_mean, J = I + A its Jacobian, and a scalar state-noise variance q = state_var,
 * the whole horizon as one call, fp32.  The transition from row t to row t + 1 uses u[t + 1] (u[0] is never read: the array that went
 * into the filter goes in unchanged).  Per trial:
 *   last row:  ms_{T-1} = mu_{T-1} (bit for bit),  Ps_{T-1} = D_{T-1};
 *   for t = T-2 .. 0, with g = g(mu_t, u_{t+1}), J = J(mu_t, u_{t+1}), sd = exp(logvar_t / 2):
 *     1. Jh = J diag(sd) / sqrt(q);
 *     2. M = I + Jh^T Jh = L L^T (Cholesky; eigenvalues >= 1 whatever logvar is);
 *     3. G = diag(sd) M^-1 Jh^T / sqrt(q)      (= D J^T (J D J^T + q I)^-1, the smoother gain);
 *     4. C = diag(sd) M^-1 diag(sd)            (= D - D J^T (J D J^T + q I)^-1 J D);
 *     5. ms_t = mu_t + G (ms_{t+1} - (mu_t + g));
 *     6. Ps_{t+1} = Ls Ls^T (Cholesky), K = G Ls, Ps_t = C + K K^T.
 * This is the information form of the textbook Ps_t = D + G (Ps_{t+1} - P^-) G^T: no difference of positive-definite matrices.
 * Carried between rows: ms and the lower triangle of Ps, in fp32.  With after_mean (B,dout) and after_cov (B,dout,dout; its lower
 * triangle is read) -- the smoothed moments of the row behind the last one -- row T-1 is smoothed like every other row, u has T + 1
 * rows and u[T] drives the step into the after-row: rows [k, T) first and rows [0, k) second with after = (mean[k], cov[k]) give the
 * bits of the undivided call.
 * mu, logvar (T,B,dout); u (T,B,du), with after_* (T+1,B,du), or NULL (du = d - dout); mean, var (T,B,dout): ms and the diagonal of Ps;
 * cov (T,B,dout,dout) or NULL: Ps written from its triangle -- exactly symmetric, its diagonal is var bit for bit; cov0 (B,dout,dout):
 * Ps_0, always written.  A trial with an input that is not finite at row t (mu, logvar, u, after_*), or with a pivot of a factor
 * that is not positive and finite (possible only through after_cov), has NaN in every output from that row back to row 0; its
 * outputs behind that row and every other trial keep their bits.  No loop bound depends on data.  A trial's outputs depend on that
 * trial's inputs alone, bit for bit (not on its row, the batch, the other trials of its tile or the stream).  Asynchronous on
 * `stream`, no host synchronisation, no scratch; reads the state tensors, writes none.
 * -1 null tensor, -20 bad shape (also T < 1, state_var not positive and finite, one of after_mean / after_cov without the other), -21 u
 * missing with d > dout (and a transition to take), -11 dout > 32 or the shape is beyond one workgroup's LDS (every dout <= 24 with
 * n <= 256 and du <= 8 fits): all before the first launch.
 * vjf_smooth_plan: the dynamic LDS of a workgroup for these sizes; -11 / -20 as the call. */
int vjf_smooth_plan(int32_t n, int32_t d, int32_t dout, int64_t* lds_bytes);
int vjf_smooth(const float* mu, const float* logvar, const float* u, const float* centroid, const float* logwidth,
               const float* w_mean, const float* after_mean, const float* after_cov, float* mean, float* var, float* cov,
               float* cov0, int32_t T, int32_t B, int32_t n, int32_t d, int32_t dout, float state_var, void* stream);
/* Posterior draws: S joint draws per trial from the smoothed posterior of a filtered sequence by backward sampling, the whole horizon as
 * one call, fp32.  Notation and inputs of vjf_smooth: f = x + g, J = I + A at (mu_t, u_{t+1}), sd = exp(logvar_t / 2), q = state_var; the
 * step from row t to row t + 1 uses u[t + 1].  noise z is standard normal, (S,T,B,dout).  Per trial and member s:
 *   last row:  x_{T-1} = mu_{T-1} + sd_{T-1} z_{T-1}   (one fused multiply-add);
 *   for t = T-2 .. 0, with g = g(mu_t, u_{t+1}), J = J(mu_t, u_{t+1}), sd = exp(logvar_t / 2):
 *     1. Jh = J diag(sd) / sqrt(q);
 *     2. M = I + Jh^T Jh = L L^T (Cholesky);
 *     3. G = diag(sd) M^-1 Jh^T / sqrt(q)                     (steps 1 to 3 are vjf_smooth's, the same arithmetic, once per trial);
 *     4. L^T w = z_t                                          (one back-substitution per member);
 *     5. x_t = (mu_t + G (x_{t+1} - (mu_t + g))) + sd w       (the mean sum in vjf_smooth's order, the noise term added last by one
 *                                                              fused multiply-add: with z = 0 the draw is vjf_smooth's mean, bit for bit).
 * sd L^-T z has covariance diag(sd) M^-1 diag(sd), the C of vjf_smooth, and x_t is affine in x_{t+1} (the linearisation point is mu_t, not
 * the draw), so the draws are exactly Gaussian: their row means are vjf_smooth's ms_t, their row covariances Ps_t and
 * Cov(x_t, x_{t+1}) = G_t Ps_{t+1}.  Carried between rows: x alone.  With after (S,B,dout) -- the draws of the row behind the last one --
 * row T-1 is drawn like every other row from z[:, T-1], u has T + 1 rows and u[T] drives the step into the after-row: rows [k, T) first
 * and rows [0, k) second with after = x[:, k] give the bits of the undivided call.
 * mu, logvar (T,B,dout); u (T,B,du), with after (T+1,B,du), or NULL (du = d - dout); noise, x (S,T,B,dout).  A trial with an input that
 * is not finite at row t (mu, logvar, u) has NaN in every member from that row back to row 0.  A member whose noise is NaN at row t,
 * component c, has NaN by propagation: components 0 .. c of row t (those the back-substitution reaches) and every component from row
 * t - 1 back; a non-finite after-row of a member likewise from row T-1 back.  The rows behind, the other members and every other trial
 * keep their bits.  No loop bound depends on data.  A member's draws depend on that trial's inputs and that member's noise alone, bit
 * for bit (not on S, its index, the members per workgroup, the trial's row, the batch, its tile-mates or the stream).  Asynchronous on
 * `stream`, no host synchronisation, no scratch; reads the state tensors, writes none.
 * -1 null tensor, -20 bad shape (also T < 1, S < 1, state_var not positive and finite), -21 u missing with d > dout (and a transition to
 * take), -11 dout > 32 or the shape is beyond one workgroup's LDS (every shape vjf_smooth accepts is accepted): all before the first
 * launch.
 * vjf_smooth_sample_plan: the members a workgroup carries (<= S; the launch has ceil(B / 16) x ceil(S / members) workgroups) and its
 * dynamic LDS for these sizes; either pointer may be NULL; -11 / -20 as the call. */
int vjf_smooth_sample_plan(int32_t n, int32_t d, int32_t dout, int32_t S, int32_t* members_per_workgroup, int64_t* lds_bytes);
int vjf_smooth_sample(const float* mu, const float* logvar, const float* u, const float* centroid, const float* logwidth,
                      const float* w_mean, const float* noise, const float* after, float* x,
                      int32_t T, int32_t S, int32_t B, int32_t n, int32_t d, int32_t dout, float state_var, void* stream);
/* Scoring predictions: the k-step-ahead prediction error of the mean map f(x, u) = x + Phi([x, u]) w_mean over a filtered record, the
 * whole record as one call, fp32 with fp64 totals.  mu (T,B,dout): the filtered means; y (T,B,dy) or NULL with the decoder dec_W
 * (dy,dout), dec_b (dy); u (T,B,du) or NULL (du = d - dout), the array that went into the filter: the transition from row t to row
 * t + 1 reads u[t + 1], u[0] is never read.  For every origin t and trial b:
 *   xh_0 = mu[t,b],  xh_j = xh_{j-1} + Phi([xh_{j-1}, u[t+j,b]]) w_mean  for j = 1 .. K;   horizon h is valid iff t + h <= T - 1.
 * Outputs, float64, horizon h = 0 .. K on the first axis, sums over the valid (t, b):
 *   sse_x (K+1,dout) = sum (xh_h - mu[t+h])^2, row 0 exactly 0;   base_x (K+1,dout) = sum (mu[t] - mu[t+h])^2, persistence;
 *   with y, poisson == 0:  sse_y (K+1,dy) = sum (xh_h dec_W^T + dec_b - y[t+h])^2 (row 0: the filter's own reconstruction error),
 *                          base_y the same with xh_0 in place of xh_h;
 *   with y, poisson != 0:  sse_y = sum (exp(ec) - y[t+h] ec), ec = min(eta, 10), eta = xh_h dec_W^T + dec_b (PoissonLikelihood.loss,
 *                          vjf/likelihood.py:60, without log y!, per output column), base_y the same for xh_0;
 *   pred (K,T,B,dout) float32 or NULL: pred[h-1,t,b] = xh_h where valid, NaN elsewhere.
 * The counts max(T - h, 0) B are the caller's arithmetic; a horizon beyond the record has sums exactly 0.
 * Summation order (the results have defined bits).  The record is handled flattened: start r = t B + b is compared at horizon h with
 * row r + h B and step j reads row r + j B of u.  Tile i holds the starts 16 i .. 16 i + 15 and may straddle origins.  Per tile,
 * horizon and column the valid starts' terms are added in start order in fp32, each term rounded on its own (the difference, its
 * square, then the sum: three roundings; Poisson: exp, the product, their difference, the sum) -- a partial in `scratch`; a second
 * kernel adds the tiles' partials in tile order in fp64.  No floating-point atomics.  So the bits do not depend on the stream, on
 * VJF_KS_CHUNK (tiles per chunk; default: partials within 32 MiB) or on the forms of the kernels (VJF_FC_CENTROID_LDS,
 * VJF_FC_LOOKAHEAD); they DO depend on the order of the trials.  pred of a start depends on that start's inputs alone and is, bit for
 * bit, vjf_forecast_seq from mu[t] with zero weight noise.  A start whose horizon has run out of record keeps stepping on the control
 * input it read last and is masked out.  Asynchronous on `stream`, no host synchronisation; reads the state tensors, writes none.
 * scratch: >= vjf_kstep_score_scratch_size bytes (dy = 0 without y), one call at a time per scratch.
 * -1 null tensor, -20 bad shape (also T < 1, K < 1, y without a decoder), -21 u missing with d > dout, -11 the shape is beyond one
 * workgroup's LDS (the message names the limit): all before the first launch.
 * vjf_kstep_score_plan: pure arithmetic, callable without a GPU: the dynamic LDS of a workgroup, the tiles of the record, the tiles
 * per chunk and the forms (bit 0 centroids in LDS, bit 1 w_mean's operands in registers, bit 2 decoder in LDS); any pointer may be
 * NULL; -11 / -20 as the call. */
int vjf_kstep_score_scratch_size(int32_t T, int32_t B, int32_t K, int32_t dout, int32_t dy, int64_t* bytes);
int vjf_kstep_score_plan(int32_t T, int32_t B, int32_t K, int32_t n, int32_t d, int32_t dout, int32_t dy, int64_t* lds_bytes,
                         int64_t* tiles, int64_t* tiles_per_chunk, int32_t* forms);
int vjf_kstep_score(const float* mu, const float* y, const float* u, const float* centroid, const float* logwidth,
                    const float* w_mean, const float* dec_W, const float* dec_b, double* sse_x, double* base_x, double* sse_y,
                    double* base_y, float* pred, void* scratch, int32_t T, int32_t B, int32_t K, int32_t n, int32_t d, int32_t dout,
                    int32_t dy, int32_t poisson, void* stream);
/* Extended Kalman filter and model evidence: the Bayesian filter of the learned generative model itself -- the mean map
 * f(x, u) = x + Phi([x, u]) w_mean with J = I + A its Jacobian, a scalar state-noise variance q = state_var, the linear decoder
 * y = C x + b (C = dec_W (dy,dout), b = dec_b) and a scalar Gaussian observation variance r = obs_var -- over a whole record as one
 * call, fp32 (replaces the per-step host loop of vjf/kalman.py:16-101).  u[t] drives the transition INTO row t, as in the filter;
 * row 0 is predicted from the prior with u[0].  Gc = C^T C / r is formed once per call.  Carried per trial: m and the lower triangle
 * of P.  Per row t:
 *   1. predict:  g, A at (m, u_t), J = I + A;  m^- = m + g;  Ls Ls^T = P (Cholesky);  K = J Ls;  P^- = K K^T + q I = Lp Lp^T;
 *   2. update:   M = I + Lp^T Gc Lp = Lm Lm^T (eigenvalues >= 1 whatever r and P^- are);  v = y - b - C m^-;  s = C^T v / r;
 *                Lm Y = Lp^T;  P = Y^T Y (= Lp M^-1 Lp^T);  m = m^- + P s;
 *   3. loglik[t] = -1/2 (dy log 2 pi + log det S + v^T S^-1 v),  S = C P^- C^T + r I,  through
 *                log det S = dy log r + 2 sum log diag(Lm),   v^T S^-1 v = |y - b - C m|^2 / r + |Lp^-1 (m - m^-)|^2
 *                (no dy x dy matrix, no difference of covariances, no subtraction of like terms);
 *   4. a row with observed[t,b] == 0: the update runs with Gc = 0 and v = 0, so M = I and P = Lp Lp^T = P^- exactly, m = m^- and
 *      loglik = 0 by per-trial selects; its y is never used in arithmetic and may hold anything (NaN included).
 * y (T,B,dy); u (T,B,du) or NULL (du = d - dout); observed uint8 (T,B) or NULL (every row observed); the prior of the row before
 * row 0: prior_mean (B,dout) with EITHER prior_logvar (B,dout), P = diag(exp(logvar)), OR prior_cov (B,dout,dout), its lower
 * triangle is read -- exactly one of the two is non-NULL.  mean, var (T,B,dout): m and the diagonal of P; cov (T,B,dout,dout) or
 * NULL: P written from its triangle -- exactly symmetric, its diagonal is var bit for bit; loglik (T,B); cov_last (B,dout,dout): P
 * of the last row, always written.  Rows [0, k) first and rows [k, T) second with prior_mean = mean[k-1], prior_cov = cov[k-1] give
 * the bits of the undivided call.  A trial with a non-finite m (the prior), u or observed y at row t, or with a pivot of a factor
 * that is not positive and finite, has NaN in mean, var, cov and loglik from that row ON; its rows before and every other trial keep
 * their bits.  No loop bound depends on data.  A trial's outputs depend on that trial's inputs alone, bit for bit (not on its row,
 * the batch, the other trials of its tile, the stream, or where the planner puts the centroids and the decoder:
 * VJF_FC_CENTROID_LDS, VJF_EKF_DECODER_LDS).  Asynchronous on `stream`, no host synchronisation, no scratch; reads the state
 * tensors, writes none.
 * -1 null tensor, -20 bad shape (also T < 1, dy < 1, state_var or obs_var not positive and finite, both or neither of prior_logvar /
 * prior_cov), -21 u missing with d > dout, -11 dout > 32 or the shape is beyond one workgroup's LDS (every dout <= 24 with n <= 256
 * and du <= 8 fits, whatever dy is): all before the first launch and before anything is written.
 * vjf_ekf_plan: pure arithmetic, callable without a GPU: the dynamic LDS of a workgroup for these sizes; -11 / -20 as the call. */
int vjf_ekf_plan(int32_t n, int32_t d, int32_t dout, int32_t dy, int64_t* lds_bytes);
int vjf_ekf(const float* y, const float* u, const uint8_t* observed, const float* centroid, const float* logwidth,
            const float* w_mean, const float* dec_W, const float* dec_b, const float* prior_mean, const float* prior_logvar,
            const float* prior_cov, float* mean, float* var, float* cov, float* loglik, float* cov_last, int32_t T, int32_t B,
            int32_t n, int32_t d, int32_t dout, int32_t dy, float state_var, float obs_var, void* stream);
/* Poisson filter and model evidence: the filter of the learned generative model with count observations -- the mean map
 * f(x, u) = x + Phi([x, u]) w_mean with J = I + A its Jacobian, a scalar state-noise variance q = state_var, the linear decoder
 * eta = C x + b (C = dec_W (dy,dout), b = dec_b) and y_j ~ Poisson(exp(eta_j)) -- over a whole record as one call, fp32.  The
 * posterior of each row is the Laplace approximation at the mode and the evidence is the Laplace evidence.  eta is NOT clamped
 * (the clamp(max=10) of the training loss, vjf/likelihood.py:60, is a guard of that loss and makes the objective non-convex); the
 * step control below keeps an overflowing rate out.  u[t] drives the transition INTO row t; row 0 is predicted from the prior
 * with u[0].  Carried per trial: m and the lower triangle of P.  Per row t:
 *   1. predict, exactly as vjf_ekf:  g, A at (m, u_t);  m^- = m + g;  Ls Ls^T = P;  K = (I + A) Ls;  P^- = K K^T + q I = Lp Lp^T;
 *   2. mode, in whitened coordinates x = m^- + Lp z:
 *        E(z):  eta = C x + b;  lam = exp(eta) (the accurate expf);  phi = sum_j (lam_j - y_j eta_j) + |z|^2 / 2;
 *        D(z):  H = sum_j lam_j c_j c_j^T;  M = I + Lp^T H Lp = Lm Lm^T (eigenvalues >= 1);  grad = z - Lp^T C^T (y - lam);
 *               dz = -M^-1 grad;
 *        start: z = 0, E, D, alpha = 1;  then exactly n_iter times:  z_c = z + alpha dz;  E(z_c);  accept = phi_c <= phi, false
 *        where phi_c is not finite;  where accepted z, phi, eta, lam become the candidate's;  D(z) runs for every trial; where
 *        accepted dz becomes the new direction and alpha = 1, elsewhere dz stays and alpha becomes alpha / 4.  Every decision is
 *        a per-trial select; no trip count depends on data.  The decision phi_c <= phi is taken on the difference formed term by
 *        term, sum_j (lam_j expm1(delta_j) - y_j delta_j) + z.d + |d|^2 / 2 with d = z_c - z and delta = C Lp d: in fp32 phi_c and phi
 *        rounded one by one agree in all their digits while z is still some 1e-3 from the mode, and their comparison is rounding;
 *   3. posterior:  m = m^- + Lp z;  Lm Y = Lp^T;  P = Y^T Y, with the Lm of the last D;
 *   4. loglik[t] = sum_j (y_j eta_j - lam_j - lgamma(y_j + 1)) - |z|^2 / 2 - sum log diag(Lm), the terms of the sum formed per
 *      count before they are added up (y eta and lgamma(y + 1) cancel there, not between two large sums);
 *   5. grad_norm[t] = |grad| of the last D: the caller sees from it whether n_iter was enough;
 *   6. a row with observed[t,b] == 0: H = 0 and y - lam = 0 by selects (and the terms of phi), so M = I, z stays 0, P = P^-,
 *      m = m^-, and loglik = grad_norm = 0; its y never enters arithmetic and may hold anything (NaN included);
 *   7. poison: a trial has NaN in mean, var, cov, loglik and grad_norm from row t ON when at that row m, u or an observed y is
 *      not finite, an observed y < 0, phi at z = 0 is not finite, a pivot of a factor (Ls, Lp, any Lm) is not positive and
 *      finite, or loglik is not finite.  Its rows before and every other trial keep their bits.  y >= 0 need not be an integer.
 * y (T,B,dy); u (T,B,du) or NULL (du = d - dout); observed uint8 (T,B) or NULL (every row observed); the prior of the row before
 * row 0: prior_mean (B,dout) with EITHER prior_logvar (B,dout) OR prior_cov (B,dout,dout), its lower triangle is read -- exactly
 * one of the two is non-NULL.  mean, var (T,B,dout); cov (T,B,dout,dout) or NULL: exactly symmetric, its diagonal is var bit for
 * bit; loglik, grad_norm (T,B); cov_last (B,dout,dout): P of the last row, always written.  Rows [0, k) first and rows [k, T)
 * second with prior_mean = mean[k-1], prior_cov = cov[k-1] give the bits of the undivided call.  A trial's outputs depend on that
 * trial's inputs alone, bit for bit (not on its row, the batch, the other trials of its tile, the stream, or where the planner
 * puts the centroids and the decoder: VJF_FC_CENTROID_LDS, VJF_LAPLACE_DECODER_LDS).  Asynchronous on `stream`, no host
 * synchronisation, no scratch; reads the state tensors, writes none.
 * -1 null tensor, -20 bad shape (also T < 1, dy < 1, n_iter < 1 or n_iter > 64, state_var not positive and finite, both or
 * neither of prior_logvar / prior_cov), -21 u missing with d > dout, -11 dout > 24 or the shape is beyond one workgroup's LDS
 * (every dout <= 16 with n <= 256 and du <= 8 fits, whatever dy is): all before the first launch and before anything is written.
 * vjf_laplace_filter_plan: pure arithmetic, callable without a GPU: the dynamic LDS of a workgroup; -11 / -20 as the call. */
int vjf_laplace_filter_plan(int32_t n, int32_t d, int32_t dout, int32_t dy, int64_t* lds_bytes);
int vjf_laplace_filter(const float* y, const float* u, const uint8_t* observed, const float* centroid, const float* logwidth,
                       const float* w_mean, const float* dec_W, const float* dec_b, const float* prior_mean,
                       const float* prior_logvar, const float* prior_cov, float* mean, float* var, float* cov, float* loglik,
                       float* grad_norm, float* cov_last, int32_t T, int32_t B, int32_t n, int32_t d, int32_t dout, int32_t dy,
                       int32_t n_iter, float state_var, void* stream);
/* LinearRegression.rls (vjf/module.py:79-112), in place on w_mean/w_chol/w_precision/w_pchol.
 * v: device scalar.  scratch: >= vjf_rls_scratch_size(B,n,dout) bytes.  status: device uint32
 * (0 ok, VJF_STATUS_RLS_FAILED when the state was left unchanged). */
int vjf_rls_scratch_size(int32_t B, int32_t n, int32_t dout, int64_t* bytes);
int vjf_blr_rls(const float* x, const float* target, const float* v, float shrink, const float* centroid,
                const float* logwidth, float* w_mean, float* w_chol, float* w_precision, float* w_pchol,
                void* scratch, uint32_t* status, int32_t B, int32_t n, int32_t d, int32_t dout, void* stream);

/* LinearRegression.kalman (vjf/module.py:114-142 over vjf/kalman.py:15-50, 102-145), A = I, Q = diffusion I, R = v I, in
 * n x n algebra on the Gram statistics: the reference's (samples x samples) innovation covariance is never formed (its
 * update -- S^-1 enters the gain twice, kalman.py:134-135 -- is reproduced as it is).  w_mean (n, dout) and w_chol (n, n) in
 * place; w_chol leaves as the lower Cholesky factor of the covariance.  status[0] (device, may
 * be NULL): 0 or VJF_STATUS_RLS_FAILED (state untouched). */
int vjf_kalman_scratch_size(int32_t B, int32_t n, int32_t dout, int64_t* bytes);
int vjf_blr_kalman(const float* x, const float* target, const float* v, float diffusion, const float* centroid,
                   const float* logwidth, float* w_mean, float* w_chol, void* scratch, uint32_t* status, int32_t B,
                   int32_t n, int32_t d, int32_t dout, void* stream);
/* Recognition.forward (vjf/recognition.py:31-42). Wb: pointers to layer weights/biases on device. */
int vjf_recognition_forward(const float* y, const float* u, const float* mu_s, const float* lv_s,
                            const float* const* rec_W, const float* const* rec_b, const float* mean_W,
                            const float* lv_W, const float* lv_b, float* mu_t, float* lv_t, int32_t B,
                            int32_t ydim, int32_t udim, int32_t xdim, int32_t n_hidden,
                            const int32_t* hidden, void* stream);
/* Recognition.forward with an activation (vjf_recognition_forward is the VJF_ACT_TANH case).  Invalid kinds or parameters: < 0. */
int vjf_recognition_forward_act(const float* y, const float* u, const float* mu_s, const float* lv_s,
                                const float* const* rec_W, const float* const* rec_b, const float* mean_W,
                                const float* lv_W, const float* lv_b, float* mu_t, float* lv_t, int32_t B,
                                int32_t ydim, int32_t udim, int32_t xdim, int32_t n_hidden,
                                const int32_t* hidden, const vjf_activation* act, void* stream);
/* functional.gaussian_loss (vjf/functional.py:32-75): lv1/lv2 NULL for point arguments;
 * logvar: device scalar; out: device scalar. */
int vjf_gaussian_loss(const float* m1, const float* lv1, const float* m2, const float* lv2,
                      const float* logvar, float* out, int32_t B, int32_t d, void* stream);
/* functional.gaussian_entropy (vjf/functional.py:25-29). */
int vjf_gaussian_entropy(const float* lv, float* out, int32_t B, int32_t d, void* stream);
/* PoissonLikelihood.loss (vjf/likelihood.py:51-62). */
int vjf_poisson_loss(const float* eta, const float* target, float* out, int32_t B, int32_t d, void* stream);
/* LinearDecoder.forward, Tensor branch (vjf/model.py:28-30): out(B,ydim) = x @ W^T + b. */
int vjf_linear_forward(const float* x, const float* W, const float* b, float* out, int32_t B, int32_t din,
                       int32_t dout, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VJF_HIP_H */
