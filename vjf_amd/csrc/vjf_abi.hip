// vjf_abi.hip -- extern "C" entry points declared in include/vjf_hip.h, no kernel and no launch (those: its vjf_host_*.h).  gfx950 only.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <dlfcn.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <atomic>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/vjf_hip.h"
#include "vjf_chol_blocks.h"
#include "vjf_chol_kernel.h"
#include "vjf_gram_kernel.h"
#include "vjf_handoff.h"
#include "vjf_mega_kernel.h"
#include "vjf_ops_kernels.h"
#include "vjf_plan.h"
#include "vjf_post_kernel.h"
#include "vjf_rls_operands.h"
#include "vjf_rlsb_kernels.h"
#include "vjf_serial_kernel.h"
#include "vjf_trial_kernel.h"
#include "vjf_trial_mfma_kernel.h"
#include "vjf_trial_wide.h"

#include "vjf_host_ctx.h"
#include "vjf_host_launch.h"
#include "vjf_host_routes.h"
#include "vjf_host_ops.h"
#include "vjf_host_forecast.h"
#include "vjf_host_tangent.h"
#include "vjf_host_fixed_point.h"
#include "vjf_host_smooth.h"
#include "vjf_host_smooth_sample.h"
#include "vjf_host_kstep.h"
#include "vjf_host_ekf.h"
#include "vjf_host_laplace.h"

#ifdef VJF_CHAOS
// diagnostic build: which workgroups are held, and where (vjf_handoff.h), from the environment at every entry
static void chaos_refresh(const vjf_ctx* c) {
    const int range[6] = {getenv("VJF_CHAOS_LO") ? atoi(getenv("VJF_CHAOS_LO")) : 0, getenv("VJF_CHAOS_HI") ? atoi(getenv("VJF_CHAOS_HI")) : 1 << 30,
                          getenv("VJF_CHAOS_SITE") ? atoi(getenv("VJF_CHAOS_SITE")) : -1, getenv("VJF_CHAOS_KIND") ? atoi(getenv("VJF_CHAOS_KIND")) : 0,
                          getenv("VJF_CHAOS_TICKS") && atoi(getenv("VJF_CHAOS_TICKS")) > 0 ? atoi(getenv("VJF_CHAOS_TICKS")) : 20000,
                          getenv("VJF_CHAOS_MASK") ? atoi(getenv("VJF_CHAOS_MASK")) : 7};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(vjf_chaos_range), range, sizeof(range));
    const unsigned* base = c->mega_counters(c->mega_launches);   // (the block the next launch counts in)
    (void)hipMemcpyToSymbol(HIP_SYMBOL(vjf_chaos_base), &base, sizeof(base));
}
#define VJF_CHAOS_REFRESH(c) chaos_refresh(c)
#else
#define VJF_CHAOS_REFRESH(c) ((void)0)
#endif

extern "C" {

int vjf_abi_version(void) { return VJF_ABI_VERSION; }
const char* vjf_last_error(void) { return g_err.c_str(); }

int vjf_state_size(const vjf_config* cfg, int64_t* n_floats) {
    VjfPlan P;
    if (int rc = plan_for("vjf_state_size", cfg, &P)) return rc;
    if (!n_floats) return fail(-1, "vjf_state_size: null output");
    *n_floats = P.n_state;
    return 0;
}

int vjf_state_layout(const vjf_config* cfg, int64_t* offsets, int64_t* sizes) {
    VjfPlan P;
    if (int rc = plan_for("vjf_state_layout", cfg, &P)) return rc;
    if (!offsets || !sizes) return fail(-1, "vjf_state_layout: null output");
    for (int s = 0; s < VJF_N_SLOTS; ++s) { offsets[s] = P.off[s]; sizes[s] = P.size[s]; }
    return 0;
}

int vjf_workspace_size(const vjf_config* cfg, int64_t* bytes) {
    VjfPlan P;
    if (int rc = plan_for("vjf_workspace_size", cfg, &P)) return rc;
    if (!bytes) return fail(-1, "vjf_workspace_size: null output");
    if (cfg->max_batch < 1) return fail(-7, "vjf_workspace_size: max_batch must be >= 1");
    std::vector<VjfJob> jobs;
    build_jobs(P, jobs);
    *bytes = (int64_t)carve_ws(P, cfg->max_batch, (int)jobs.size()).total;
    return 0;
}

int vjf_mega_grad_tile_table(const vjf_config* cfg, int32_t* table, int32_t capacity, int32_t* n_words) {
    VjfPlan P;
    if (int rc = plan_for("vjf_mega_grad_tile_table", cfg, &P)) return rc;
    const int words = vjf_mega_grad_tiles(P, nullptr);
    if (n_words) *n_words = words;
    if (!table) return 0;
    if (capacity < words) return fail(-7, "vjf_mega_grad_tile_table: capacity %d < %d words", (int)capacity, words);
    vjf_mega_grad_tiles(P, table);
    return 0;
}

int vjf_ctx_create(const vjf_config* cfg, float* state, void* workspace, int64_t workspace_bytes, void* stream,
                   vjf_ctx** out) {
    if (!cfg || !state || !workspace || !out) return fail(-1, "vjf_ctx_create: null argument");
    VjfPlan P;
    if (int rc = plan_for("vjf_ctx_create", cfg, &P)) return rc;
    if (cfg->max_batch < 1) return fail(-7, "vjf_ctx_create: max_batch must be >= 1");
    std::vector<VjfJob> jobs;
    build_jobs(P, jobs);
    if ((int)jobs.size() > VJF_MAX_JOBS) return fail(-8, "vjf_ctx_create: %zu Gram tiles exceed the limit", jobs.size());
    Carve cv = carve_ws(P, cfg->max_batch, (int)jobs.size());
    if ((int64_t)cv.total > workspace_bytes)
        return fail(-9, "vjf_ctx_create: workspace too small (%lld < %zu bytes)", (long long)workspace_bytes, cv.total);
    const size_t lds_k2 = vjf_serial_lds_floats(P) * 4;
    const bool fast_chol = vjf_chol_lds_ok(P);
    if (!fast_chol && lds_k2 > kMaxLds - 1024 && P.n <= 32 * VJF_CHOL_MAXBLK)
        return fail(-11, "vjf_ctx_create: n_rbf=%d too large for the single-workgroup RLS kernel", P.n);
    VJF_HIP(hipSetDevice(cfg->device));
    vjf_ctx* c = new (std::nothrow) vjf_ctx();
    if (!c) return fail(-12, "vjf_ctx_create: out of host memory");
    c->cfg = *cfg; c->plan = P; c->state = state; c->ws = (char*)workspace; c->ws_bytes = workspace_bytes;
    c->stream = (hipStream_t)stream; c->cv = cv; c->njobs = (int)jobs.size();
    c->lds_k2 = lds_k2;
    c->fast_chol = fast_chol;
    c->lds_post = vjf_post_lds_bytes(P);
    c->post_kernels = fast_chol && P.dz <= 16 && c->lds_post <= kMaxLds - 1024;
    // the single-workgroup chain kernels ask for the whole LDS of their compute unit: nothing else (every other kernel of
    // a step uses some LDS) is then placed beside them to share their SIMDs' issue slots and matrix cores
    c->lds_chol = fast_chol ? kMaxLds - 256 : vjf_chol_lds_bytes(P);
    if (c->post_kernels) c->lds_post = kMaxLds - 256;
    c->lds_k1m = vjf_trial_mfma_lds_floats(P) * 4;
    c->mfma_trial = c->lds_k1m <= kMaxLds - 1024;
    for (const VjfJob& j : jobs) c->n_ejobs += j.kind == 0;
    // the one-launch route's hand-offs: the producer stores write-through (sc1), every storing wavefront drains vmcnt, the workgroup
    // barrier, ONE lane's agent-scope add; the consumer polls that count with one lane (an sc1 load), the workgroup barrier, and then
    // EVERY load of a handed-off byte is an sc1 load (4- or 16-byte, global_ / buffer_, never flat_), one workgroup per compute unit,
    // hipMalloc memory: the first row of the MI355X guide's table "hand-offs measured with sc1 loads in place of the acquire", in every
    // cell.  That form is the default.  VJF_HANDOFF_ACQUIRE=1 adds an agent-scope acquire (L1 invalidate, ~1.7 us the polling
    // wavefront waits for) behind every wait -- the form with an architectural guarantee, ~2.5 % slower at config B; the perturbed-
    // timing test (tests/test_gpu_handoffs.py) runs in both.
    { const char* ha = getenv("VJF_HANDOFF_ACQUIRE"); c->handoff_acquire = ha && atoi(ha) != 0; }
    c->mega_ok = c->mega_plan = mega_plan_ok(P);
    VJF_HIP(hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, cfg->device));
    if (const char* ce = getenv("VJF_COLLECTIVES")) { if (atoi(ce) == 1) c->collectives = 1; }
    hipError_t e = hipMemcpyAsync(c->jobs(), jobs.data(), jobs.size() * sizeof(VjfJob), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->red(), 0, (size_t)P.red_len * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->red_rls(0), 0, (size_t)P.red_len * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->red_rls(1), 0, (size_t)P.red_len * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->flag_words(), 0, 256, c->stream);
    SlabTables tb;
    std::vector<int> gtab;
    if (c->mega_ok) {
        const VjfMegaTrialLds Lo = vjf_mega_trial_lds(P, (int)(kMegaLds / 4) - 8);
        tb = slab_tables(P, Lo, vjf_mega_slab_layout(P));
        if (e == hipSuccess) e = hipMemcpyAsync(c->mg_pidx(), tb.pidx.data(), tb.pidx.size() * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c->mg_cidx(), tb.cidx.data(), tb.cidx.size() * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c->mg_grp(), tb.grp.data(), tb.grp.size() * 4, hipMemcpyHostToDevice, c->stream);
        gtab.resize((size_t)vjf_mega_grad_tiles(P, nullptr));
        vjf_mega_grad_tiles(P, gtab.data());
        if (e == hipSuccess) e = hipMemcpyAsync(c->mg_gtab(), gtab.data(), gtab.size() * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->mg_img(), 0, (size_t)Lo.th_len * 4, c->stream);   // (its padding stays 0)
        if (e == hipSuccess) e = hipMemsetAsync(c->mega_counters(0), 0, (size_t)2 * MG_C_WORDS * 4, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // `jobs`, `tb`, `gtab` (host) must outlive the copies
    if (e != hipSuccess) { delete c; return fail(-100, "vjf_ctx_create: %s", hipGetErrorString(e)); }
    allow_lds(vjf_serial_kernel, c->lds_k2);
    allow_lds(vjf_rls_post_kernel, c->lds_post);
    allow_lds(vjf_prepg_kernel, vjf_prepg_lds_bytes(P));
    if (c->mfma_trial) allow_lds(vjf_trial_mfma_kernel<>, c->lds_k1m);
    allow_lds(chol_kernels(P.dz).chol, c->lds_chol);        // (the instantiations this context launches)
    if (P.dz <= 16) allow_lds(chol_kernels(P.dz).pair, c->lds_chol);
    mega_residency(c);
    if (DevShared* d = dev_shared(cfg->device)) {
        std::lock_guard<std::mutex> lk(d->mu);
        if (!d->mirror_h) {
            unsigned* h = nullptr; unsigned* dp = nullptr;
            if (hipHostMalloc((void**)&h, VJF_MIRROR_WORDS * sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
                hipHostGetDevicePointer((void**)&dp, h, 0) == hipSuccess) {
                memset(h, 0, VJF_MIRROR_WORDS * sizeof(unsigned));
                d->mirror_h = h; d->mirror_d = dp;
            }
            (void)hipGetLastError();                                // (without the page: no early notice, the status word still tells)
        }
        count_mega(c, d);
    }
    *out = c;
    return 0;
}

int vjf_ctx_destroy(vjf_ctx* ctx) {
    if (!ctx) return 0;
    if (DevShared* d = dev_shared(ctx->cfg.device)) {
        std::lock_guard<std::mutex> lk(d->mu);
        if (ctx->mega_counted && d->mega_ctxs > 0) --d->mega_ctxs;
    }
    if (ctx->comm_a) {
        if (ctx->stream2) { (void)hipStreamSynchronize(ctx->stream2); (void)hipStreamSynchronize(ctx->stream3); }
        (void)hipStreamSynchronize(ctx->stream);
        (void)nccl().comm_destroy(ctx->comm_a); (void)nccl().comm_destroy(ctx->comm_b);
        ctx->comm_a = ctx->comm_b = nullptr;
    }
    if (ctx->stream2) {
        (void)hipStreamSynchronize(ctx->stream2); (void)hipStreamSynchronize(ctx->stream3);
        (void)hipEventDestroy(ctx->ev_s); (void)hipEventDestroy(ctx->ev_c);
        for (int i = 0; i < 2; ++i) { (void)hipEventDestroy(ctx->ev_f[i]); (void)hipEventDestroy(ctx->ev_r[i]); (void)hipEventDestroy(ctx->ev_b[i]); (void)hipEventDestroy(ctx->ev_g[i]); }
        (void)hipStreamDestroy(ctx->stream2); (void)hipStreamDestroy(ctx->stream3);
    }
    delete ctx;
    return 0;
}

int vjf_set_overlap(vjf_ctx* ctx, int enable) {
    if (!ctx) return fail(-1, "vjf_set_overlap: null context");
    ctx->overlap = enable != 0;
    ctx->force_streams = enable == 3;
    return ctx->overlap ? (ctx->force_streams ? 3 : 1) : 0;
}

int vjf_comm_unique_id(void* ids256) {
    if (!ids256) return fail(-1, "vjf_comm_unique_id: null output");
    if (!nccl().ok) return fail(-111, "vjf_comm_unique_id: RCCL is not available in this process");
    VJF_NCCL(nccl().get_unique_id((VjfNcclId*)ids256));
    VJF_NCCL(nccl().get_unique_id((VjfNcclId*)ids256 + 1));
    return 0;
}

int vjf_comm_init(vjf_ctx* ctx, const void* ids256, int32_t rank, int32_t world) {
    if (!ctx || !ids256) return fail(-1, "vjf_comm_init: null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(-20, "vjf_comm_init: rank %d of %d", rank, world);
    if (!nccl().ok) return fail(-111, "vjf_comm_init: RCCL is not available in this process");
    if (ctx->comm_a) return fail(-112, "vjf_comm_init: the context already has communicators");
    if (ctx->collectives != 1 && !(ctx->fast_chol && ctx->post_kernels && ctx->mfma_trial))
        return fail(-113, "vjf_comm_init: this plan has no multi-stream route; keep the all-reduce on the caller's side (vjf_filter_local / vjf_filter_global)");
    VJF_HIP(hipSetDevice(ctx->cfg.device));
    VjfNcclId ids[2];
    memcpy(ids, ids256, sizeof ids);
    void* ca = nullptr; void* cb = nullptr;
    VJF_NCCL(nccl().comm_init_rank(&ca, world, ids[0], rank));
    int e = nccl().comm_init_rank(&cb, world, ids[1], rank);
    if (e != 0) { (void)nccl().comm_destroy(ca); return fail(-110, "ncclCommInitRank failed: %s", nccl().err ? nccl().err(e) : "rccl error"); }
    ctx->comm_a = ca; ctx->comm_b = cb; ctx->world = world;
    ctx->fake_world = 1;
    if (const char* fw = getenv("VJF_DEBUG_FAKE_WORLD")) { const int k = atoi(fw); if (world == 1 && k > 1 && k <= 64) ctx->fake_world = k; }
    return 0;
}

int vjf_comm_ranks(vjf_ctx* ctx, int32_t* ranks2) {
    if (!ctx || !ranks2) return fail(-1, "vjf_comm_ranks: null argument");
    ranks2[0] = ranks2[1] = 0;
    if (!ctx->comm_a) return 0;
    if (!nccl().comm_count) return fail(-111, "vjf_comm_ranks: ncclCommCount is not available in this process");
    int na = 0, nb = 0;
    VJF_NCCL(nccl().comm_count(ctx->comm_a, &na));
    VJF_NCCL(nccl().comm_count(ctx->comm_b, &nb));
    ranks2[0] = na; ranks2[1] = nb;
    return 0;
}

int vjf_set_collectives(vjf_ctx* ctx, int32_t per_step) {
    if (!ctx) return fail(-1, "vjf_set_collectives: null context");
    if (per_step != 1 && per_step != 2) return fail(-20, "vjf_set_collectives: %d (1 or 2)", per_step);
    ctx->collectives = per_step;
    return 0;
}

int vjf_set_stream(vjf_ctx* ctx, void* stream) {
    if (!ctx) return fail(-1, "vjf_set_stream: null context");
    ctx->stream = (hipStream_t)stream;
    return 0;
}

int vjf_get_status(vjf_ctx* ctx, uint32_t* status) {
    if (!ctx || !status) return fail(-1, "vjf_get_status: null argument");
    float* p = ctx->status_word();
    float v = 0.f;
    VJF_HIP(hipMemcpyAsync(&v, p, 4, hipMemcpyDeviceToHost, ctx->stream));
    VJF_HIP(hipMemsetAsync(p, 0, 4, ctx->stream));
    VJF_HIP(hipStreamSynchronize(ctx->stream));
    *status = (uint32_t)v;
    if (*status & VJF_STATUS_WAIT_MASK) {
        if (ctx->on_mega) ctx->mega_ok = false;                    // (see refuse_if_poisoned)
        if (DevShared* d = dev_shared(ctx->cfg.device))
            if (d->mirror_h) __atomic_store_n(d->mirror_h + VJF_MIRROR_SLOT(p), 0u, __ATOMIC_RELAXED);   // acknowledged
    }
    return 0;
}

int vjf_debug_stamps(vjf_ctx* ctx, int enable, uint64_t* out32) {
    if (!ctx) return fail(-1, "vjf_debug_stamps: null context");
    const char* src = nullptr;                               // the 256 bytes to hand out
    if (enable >= 128) {                                     // 128 + k: the one-launch route's role stamps of step k % 32 (32 words);
        const size_t at = enable >= 256 ? (size_t)32 * 256 + (size_t)((enable - 256) % (kMegaMaxTrialWg / 4)) * 256 : (size_t)((enable - 128) & 31) * 256;
        if (ctx->mega_ok) src = (char*)ctx->mega_stamps() + at;   // 256 + j: the last step's 8 words of trial workgroups 4 j .. 4 j + 3
    } else if (enable >= 64) {                               // 64 + k: 256-byte chunk k of the trial kernel's per-workgroup partials (even steps)
        src = (char*)ctx->partial() + (size_t)(enable - 64) * 256;
    } else if (enable >= 16) {                               // 16 + k: ring entry k (steps with epoch % 8 == k), mode unchanged
        src = (char*)ctx->step_stamps() + (enable - 16) % 10 * 256;
    } else {
        ctx->stamps = enable != 0;
        ctx->stamps_keep_overlap = enable == 2;
        src = (char*)ctx->step_stamps();
    }
    if (out32 && src) {
        VJF_HIP(hipMemcpyAsync(out32, src, 256, hipMemcpyDeviceToHost, ctx->stream));
        VJF_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

int vjf_reduce_buffer(vjf_ctx* ctx, float** ptr, int64_t* n_floats) {
    if (!ctx || !ptr || !n_floats) return fail(-1, "vjf_reduce_buffer: null argument");
    *ptr = ctx->red();
    *n_floats = ctx->plan.red_len;
    return 0;
}

int vjf_filter_local(vjf_ctx* c, int32_t B, const float* y, const float* u, const float* mu_s, const float* lv_s,
                     const float* eps_s, const float* eps_t, float* mu_t, float* lv_t, uint32_t flags) {
    if (!c) return fail(-1, "vjf_filter_local: null context");
    c->ran = true;
    DeviceGuard on_device(c->cfg.device);                   // (every launch below goes to the context's device, whatever is current)
    VJF_CHAOS_REFRESH(c);
    if (int rp = refuse_if_poisoned(c, "vjf_filter_local")) return rp;
    return launch_local(c, SeqView::one_step(B, y, u, mu_s, lv_s, eps_s, eps_t, mu_t, lv_t), flags, false);
}

int vjf_filter_global(vjf_ctx* c, int32_t B_total, float* loss4, uint32_t flags) {
    if (!c) return fail(-1, "vjf_filter_global: null context");
    c->ran = true;
    DeviceGuard on_device(c->cfg.device);                   // (every launch below goes to the context's device, whatever is current)
    VJF_CHAOS_REFRESH(c);
    if (B_total < 1) return fail(-20, "vjf_filter_global: B_total=%d", B_total);
    return filter_global_impl(c, B_total, loss4, flags, nullptr);   // (the caller's ranks hold shards: no replay, see vjf_hip.h)
}

int vjf_filter_step(vjf_ctx* c, int32_t B, const float* y, const float* u, const float* mu_s, const float* lv_s,
                    const float* eps_s, const float* eps_t, float* mu_t, float* lv_t, float* loss4, uint32_t flags) {
    if (!c) return fail(-1, "vjf_filter_step: null context");
    c->ran = true;
    DeviceGuard on_device(c->cfg.device);                   // (every launch below goes to the context's device, whatever is current)
    VJF_CHAOS_REFRESH(c);
    if (int rp = refuse_if_poisoned(c, "vjf_filter_step")) return rp;
    const VjfTrialArgs step = SeqView::one_step(B, y, u, mu_s, lv_s, eps_s, eps_t, mu_t, lv_t);
    if (pick_route(c, flags, 1) == kRouteMega) {
        const size_t sz = (size_t)B * c->plan.dz;
        const float* eps = eps_s;
        if (!(eps_s && eps_t && eps_t == eps_s + sz)) {                    // (the sequence layout of eps: (2, B, dz))
            // the two draws are separate tensors: the sequence entry point wants them adjacent -- stage them in the workspace
            int rc = check_step_args(c, step);
            if (rc) return rc;
            float* st = c->DEL();                                          // (B, ldD >= 2 dz) floats, unused by this route
            VJF_HIP(hipMemcpyAsync(st, eps_s, sz * 4, hipMemcpyDeviceToDevice, c->stream));
            VJF_HIP(hipMemcpyAsync(st + sz, eps_t, sz * 4, hipMemcpyDeviceToDevice, c->stream));
            eps = st;
        }
        const int rc = filter_seq_mega(c, 1, seq_view(c, B, y, u, eps, mu_s, lv_s, mu_t, lv_t, loss4), flags);
        if (rc != kMegaRefused) return rc;
    }
    int rc = vjf_filter_local(c, B, y, u, mu_s, lv_s, eps_s, eps_t, mu_t, lv_t, flags);
    if (rc) return rc;
    const VjfTrialArgs ta = trial_args(c, step, flags);
    return filter_global_impl(c, B, loss4, flags, c->world > 1 ? nullptr : &ta);
}

int vjf_set_activation(vjf_ctx* ctx, const vjf_activation* act) {
    VjfAct f{};
    if (int rc = act_check(act, "vjf_set_activation", &f)) return rc;   // (the arguments first: no device call before them)
    if (!ctx) return fail(-1, "vjf_set_activation: null context");
    if (ctx->ran) return fail(-32, "vjf_set_activation: the context has already run a vjf_filter_* call");
    DeviceGuard on_device(ctx->cfg.device);
    ctx->act = f;
    if (ctx->mfma_trial) with_trial_kernel(f, [&](auto kernel, auto...) { allow_lds(kernel, ctx->lds_k1m); });
    mega_residency(ctx);                                    // (the residency check again, on the kernels the context will now launch)
    if (DevShared* d = dev_shared(ctx->cfg.device)) {
        std::lock_guard<std::mutex> lk(d->mu);
        count_mega(ctx, d);
    }
    return 0;
}

int vjf_route(vjf_ctx* c, uint32_t flags) {
    if (!c) return fail(-1, "vjf_route: null context");
    return pick_route(c, flags, kRouteOfASequence);
}

int vjf_filter_seq(vjf_ctx* c, int32_t T, int32_t B, const float* y, const float* u, const float* eps, const float* mu0,
                   const float* lv0, float* mu, float* lv, float* loss, uint32_t flags) {
    if (!c) return fail(-1, "vjf_filter_seq: null context");
    c->ran = true;
    DeviceGuard on_device(c->cfg.device);                   // (every launch below goes to the context's device, whatever is current)
    VJF_CHAOS_REFRESH(c);
    if (T < 1) return fail(-23, "vjf_filter_seq: T=%d", T);
    if (int rp = refuse_if_poisoned(c, "vjf_filter_seq")) return rp;
    if (!y || !eps || !mu || !lv) return fail(-1, "vjf_filter_seq: null tensor");
    const SeqView s = seq_view(c, B, y, u, eps, mu0, lv0, mu, lv, loss);
    const Route route = pick_route(c, flags, T);
    switch (route) {
        case kRoutePacked: return filter_seq_steps(c, T, s, flags, true);
        case kRouteTwo: return filter_seq_two(c, T, s, flags);
        case kRouteMega: case kRouteStreams: {
            const bool streams = route == kRouteStreams;
            const int32_t chunk = seq_chunk();
            for (int32_t t0 = 0; t0 < T; t0 += chunk) {
                int32_t n = T - t0 < chunk ? T - t0 : chunk;
                if (streams && T - t0 - n == 1) n += 1;                    // (no chunk of a single step on the three-stream route)
                const SeqView r = s.from(t0);
                const int rc = streams ? filter_seq_streams(c, n, r, flags) : filter_seq_mega(c, n, r, flags);
                if (rc == kMegaRefused)                                    // (the context has left the one-launch route: the rest per step)
                    return vjf_filter_seq(c, T - t0, B, r.y, r.u, r.eps, r.mu0, r.lv0, r.mu, r.lv, r.loss, flags);
                if (rc) return rc;
                if (n > chunk) break;
            }
            return 0;
        }
        case kRoutePerStep: break;
    }
    if (c->world > 1)
        return fail(-24, "vjf_filter_seq: with communicators only the multi-stream schedule exists (update, no warm-up, T > 1, "
                         "fast kernels); use vjf_filter_local / vjf_filter_global around your own all-reduce otherwise");
    return filter_seq_steps(c, T, s, flags, false);
}

// ---- stand-alone operators: argument checks, then one call (vjf_host_ops.h, vjf_host_forecast.h)

int vjf_rbf_forward(const float* x, const float* centroid, const float* logwidth, float* out, int32_t B, int32_t n, int32_t d,
                    void* stream) {
    if (!x || !centroid || !logwidth || !out) return fail(-1, "vjf_rbf_forward: null tensor");
    if (B < 1 || n < 1 || d < 1) return fail(-20, "vjf_rbf_forward: bad shape");
    return launch_rbf(x, centroid, logwidth, out, B, n, d, (hipStream_t)stream);
}

int vjf_blr_predict(const float* x, const float* centroid, const float* logwidth, const float* w_mean, const float* w_chol,
                    float* mean, float* logvar, int32_t B, int32_t n, int32_t d, int32_t dout, void* stream) {
    if (!x || !centroid || !logwidth || !w_mean || !w_chol) return fail(-1, "vjf_blr_predict: null tensor");
    if (B < 1 || n < 1 || d < 1 || dout < 1) return fail(-20, "vjf_blr_predict: bad shape");
    return launch_predict("vjf_blr_predict", VjfPredArgs{x, centroid, logwidth, w_mean, w_chol, mean, logvar, B, n, d, dout}, (hipStream_t)stream);
}

int vjf_blr_sample(const float* x, const float* centroid, const float* logwidth, const float* w_mean, const float* w_chol,
                   const float* noise, float* out, float* w_scratch, int32_t B, int32_t n, int32_t d, int32_t dout, void* stream) {
    if (!x || !centroid || !logwidth || !w_mean || !w_chol || !noise || !out || !w_scratch) return fail(-1, "vjf_blr_sample: null tensor");
    if (B < 1 || n < 1 || d < 1 || dout < 1) return fail(-20, "vjf_blr_sample: bad shape");
    VjfWideGemm g{};                                       // w = w_mean + w_chol @ noise   (module.py:71)
    g.A = w_chol; g.lda = n; g.Bm = noise; g.ldb = dout; g.C = w_scratch; g.ldc = dout; g.M = n; g.N = dout; g.K = n;
    g.epi = WEPI_ADD_SRC; g.src = w_mean; g.lds = dout; g.src_scale = 1.f;
    launch_wide_gemm(g, (hipStream_t)stream);
    VJF_HIP(hipGetLastError());
    return launch_predict("vjf_blr_sample", VjfPredArgs{x, centroid, logwidth, w_scratch, w_chol, out, nullptr, B, n, d, dout}, (hipStream_t)stream);
}

int vjf_forecast_scratch_size(int32_t T, int32_t n, int32_t dout, int64_t* bytes) {
    if (!bytes || T < 1 || n < 1 || dout < 1) return fail(-20, "vjf_forecast_scratch_size: bad argument");
    *bytes = (int64_t)fc_scratch_bytes(T, n, dout);
    return 0;
}

int vjf_forecast_seq(const float* x0, const float* u, const float* w_noise, const float* s_noise, const float* centroid,
                     const float* logwidth, const float* w_mean, const float* w_chol, const float* tr_logvar, float* x, void* scratch,
                     int32_t T, int32_t B, int32_t n, int32_t d, int32_t dout, void* stream) {
    if (!x0 || !w_noise || !centroid || !logwidth || !w_mean || !w_chol || !x || !scratch) return fail(-1, "vjf_forecast_seq: null tensor");
    if (T < 1 || B < 1 || n < 1 || dout < 1 || d < dout) return fail(-20, "vjf_forecast_seq: bad shape (T=%d B=%d n=%d d=%d dout=%d)", T, B, n, d, dout);
    if (d > dout && !u) return fail(-21, "vjf_forecast_seq: u is required when d > dout");
    if (s_noise && !tr_logvar) return fail(-1, "vjf_forecast_seq: state noise without tr_logvar");
    const FcForms fm = fc_forms(n, d, dout);
    if (!fm.fits) return fail(-11, "vjf_forecast_seq: n=%d, d=%d too large", n, d);
    VjfFcArgs a{};
    a.u = u; a.c = centroid; a.logw = logwidth; a.tr_logvar = tr_logvar; a.B = B; a.n = n; a.d = d; a.dout = dout;
    return forecast_run(a, w_mean, w_chol, x0, w_noise, s_noise, x, scratch, T, fm, fc_env_int("VJF_FC_CHUNK"), nullptr, (hipStream_t)stream);
}

int vjf_forecast_ens_scratch_size(int32_t T, int32_t S, int32_t B, int32_t n, int32_t dout, int64_t* bytes) {
    if (!bytes || T < 0 || S < 1 || B < 1 || n < 1 || dout < 1) return fail(-20, "vjf_forecast_ens_scratch_size: bad argument");
    *bytes = (int64_t)(fe_w_bytes(T < 1 ? 1 : T, S, n, dout) + fe_x_bytes(T, S, B, dout));
    return 0;
}

int vjf_forecast_ens_chunks(int32_t T, int32_t S, int32_t B, int32_t n, int32_t dout, int32_t* members, int32_t* steps) {
    if (!members || !steps || T < 1 || S < 1 || B < 1 || n < 1 || dout < 1) return fail(-20, "vjf_forecast_ens_chunks: bad argument");
    const FeChunks ch = fe_chunks(T, S, B, n, dout, fc_env_int("VJF_FE_MEMBERS"), fc_env_int("VJF_FC_CHUNK"));
    *members = ch.Sc; *steps = ch.Tc;
    return 0;
}

int vjf_forecast_ens(const float* x0, int64_t x0_member_stride, const float* u, const float* w_noise, const float* s_noise,
                     const float* centroid, const float* logwidth, const float* w_mean, const float* w_chol, const float* tr_logvar,
                     const float* dec_W, const float* dec_b, float* x_mean, float* x_var, float* y_mean, float* y_var, float* x_members,
                     void* scratch, int32_t T, int32_t S, int32_t B, int32_t n, int32_t d, int32_t dout, int32_t dy, void* stream) {
    if (!x0 || !centroid || !logwidth || !w_mean || !w_chol || !x_mean || !x_var || !scratch || (T > 0 && !w_noise))
        return fail(-1, "vjf_forecast_ens: null tensor");
    if (dec_W && (!dec_b || !y_mean || !y_var)) return fail(-1, "vjf_forecast_ens: decoder without bias or y outputs");
    if (T < 0 || S < 1 || B < 1 || n < 1 || dout < 1 || d < dout || (dec_W && dy < 1) ||
        (x0_member_stride != 0 && x0_member_stride != (int64_t)B * dout))
        return fail(-20, "vjf_forecast_ens: bad shape (T=%d S=%d B=%d n=%d d=%d dout=%d dy=%d, x0 member stride %lld)", T, S, B, n, d, dout,
                    dy, (long long)x0_member_stride);
    if (d > dout && !u && T > 0) return fail(-21, "vjf_forecast_ens: u is required when d > dout");
    if (s_noise && !tr_logvar) return fail(-1, "vjf_forecast_ens: state noise without tr_logvar");
    if (!dec_W) dy = 0;
    const FcForms fm = fc_forms(n, d, dout);
    if (!fm.fits) return fail(-11, "vjf_forecast_ens: n=%d, d=%d too large", n, d);
    FeEns e{};
    e.mf = fe_mom_forms(dout, dy); e.x0_ms = x0_member_stride; e.members = fc_env_int("VJF_FE_MEMBERS");
    if (e.mf.lds > kMaxLds - 1024) return fail(-11, "vjf_forecast_ens: dout=%d too large", dout);
    VjfFeMomArgs& m = e.mom;
    m.dec_W = dec_W; m.dec_b = dec_b; m.x_mean = x_mean; m.x_var = x_var; m.y_mean = dy ? y_mean : nullptr; m.y_var = dy ? y_var : nullptr;
    m.S = S; m.B = B; m.dout = dout; m.dy = dy; m.mb = e.mf.mb;
    VjfFcArgs a{};
    a.u = u; a.c = centroid; a.logw = logwidth; a.tr_logvar = tr_logvar; a.B = B; a.n = n; a.d = d; a.dout = dout;
    return forecast_run(a, w_mean, w_chol, x0, w_noise, s_noise, x_members, scratch, T, fm, fc_env_int("VJF_FC_CHUNK"), &e, (hipStream_t)stream);
}

int vjf_tangent_plan(int32_t n, int32_t d, int32_t dout, int32_t m, int32_t* vectors_per_pass, int64_t* lds_bytes) {
    if (n < 1 || dout < 1 || d < dout || m < 1 || m > dout) return fail(-20, "vjf_tangent_plan: bad shape (n=%d d=%d dout=%d m=%d)", n, d, dout, m);
    const TgPlan p = tg_plan(n, d, dout, m, fc_env_on("VJF_FC_CENTROID_LDS"), fc_env_on("VJF_FC_LOOKAHEAD"));
    if (!p.fits) return fail(-11, "vjf_tangent_plan: n=%d, d=%d, dout=%d, m=%d beyond one workgroup's LDS", n, d, dout, m);
    if (vectors_per_pass) *vectors_per_pass = p.vg;
    if (lds_bytes) *lds_bytes = (int64_t)p.lds;
    return 0;
}

int vjf_tangent_rollout(const float* x0, const float* u, const float* q0, const float* centroid, const float* logwidth, const float* w_mean,
                        float* x_out, float* q_out, float* lsum, float* lhist, int32_t T, int32_t B, int32_t n, int32_t d, int32_t dout,
                        int32_t m, int32_t qr_every, int32_t accumulate, void* stream) {
    if (!x0 || !centroid || !logwidth || !w_mean || !x_out || !q_out || (qr_every > 0 && !lsum)) return fail(-1, "vjf_tangent_rollout: null tensor");
    if (T < 0 || B < 1 || n < 1 || dout < 1 || d < dout || m < 1 || m > dout || qr_every < 0 || (qr_every == 0 && lhist))
        return fail(-20, "vjf_tangent_rollout: bad shape (T=%d B=%d n=%d d=%d dout=%d m=%d qr_every=%d%s)", T, B, n, d, dout, m, qr_every,
                    qr_every == 0 && lhist ? ", a history without intervals" : "");
    if (d > dout && !u && T > 0) return fail(-21, "vjf_tangent_rollout: u is required when d > dout");
    const TgPlan p = tg_plan(n, d, dout, m, fc_env_on("VJF_FC_CENTROID_LDS"), fc_env_on("VJF_FC_LOOKAHEAD"));
    if (!p.fits) return fail(-11, "vjf_tangent_rollout: n=%d, d=%d, dout=%d, m=%d beyond one workgroup's LDS", n, d, dout, m);
    VjfTgArgs a{};
    a.u = u; a.c = centroid; a.logw = logwidth; a.w = w_mean; a.x_out = x_out; a.q_out = q_out; a.lsum = lsum; a.lhist = lhist;
    a.B = B; a.n = n; a.d = d; a.dout = dout; a.m = m; a.qr = qr_every;
    return tangent_run(a, x0, q0, T, accumulate != 0, p, fc_env_int("VJF_FC_CHUNK"), (hipStream_t)stream);
}

int vjf_fixed_points_plan(int32_t n, int32_t d, int32_t dout, int64_t* lds_bytes) {
    if (n < 1 || dout < 1 || d < dout) return fail(-20, "vjf_fixed_points_plan: bad shape (n=%d d=%d dout=%d)", n, d, dout);
    const FpPlan p = fp_plan(n, d, dout, fc_env_on("VJF_FC_CENTROID_LDS"));
    if (!p.fits)
        return fail(-11, "vjf_fixed_points_plan: n=%d, d=%d, dout=%d beyond %s", n, d, dout,
                    dout > VJF_FP_MAXDOUT ? "dout <= 32 (VJF_FP_MAXDOUT)" : "one workgroup's LDS");
    if (lds_bytes) *lds_bytes = (int64_t)p.lds;
    return 0;
}

int vjf_fixed_points(const float* x0, const float* u, const float* centroid, const float* logwidth, const float* w_mean, float* x,
                     float* residual, int32_t* n_iter, int32_t* converged, float* jac, int32_t B, int32_t n, int32_t d, int32_t dout,
                     int32_t max_iter, float tol, float lam0, void* stream) {
    if (!x0 || !centroid || !logwidth || !w_mean || !x || !residual || !n_iter || !converged) return fail(-1, "vjf_fixed_points: null tensor");
    if (B < 1 || n < 1 || dout < 1 || d < dout || max_iter < 0 || !(tol > 0.f && tol < INFINITY) || !(lam0 > 0.f && lam0 < INFINITY))
        return fail(-20, "vjf_fixed_points: bad shape (B=%d n=%d d=%d dout=%d max_iter=%d tol=%g lam0=%g)", B, n, d, dout, max_iter, (double)tol,
                    (double)lam0);
    if (d > dout && !u) return fail(-21, "vjf_fixed_points: u is required when d > dout");
    const FpPlan p = fp_plan(n, d, dout, fc_env_on("VJF_FC_CENTROID_LDS"));
    if (!p.fits)
        return fail(-11, "vjf_fixed_points: n=%d, d=%d, dout=%d beyond %s", n, d, dout,
                    dout > VJF_FP_MAXDOUT ? "dout <= 32 (VJF_FP_MAXDOUT)" : "one workgroup's LDS");
    VjfFpArgs a{};
    a.x0 = x0; a.u = d > dout ? u : nullptr; a.c = centroid; a.logw = logwidth; a.w = w_mean; a.x = x; a.residual = residual; a.n_iter = n_iter;
    a.converged = converged; a.jac = jac; a.B = B; a.n = n; a.d = d; a.dout = dout; a.max_iter = max_iter; a.tol = tol; a.lam0 = lam0;
    return fixed_point_run(a, p, (hipStream_t)stream);
}

int vjf_smooth_plan(int32_t n, int32_t d, int32_t dout, int64_t* lds_bytes) {
    if (n < 1 || dout < 1 || d < dout) return fail(-20, "vjf_smooth_plan: bad shape (n=%d d=%d dout=%d)", n, d, dout);
    const SmPlan p = sm_plan(n, d, dout, fc_env_on("VJF_FC_CENTROID_LDS"));
    if (!p.fits)
        return fail(-11, "vjf_smooth_plan: n=%d, d=%d, dout=%d beyond %s", n, d, dout,
                    dout > VJF_SM_MAXDOUT ? "dout <= 32 (VJF_SM_MAXDOUT)" : "one workgroup's LDS");
    if (lds_bytes) *lds_bytes = (int64_t)p.lds;
    return 0;
}

int vjf_smooth(const float* mu, const float* logvar, const float* u, const float* centroid, const float* logwidth, const float* w_mean,
               const float* after_mean, const float* after_cov, float* mean, float* var, float* cov, float* cov0, int32_t T, int32_t B,
               int32_t n, int32_t d, int32_t dout, float state_var, void* stream) {
    if (!mu || !logvar || !centroid || !logwidth || !w_mean || !mean || !var || !cov0) return fail(-1, "vjf_smooth: null tensor");
    if (T < 1 || B < 1 || n < 1 || dout < 1 || d < dout || !(state_var > 0.f && state_var < INFINITY) || !after_mean != !after_cov)
        return fail(-20, "vjf_smooth: bad shape (T=%d B=%d n=%d d=%d dout=%d state_var=%g%s)", T, B, n, d, dout, (double)state_var,
                    !after_mean != !after_cov ? ", one of after_mean / after_cov without the other" : "");
    if (d > dout && !u && (T > 1 || after_mean)) return fail(-21, "vjf_smooth: u is required when d > dout");
    const SmPlan p = sm_plan(n, d, dout, fc_env_on("VJF_FC_CENTROID_LDS"));
    if (!p.fits)
        return fail(-11, "vjf_smooth: n=%d, d=%d, dout=%d beyond %s", n, d, dout,
                    dout > VJF_SM_MAXDOUT ? "dout <= 32 (VJF_SM_MAXDOUT)" : "one workgroup's LDS");
    VjfSmArgs a{};
    a.mu = mu; a.lv = logvar; a.u = d > dout ? u : nullptr; a.c = centroid; a.logw = logwidth; a.w = w_mean; a.after_mean = after_mean;
    a.after_cov = after_cov; a.mean = mean; a.var = var; a.cov = cov; a.cov0 = cov0; a.T = T; a.B = B; a.n = n; a.d = d; a.dout = dout;
    a.rsq = 1.f / sqrtf(state_var);
    return smooth_run(a, p, (hipStream_t)stream);
}

int vjf_smooth_sample_plan(int32_t n, int32_t d, int32_t dout, int32_t S, int32_t* members_per_workgroup, int64_t* lds_bytes) {
    if (n < 1 || dout < 1 || d < dout || S < 1) return fail(-20, "vjf_smooth_sample_plan: bad shape (n=%d d=%d dout=%d S=%d)", n, d, dout, S);
    const SmsPlan p = sms_plan(n, d, dout, S, fc_env_on("VJF_FC_CENTROID_LDS"), fc_env_int("VJF_SMS_MEMBERS"));
    if (!p.fits)
        return fail(-11, "vjf_smooth_sample_plan: n=%d, d=%d, dout=%d beyond %s", n, d, dout,
                    dout > VJF_SMS_MAXDOUT ? "dout <= 32 (VJF_SMS_MAXDOUT)" : "one workgroup's LDS");
    if (members_per_workgroup) *members_per_workgroup = p.sc;
    if (lds_bytes) *lds_bytes = (int64_t)p.lds;
    return 0;
}

int vjf_smooth_sample(const float* mu, const float* logvar, const float* u, const float* centroid, const float* logwidth,
                      const float* w_mean, const float* noise, const float* after, float* x, int32_t T, int32_t S, int32_t B, int32_t n,
                      int32_t d, int32_t dout, float state_var, void* stream) {
    if (!mu || !logvar || !centroid || !logwidth || !w_mean || !noise || !x) return fail(-1, "vjf_smooth_sample: null tensor");
    if (T < 1 || S < 1 || B < 1 || n < 1 || dout < 1 || d < dout || !(state_var > 0.f && state_var < INFINITY))
        return fail(-20, "vjf_smooth_sample: bad shape (T=%d S=%d B=%d n=%d d=%d dout=%d state_var=%g)", T, S, B, n, d, dout, (double)state_var);
    if (d > dout && !u && (T > 1 || after)) return fail(-21, "vjf_smooth_sample: u is required when d > dout");
    const SmsPlan p = sms_plan(n, d, dout, S, fc_env_on("VJF_FC_CENTROID_LDS"), fc_env_int("VJF_SMS_MEMBERS"));
    if (!p.fits)
        return fail(-11, "vjf_smooth_sample: n=%d, d=%d, dout=%d beyond %s", n, d, dout,
                    dout > VJF_SMS_MAXDOUT ? "dout <= 32 (VJF_SMS_MAXDOUT)" : "one workgroup's LDS");
    if ((S + p.sc - 1) / p.sc > 65535) return fail(-11, "vjf_smooth_sample: S=%d beyond 65535 chunks of %d members", S, p.sc);
    VjfSmsArgs a{};
    a.mu = mu; a.lv = logvar; a.u = d > dout ? u : nullptr; a.c = centroid; a.logw = logwidth; a.w = w_mean; a.z = noise; a.after = after;
    a.x = x; a.T = T; a.S = S; a.B = B; a.n = n; a.d = d; a.dout = dout; a.rsq = 1.f / sqrtf(state_var);
    return smooth_sample_run(a, p, (hipStream_t)stream);
}

int vjf_kstep_score_scratch_size(int32_t T, int32_t B, int32_t K, int32_t dout, int32_t dy, int64_t* bytes) {
    if (!bytes || T < 1 || B < 1 || K < 1 || dout < 1 || dy < 0 || ((int64_t)K + 1) * (2 * (int64_t)dout + 2 * (int64_t)dy) > (1 << 28))
        return fail(-20, "vjf_kstep_score_scratch_size: bad argument");
    *bytes = (int64_t)ks_scratch_bytes(T, B, K, dout, dy);
    return 0;
}

int vjf_kstep_score_plan(int32_t T, int32_t B, int32_t K, int32_t n, int32_t d, int32_t dout, int32_t dy, int64_t* lds_bytes,
                         int64_t* tiles, int64_t* tiles_per_chunk, int32_t* forms) {
    if (T < 1 || B < 1 || K < 1 || n < 1 || dout < 1 || d < dout || dy < 0 || ((int64_t)K + 1) * (2 * (int64_t)dout + 2 * (int64_t)dy) > (1 << 28))
        return fail(-20, "vjf_kstep_score_plan: bad shape (T=%d B=%d K=%d n=%d d=%d dout=%d dy=%d)", T, B, K, n, d, dout, dy);
    const KsPlan p = ks_plan(T, B, K, n, d, dout, dy, fc_env_on("VJF_FC_CENTROID_LDS"), fc_env_on("VJF_FC_LOOKAHEAD"), fc_env_int("VJF_KS_CHUNK"));
    if (!p.fits)
        return fail(-11, "vjf_kstep_score_plan: n=%d, d=%d, dout=%d, dy=%d beyond one workgroup's LDS (%zu bytes)", n, d, dout, dy, kMaxLds - 1024);
    if (lds_bytes) *lds_bytes = (int64_t)p.lds;
    if (tiles) *tiles = p.tiles;
    if (tiles_per_chunk) *tiles_per_chunk = p.per_chunk;
    if (forms) *forms = (p.cl ? 1 : 0) | (p.la ? 2 : 0) | (p.dl ? 4 : 0);
    return 0;
}

int vjf_kstep_score(const float* mu, const float* y, const float* u, const float* centroid, const float* logwidth, const float* w_mean,
                    const float* dec_W, const float* dec_b, double* sse_x, double* base_x, double* sse_y, double* base_y, float* pred,
                    void* scratch, int32_t T, int32_t B, int32_t K, int32_t n, int32_t d, int32_t dout, int32_t dy, int32_t poisson,
                    void* stream) {
    if (!mu || !centroid || !logwidth || !w_mean || !sse_x || !base_x || !scratch || (y && (!sse_y || !base_y)))
        return fail(-1, "vjf_kstep_score: null tensor");
    if (y && (!dec_W || !dec_b)) return fail(-20, "vjf_kstep_score: y without a decoder");
    if (!y) dy = 0;
    if (T < 1 || B < 1 || K < 1 || n < 1 || dout < 1 || d < dout || (y && dy < 1) ||
        ((int64_t)K + 1) * (2 * (int64_t)dout + 2 * (int64_t)dy) > (1 << 28))
        return fail(-20, "vjf_kstep_score: bad shape (T=%d B=%d K=%d n=%d d=%d dout=%d dy=%d)", T, B, K, n, d, dout, dy);
    if (d > dout && !u) return fail(-21, "vjf_kstep_score: u is required when d > dout");
    const KsPlan p = ks_plan(T, B, K, n, d, dout, dy, fc_env_on("VJF_FC_CENTROID_LDS"), fc_env_on("VJF_FC_LOOKAHEAD"), fc_env_int("VJF_KS_CHUNK"));
    if (!p.fits)
        return fail(-11, "vjf_kstep_score: n=%d, d=%d, dout=%d, dy=%d beyond one workgroup's LDS (%zu bytes)", n, d, dout, dy, kMaxLds - 1024);
    VjfKsArgs a{};
    a.mu = mu; a.y = y; a.u = d > dout ? u : nullptr; a.c = centroid; a.logw = logwidth; a.w = w_mean; a.dec_W = dec_W; a.dec_b = dec_b;
    a.pred = pred; a.R = (long long)T * B; a.B = B; a.K = K; a.n = n; a.d = d; a.dout = dout; a.dy = dy; a.poisson = poisson != 0;
    VjfKsFoldArgs f{};
    f.sse_x = sse_x; f.base_x = base_x; f.sse_y = sse_y; f.base_y = base_y;
    return kstep_run(a, f, scratch, p, (hipStream_t)stream);
}

int vjf_ekf_plan(int32_t n, int32_t d, int32_t dout, int32_t dy, int64_t* lds_bytes) {
    if (n < 1 || dout < 1 || d < dout || dy < 1) return fail(-20, "vjf_ekf_plan: bad shape (n=%d d=%d dout=%d dy=%d)", n, d, dout, dy);
    const EkfPlan p = ekf_plan(n, d, dout, dy, fc_env_on("VJF_FC_CENTROID_LDS"), fc_env_on("VJF_EKF_DECODER_LDS"));
    if (!p.fits)
        return fail(-11, "vjf_ekf_plan: n=%d, d=%d, dout=%d beyond %s", n, d, dout,
                    dout > VJF_EKF_MAXDOUT ? "dout <= 32 (VJF_EKF_MAXDOUT)" : "one workgroup's LDS");
    if (lds_bytes) *lds_bytes = (int64_t)p.lds;
    return 0;
}

int vjf_ekf(const float* y, const float* u, const uint8_t* observed, const float* centroid, const float* logwidth, const float* w_mean,
            const float* dec_W, const float* dec_b, const float* prior_mean, const float* prior_logvar, const float* prior_cov,
            float* mean, float* var, float* cov, float* loglik, float* cov_last, int32_t T, int32_t B, int32_t n, int32_t d,
            int32_t dout, int32_t dy, float state_var, float obs_var, void* stream) {
    if (!y || !centroid || !logwidth || !w_mean || !dec_W || !dec_b || !prior_mean || !mean || !var || !loglik || !cov_last)
        return fail(-1, "vjf_ekf: null tensor");
    if (T < 1 || B < 1 || n < 1 || dout < 1 || d < dout || dy < 1 || !(state_var > 0.f && state_var < INFINITY) ||
        !(obs_var > 0.f && obs_var < INFINITY) || !prior_logvar == !prior_cov)
        return fail(-20, "vjf_ekf: bad shape (T=%d B=%d n=%d d=%d dout=%d dy=%d state_var=%g obs_var=%g%s)", T, B, n, d, dout, dy,
                    (double)state_var, (double)obs_var, !prior_logvar == !prior_cov ? ", exactly one of prior_logvar / prior_cov is needed" : "");
    if (d > dout && !u) return fail(-21, "vjf_ekf: u is required when d > dout");
    const EkfPlan p = ekf_plan(n, d, dout, dy, fc_env_on("VJF_FC_CENTROID_LDS"), fc_env_on("VJF_EKF_DECODER_LDS"));
    if (!p.fits)
        return fail(-11, "vjf_ekf: n=%d, d=%d, dout=%d beyond %s", n, d, dout,
                    dout > VJF_EKF_MAXDOUT ? "dout <= 32 (VJF_EKF_MAXDOUT)" : "one workgroup's LDS");
    VjfEkfArgs a{};
    a.y = y; a.u = d > dout ? u : nullptr; a.obs = observed; a.c = centroid; a.logw = logwidth; a.w = w_mean; a.dec_W = dec_W;
    a.dec_b = dec_b; a.prior_mean = prior_mean; a.prior_lv = prior_logvar; a.prior_cov = prior_cov; a.mean = mean; a.var = var;
    a.cov = cov; a.ll = loglik; a.cov_last = cov_last; a.T = T; a.B = B; a.n = n; a.d = d; a.dout = dout; a.dy = dy; a.q = state_var;
    a.r = obs_var;
    return ekf_run(a, p, (hipStream_t)stream);
}

int vjf_laplace_filter_plan(int32_t n, int32_t d, int32_t dout, int32_t dy, int64_t* lds_bytes) {
    if (n < 1 || dout < 1 || d < dout || dy < 1)
        return fail(-20, "vjf_laplace_filter_plan: bad shape (n=%d d=%d dout=%d dy=%d)", n, d, dout, dy);
    const LapPlan p = lap_plan(n, d, dout, dy, fc_env_on("VJF_FC_CENTROID_LDS"), fc_env_on("VJF_LAPLACE_DECODER_LDS"));
    if (!p.fits)
        return fail(-11, "vjf_laplace_filter_plan: n=%d, d=%d, dout=%d beyond %s", n, d, dout,
                    dout > VJF_LAP_MAXDOUT ? "dout <= 24 (VJF_LAP_MAXDOUT)" : "one workgroup's LDS");
    if (lds_bytes) *lds_bytes = (int64_t)p.lds;
    return 0;
}

int vjf_laplace_filter(const float* y, const float* u, const uint8_t* observed, const float* centroid, const float* logwidth,
                       const float* w_mean, const float* dec_W, const float* dec_b, const float* prior_mean, const float* prior_logvar,
                       const float* prior_cov, float* mean, float* var, float* cov, float* loglik, float* grad_norm, float* cov_last,
                       int32_t T, int32_t B, int32_t n, int32_t d, int32_t dout, int32_t dy, int32_t n_iter, float state_var,
                       void* stream) {
    if (!y || !centroid || !logwidth || !w_mean || !dec_W || !dec_b || !prior_mean || !mean || !var || !loglik || !grad_norm || !cov_last)
        return fail(-1, "vjf_laplace_filter: null tensor");
    if (T < 1 || B < 1 || n < 1 || dout < 1 || d < dout || dy < 1 || n_iter < 1 || n_iter > VJF_LAP_MAXITER ||
        !(state_var > 0.f && state_var < INFINITY) || !prior_logvar == !prior_cov)
        return fail(-20, "vjf_laplace_filter: bad shape (T=%d B=%d n=%d d=%d dout=%d dy=%d n_iter=%d (1..64) state_var=%g%s)", T, B, n, d,
                    dout, dy, n_iter, (double)state_var,
                    !prior_logvar == !prior_cov ? ", exactly one of prior_logvar / prior_cov is needed" : "");
    if (d > dout && !u) return fail(-21, "vjf_laplace_filter: u is required when d > dout");
    const LapPlan p = lap_plan(n, d, dout, dy, fc_env_on("VJF_FC_CENTROID_LDS"), fc_env_on("VJF_LAPLACE_DECODER_LDS"));
    if (!p.fits)
        return fail(-11, "vjf_laplace_filter: n=%d, d=%d, dout=%d beyond %s", n, d, dout,
                    dout > VJF_LAP_MAXDOUT ? "dout <= 24 (VJF_LAP_MAXDOUT)" : "one workgroup's LDS");
    VjfLapArgs a{};
    a.y = y; a.u = d > dout ? u : nullptr; a.obs = observed; a.c = centroid; a.logw = logwidth; a.w = w_mean; a.dec_W = dec_W;
    a.dec_b = dec_b; a.prior_mean = prior_mean; a.prior_lv = prior_logvar; a.prior_cov = prior_cov; a.mean = mean; a.var = var;
    a.cov = cov; a.ll = loglik; a.gn = grad_norm; a.cov_last = cov_last; a.T = T; a.B = B; a.n = n; a.d = d; a.dout = dout; a.dy = dy;
    a.n_iter = n_iter; a.q = state_var;
    return lap_run(a, p, (hipStream_t)stream);
}

int vjf_rls_scratch_size(int32_t B, int32_t n, int32_t dout, int64_t* bytes) {
    if (!bytes || B < 1 || n < 1 || dout < 1) return fail(-20, "vjf_rls_scratch_size: bad argument");
    *bytes = (int64_t)rls_carve(B, n, dout, nullptr).total;
    return 0;
}

int vjf_blr_rls(const float* x, const float* target, const float* v, float shrink, const float* centroid, const float* logwidth,
                float* w_mean, float* w_chol, float* w_precision, float* w_pchol, void* scratch, uint32_t* status, int32_t B,
                int32_t n, int32_t d, int32_t dout, void* stream) {
    if (!x || !target || !v || !centroid || !logwidth || !w_mean || !w_chol || !w_precision || !w_pchol || !scratch)
        return fail(-1, "vjf_blr_rls: null tensor");
    if (B < 1 || n < 1 || d < 1 || dout < 1) return fail(-20, "vjf_blr_rls: bad shape");
    return rls_update("vjf_blr_rls", "RLS kernel", vjf_rls_kernel, scratch, x, target, centroid, logwidth, B, n, d, dout, stream, [&](VjfRlsArgs& a, const RlsStats& st) {
        a.Pm = w_precision; a.Wm = w_mean; a.Wc = w_chol; a.Lm = w_pchol;
        a.G = st.red + st.P.red_G; a.FDX = st.red + st.P.red_FDX; a.v = v; a.work = (float*)(st.ws + st.c.work); a.status = status;
        a.n = n; a.dout = dout; a.shrink = shrink;
    });
}

int vjf_kalman_scratch_size(int32_t B, int32_t n, int32_t dout, int64_t* bytes) {
    if (!bytes || B < 1 || n < 1 || dout < 1) return fail(-20, "vjf_kalman_scratch_size: bad argument");
    *bytes = (int64_t)(rls_carve(B, n, dout, nullptr).total + 6 * kalman_stride(n, dout));
    return 0;
}

int vjf_blr_kalman(const float* x, const float* target, const float* v, float diffusion, const float* centroid, const float* logwidth,
                   float* w_mean, float* w_chol, void* scratch, uint32_t* status, int32_t B, int32_t n, int32_t d, int32_t dout,
                   void* stream) {
    if (!x || !target || !v || !centroid || !logwidth || !w_mean || !w_chol || !scratch) return fail(-1, "vjf_blr_kalman: null tensor");
    if (B < 1 || n < 1 || d < 1 || dout < 1) return fail(-20, "vjf_blr_kalman: bad shape");
    if (!(diffusion >= 0.f)) return fail(-25, "vjf_blr_kalman: diffusion needs to be non-negative");   // module.py:127
    return rls_update("vjf_blr_kalman", "kernel", vjf_kalman_kernel, scratch, x, target, centroid, logwidth, B, n, d, dout, stream, [&](VjfKalmanArgs& a, const RlsStats& st) {
        a.Wm = w_mean; a.Wc = w_chol; a.G = st.red + st.P.red_G; a.Fy = st.red + st.P.red_FDX; a.v = v;
        for (int q = 0; q < 6; ++q) a.T[q] = (float*)(st.ws + st.c.total + (size_t)q * kalman_stride(n, dout));
        a.Dinv = (float*)(st.ws + st.c.work);
        a.status = status; a.n = n; a.dout = dout; a.diffusion = diffusion;
    });
}

int vjf_recognition_forward(const float* y, const float* u, const float* mu_s, const float* lv_s, const float* const* rec_W,
                            const float* const* rec_b, const float* mean_W, const float* lv_W, const float* lv_b, float* mu_t,
                            float* lv_t, int32_t B, int32_t ydim, int32_t udim, int32_t xdim, int32_t n_hidden,
                            const int32_t* hidden, void* stream) {
    return recognition_forward("vjf_recognition_forward", y, u, mu_s, lv_s, rec_W, rec_b, mean_W, lv_W, lv_b, mu_t, lv_t, B, ydim, udim,
                               xdim, n_hidden, hidden, nullptr, stream);
}

int vjf_recognition_forward_act(const float* y, const float* u, const float* mu_s, const float* lv_s, const float* const* rec_W,
                                const float* const* rec_b, const float* mean_W, const float* lv_W, const float* lv_b, float* mu_t,
                                float* lv_t, int32_t B, int32_t ydim, int32_t udim, int32_t xdim, int32_t n_hidden,
                                const int32_t* hidden, const vjf_activation* act, void* stream) {
    VjfAct f{};
    if (int rc = act_check(act, "vjf_recognition_forward_act", &f)) return rc;
    return recognition_forward("vjf_recognition_forward_act", y, u, mu_s, lv_s, rec_W, rec_b, mean_W, lv_W, lv_b, mu_t, lv_t, B, ydim,
                               udim, xdim, n_hidden, hidden, &f, stream);
}

int vjf_gaussian_loss(const float* m1, const float* lv1, const float* m2, const float* lv2, const float* logvar, float* out,
                      int32_t B, int32_t d, void* stream) {
    if (!m1 || !m2 || !logvar || !out) return fail(-1, "vjf_gaussian_loss: null tensor");
    if (B < 1 || d < 1) return fail(-20, "vjf_gaussian_loss: bad shape");
    return launch_loss(0, m1, lv1, m2, lv2, logvar, out, B, d, (hipStream_t)stream);
}

int vjf_gaussian_entropy(const float* lv, float* out, int32_t B, int32_t d, void* stream) {
    if (!lv || !out) return fail(-1, "vjf_gaussian_entropy: null tensor");
    if (B < 1 || d < 1) return fail(-20, "vjf_gaussian_entropy: bad shape");
    return launch_loss(1, lv, nullptr, nullptr, nullptr, nullptr, out, B, d, (hipStream_t)stream);
}

int vjf_poisson_loss(const float* eta, const float* target, float* out, int32_t B, int32_t d, void* stream) {
    if (!eta || !target || !out) return fail(-1, "vjf_poisson_loss: null tensor");
    if (B < 1 || d < 1) return fail(-20, "vjf_poisson_loss: bad shape");
    return launch_loss(2, eta, nullptr, target, nullptr, nullptr, out, B, d, (hipStream_t)stream);
}

int vjf_linear_forward(const float* x, const float* W, const float* b, float* out, int32_t B, int32_t din, int32_t dout, void* stream) {
    if (!x || !W || !out) return fail(-1, "vjf_linear_forward: null tensor");
    if (B < 1 || din < 1 || dout < 1) return fail(-20, "vjf_linear_forward: bad shape");
    VjfWideGemm g{};                                       // out = x W^T + b on the matrix cores (vjf_trial_wide.h)
    g.A = x; g.lda = din; g.Bm = W; g.ldb = din; g.nt = 1; g.C = out; g.ldc = dout; g.M = B; g.N = dout; g.K = din;
    g.epi = b ? WEPI_BIAS : WEPI_NONE; g.bias = b;
    launch_wide_gemm(g, (hipStream_t)stream);
    VJF_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
