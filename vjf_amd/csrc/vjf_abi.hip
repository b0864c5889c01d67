// vjf_abi.hip -- extern "C" entry points declared in include/vjf_hip.h.  gfx950 only.
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
    if (c->mega_ok) {
        const VjfMegaTrialLds Lo = vjf_mega_trial_lds(P, (int)(kMegaLds / 4) - 8);
        tb = slab_tables(P, Lo, vjf_mega_slab_layout(P));
        if (e == hipSuccess) e = hipMemcpyAsync(c->mg_pidx(), tb.pidx.data(), tb.pidx.size() * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c->mg_cidx(), tb.cidx.data(), tb.cidx.size() * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c->mg_grp(), tb.grp.data(), tb.grp.size() * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->mg_img(), 0, (size_t)Lo.th_len * 4, c->stream);   // (its padding stays 0)
        if (e == hipSuccess) e = hipMemsetAsync(c->mega_counters(0), 0, (size_t)2 * MG_C_WORDS * 4, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // `jobs`, `tb` (host) must outlive the copies
    if (e != hipSuccess) { delete c; return fail(-100, "vjf_ctx_create: %s", hipGetErrorString(e)); }
    allow_lds(vjf_serial_kernel, c->lds_k2);
    allow_lds(vjf_rls_post_kernel, c->lds_post);
    allow_lds(vjf_prepg_kernel, vjf_prepg_lds_bytes(P));
    if (c->mfma_trial) allow_lds(vjf_trial_mfma_kernel, c->lds_k1m);
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

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// stand-alone operators
// ------------------------------------------------------------------------------------------------
namespace {
inline dim3 grid1d(size_t n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }
// slot of the loss kernels' partial-sum table for this call (handed out in turn: VJF_LOSS_SLOTS calls may be in flight)
inline int loss_slot() { static std::atomic<unsigned> next{0}; return (int)(next.fetch_add(1u, std::memory_order_relaxed) % VJF_LOSS_SLOTS); }

struct VjfPredArgs {
    const float* x; const float* c; const float* logw; const float* w_mean; const float* w_chol;
    float* mean; float* logvar; int B, n, d, dout;
};
// 16 trials per workgroup: features feature-major in LDS ([feature][17], as the fused kernels hold them), then Phi W (mean)
// and the row norm of Phi w_chol (logvar) as 16 x 16 output tiles on v_mfma_f32_16x16x4_f32 (mma_tile: the matrices are k-major
// for these products), one tile per wavefront and round.
__global__ __launch_bounds__(VJF_K1_THREADS) void vjf_blr_predict_kernel(VjfPredArgs A) {
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_K1_THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_phi = smem;                 // n x LD
    float* s_red = s_phi + A.n * LD;     // NW x TB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b0 = blockIdx.x * TB, nb = min(TB, A.B - b0);
    for (int i = tid; i < TB * A.n; i += VJF_K1_THREADS) {
        const int k = i / TB, b = i - k * TB;
        float ph = 0.f;
        if (b < nb) {
            float d2 = 0.f;
            for (int j = 0; j < A.d; ++j) { const float t = A.x[(size_t)(b0 + b) * A.d + j] - A.c[(size_t)k * A.d + j]; d2 = fmaf(t, t, d2); }
            const float w = expf(A.logw[k]);
            ph = expf(-0.5f * d2 / (w * w));
        }
        s_phi[k * LD + b] = ph;
    }
    __syncthreads();
    const int col = lane & 15, r4 = 4 * (lane >> 4);     // accumulator: row = r4 + r (output), column = trial
    if (A.mean)
        for (int t = wave; t * 16 < A.dout; t += NW) {
            vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            mma_tile(acc, A.w_mean, A.dout, A.dout, t * 16, s_phi, A.n, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = t * 16 + r4 + r;
                if (j < A.dout && col < nb) A.mean[(size_t)(b0 + col) * A.dout + j] = acc[r];
            }
        }
    if (!A.logvar) return;
    float v2 = 0.f;                                      // this lane's share of sum_j Z[trial col][j]^2
    for (int t = wave; t * 16 < A.n; t += NW) {
        vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        mma_tile(acc, A.w_chol, A.n, A.n, t * 16, s_phi, A.n, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) v2 = fmaf(acc[r], acc[r], v2);      // (rows beyond n are exact zeros)
    }
    v2 += __shfl_xor(v2, 16, 64);                        // the four row groups of a column, fixed order
    v2 += __shfl_xor(v2, 32, 64);
    if (lane < 16) s_red[wave * TB + lane] = v2;
    __syncthreads();
    for (int i = tid; i < nb * A.dout; i += VJF_K1_THREADS) {
        const int b = i / A.dout;
        float v = s_red[b];
        for (int w = 1; w < NW; ++w) v += s_red[w * TB + b];
        A.logvar[(size_t)(b0 + b) * A.dout + (i - b * A.dout)] = logf(v);
    }
}

// the sampled roll-out of vjf_forecast_seq: vjf_fc_weights_kernel, vjf_fc_rollout_kernel
#include "vjf_forecast_kernel.h"
// the ensemble of roll-outs of vjf_forecast_ens: vjf_fe_weights_kernel, vjf_fe_rollout_kernel, vjf_fe_moments_kernel
#include "vjf_forecast_ens_kernel.h"

struct VjfRecArgs {
    const float* y; const float* u; const float* mu_s; const float* lv_s;
    const float* W[VJF_MAX_HIDDEN]; const float* b[VJF_MAX_HIDDEN];
    const float* mean_W; const float* lv_W; const float* lv_b;
    float* mu_t; float* lv_t;
    int B, dy, du, dz, L; int h[VJF_MAX_HIDDEN];
};
// Recognition.forward for 16 trials per workgroup: activations feature-major in LDS (ping-pong), every layer as 16 x 16 output
// tiles on v_mfma_f32_16x16x4_f32 with the weights read as torch stores them (mma_tile<true>).
#define VJF_RECOGNITION_ACT 0
#include "vjf_recognition_kernel.h"     // vjf_recognition_kernel
#undef VJF_RECOGNITION_ACT
#define VJF_RECOGNITION_ACT 1
#include "vjf_recognition_kernel.h"     // vjf_recognition_act_kernel
#undef VJF_RECOGNITION_ACT

// features + target rows of the stand-alone RLS:  E[b] = [Phi(x_b) | target_b | 0]
__global__ void vjf_rls_rows_kernel(const float* x, const float* c, const float* logw, const float* target, float* E,
                                    int B, int n, int d, int dout, int ldE) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * ldE) return;
    const int b = (int)(i / ldE), k = (int)(i - (size_t)b * ldE);
    float v = 0.f;
    if (k < n) {
        float d2 = 0.f;
        for (int j = 0; j < d; ++j) { const float t = x[(size_t)b * d + j] - c[(size_t)k * d + j]; d2 = fmaf(t, t, d2); }
        const float w = expf(logw[k]);
        v = expf(-0.5f * d2 / (w * w));
    } else if (k < n + dout) {
        v = target[(size_t)b * dout + (k - n)];
    }
    E[i] = v;
}

// plan for the stand-alone RLS (only the fields the Gram kernels read for kind-0 jobs)
void rls_plan(int n, int dout, VjfPlan* P) {
    memset(P, 0, sizeof *P);
    P->n = n; P->dz = dout;
    P->ldE = (int)vjf_align(n + dout, VJF_TILE);
    P->red_SCA = 0; P->red_G = 0; P->red_FDX = n * n; P->red_SC = (int)vjf_align((int64_t)n * n + (int64_t)n * dout, 4);
    P->red_len = P->red_SC + RS_N;
}
struct RlsCarve { size_t E, slabs, red, work, jobs, partial, total; int njobs, nsplit; };
RlsCarve rls_carve(int B, int n, int dout, std::vector<VjfJob>* jobs_out) {
    VjfPlan P; rls_plan(n, dout, &P);
    std::vector<VjfJob> jobs; build_jobs(P, jobs);
    // build_jobs also emits gradient jobs from the (zeroed) plan: keep kind 0 only
    std::vector<VjfJob> k0;
    for (auto& j : jobs) if (j.kind == 0) k0.push_back(j);
    RlsCarve c{};
    c.njobs = (int)k0.size(); c.nsplit = split_for(B);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = (o + bytes + 255) / 256 * 256; return at; };
    c.E = take((size_t)B * P.ldE * 4);
    c.slabs = take((size_t)c.njobs * c.nsplit * 1024 * 4);
    c.red = take((size_t)P.red_len * 4);
    VjfPlan Q = P;
    c.work = take(vjf_serial_work_floats(Q) * 4);
    c.jobs = take(k0.size() * sizeof(VjfJob));
    c.partial = take(RS_N * 4);
    c.total = o;
    if (jobs_out) *jobs_out = k0;
    return c;
}
// Phi W (a.mean) and the row norm of Phi w_chol (a.logvar, or null) of vjf_blr_predict / vjf_blr_sample
int launch_predict(const char* who, const VjfPredArgs& a, hipStream_t s) {
    const size_t lds = ((size_t)a.n * VJF_LDT + 64) * 4;
    if (lds > kMaxLds - 1024) return fail(-11, "%s: n=%d too large", who, a.n);
    allow_lds(vjf_blr_predict_kernel, lds);
    hipLaunchKernelGGL(vjf_blr_predict_kernel, dim3((a.B + 15) / 16), dim3(VJF_K1_THREADS), lds, s, a);
    VJF_HIP(hipGetLastError());
    return 0;
}
// the statistics of the stand-alone RLS / Kalman updates: rows [Phi | target] -> Gram tiles -> their reduction; G and Phi^T target are
// then in the scratch's reduce buffer (*red_out), laid out as `P` (rls_plan) says
int rls_statistics(const VjfPlan& P, void* scratch, const float* x, const float* centroid, const float* logwidth, const float* target,
                   int B, int n, int d, int dout, hipStream_t s, RlsCarve* carve, float** red_out) {
    std::vector<VjfJob> jobs;
    const RlsCarve c = rls_carve(B, n, dout, &jobs);
    char* ws = (char*)scratch;
    VJF_HIP(hipMemcpyAsync(ws + c.jobs, jobs.data(), jobs.size() * sizeof(VjfJob), hipMemcpyHostToDevice, s));
    VJF_HIP(hipStreamSynchronize(s));     // host vector goes out of scope
    VJF_HIP(hipMemsetAsync(ws + c.partial, 0, RS_N * 4, s));
    float* E = (float*)(ws + c.E);
    hipLaunchKernelGGL(vjf_rls_rows_kernel, grid1d((size_t)B * P.ldE), dim3(256), 0, s, x, centroid, logwidth, target, E, B, n, d, dout, P.ldE);
    VJF_HIP(hipGetLastError());
    VjfGramArgs g{};
    g.jobs = (const VjfJob*)(ws + c.jobs); g.E = E; g.ACT = E; g.DEL = E; g.slabs = (float*)(ws + c.slabs);
    g.B = B; g.nsplit = c.nsplit; g.rows_per_split = ((B + c.nsplit - 1) / c.nsplit + 7) / 8 * 8;
    hipLaunchKernelGGL(vjf_gram_kernel, dim3(c.njobs * c.nsplit), dim3(VJF_GRAM_THREADS), 0, s, P, g);
    VJF_HIP(hipGetLastError());
    VjfReduceArgs r{};
    r.jobs = g.jobs; r.slabs = g.slabs; r.partial = (const float*)(ws + c.partial); r.red = (float*)(ws + c.red);
    r.njobs = c.njobs; r.nsplit = c.nsplit; r.nblocks_k1 = 1;
    hipLaunchKernelGGL(vjf_gram_reduce_kernel, dim3(c.njobs), dim3(VJF_REDUCE_THREADS), 0, s, P, r);   // sc_mask = 0: no loss sums here
    VJF_HIP(hipGetLastError());
    *carve = c; *red_out = r.red;
    return 0;
}
}  // namespace

extern "C" {

int vjf_rbf_forward(const float* x, const float* centroid, const float* logwidth, float* out, int32_t B, int32_t n, int32_t d,
                    void* stream) {
    if (!x || !centroid || !logwidth || !out) return fail(-1, "vjf_rbf_forward: null tensor");
    if (B < 1 || n < 1 || d < 1) return fail(-20, "vjf_rbf_forward: bad shape");
    const size_t lds = (size_t)16 * d * 4;
    if (lds > kMaxLds - 1024) return fail(-11, "vjf_rbf_forward: d=%d too large", d);
    allow_lds(vjf_rbf_kernel, lds);
    hipLaunchKernelGGL(vjf_rbf_kernel, dim3((n + 255) / 256, (B + 15) / 16), dim3(256), lds, (hipStream_t)stream, x, centroid, logwidth, out, B, n, d);
    VJF_HIP(hipGetLastError());
    return 0;
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
    hipStream_t s = (hipStream_t)stream;
    // w = w_mean + w_chol @ noise   (module.py:71)
    {
        VjfWideGemm g{};
        g.A = w_chol; g.lda = n; g.Bm = noise; g.ldb = dout; g.C = w_scratch; g.ldc = dout; g.M = n; g.N = dout; g.K = n;
        g.epi = WEPI_ADD_SRC; g.src = w_mean; g.lds = dout; g.src_scale = 1.f;
        launch_wide_gemm(g, s);
    }
    VJF_HIP(hipGetLastError());
    return launch_predict("vjf_blr_sample", VjfPredArgs{x, centroid, logwidth, w_scratch, w_chol, out, nullptr, B, n, d, dout}, s);
}

namespace {
// Steps per chunk of vjf_forecast_seq: the weight samples of a chunk (n dout floats per step) take at most kFcScratchBytes, and a
// chunk is at most kFcMaxChunk steps (a roll-out launch stays on the device for milliseconds, not seconds).  VJF_FC_CHUNK (tests)
// asks for shorter chunks.
constexpr size_t kFcScratchBytes = (size_t)8 << 20;
constexpr int kFcMaxChunk = 4096;
int fc_chunk_bound(int n, int dout) {
    const size_t per = (size_t)n * dout * 4;
    const size_t c = kFcScratchBytes / per;
    return c < 1 ? 1 : (c > (size_t)kFcMaxChunk ? kFcMaxChunk : (int)c);
}
int fc_chunk(int n, int dout) {
    const int bound = fc_chunk_bound(n, dout);
    const char* ce = getenv("VJF_FC_CHUNK");
    return ce && atoi(ce) >= 1 && atoi(ce) < bound ? atoi(ce) : bound;
}
// (four rows of padding behind the last W[t]: a wavefront whose share of K is shorter than 4 features -- n = 37: 12, 12, 12, 1 --
//  hands mma_tile a K < 4, whose lanes kk >= K read row kb + kk, up to n + 2, from a valid address and mask the value)
size_t fc_scratch_bytes(int T, int n, int dout) {
    const int bound = fc_chunk_bound(n, dout);
    return ((size_t)(T < bound ? T : bound) * n * dout * 4 + (size_t)4 * dout * 4 + 255) / 256 * 256;
}
bool fc_env_on(const char* name) { const char* v = getenv(name); return !(v && atoi(v) == 0 && v[0] == '0'); }
}  // namespace

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
    hipStream_t s = (hipStream_t)stream;
    const int du = d - dout;
    if (vjf_fc_lds_floats(n, d, dout, false) * 4 > kMaxLds - 1024) return fail(-11, "vjf_forecast_seq: n=%d, d=%d too large", n, d);
    // VJF_FC_CENTROID_LDS=0 / VJF_FC_LOOKAHEAD=0 (tests): the forms for shapes beyond the LDS / register budgets, at any shape
    const bool cl = vjf_fc_lds_floats(n, d, dout, true) * 4 <= kMaxLds - 1024 && fc_env_on("VJF_FC_CENTROID_LDS");
    const bool la = cl && n <= 64 * VJF_FC_KQ && dout <= 32 && fc_env_on("VJF_FC_LOOKAHEAD");
    const size_t lds = vjf_fc_lds_floats(n, d, dout, cl) * 4, lds_w = (size_t)n * VJF_LDT * 4;
    const int mt = (n + 15) / 16, chunk = fc_chunk(n, dout);
    float* W = (float*)scratch;
    allow_lds(vjf_fc_weights_kernel, lds_w);
    for (int32_t t0 = 0; t0 < T; t0 += chunk) {
        const int Tc = T - t0 < chunk ? T - t0 : chunk;
        VjfFcWeightArgs wa{w_mean, w_chol, w_noise + (size_t)t0 * n * dout, W, Tc, n, dout};
        int gy = (Tc + VJF_FC_WAVES - 1) / VJF_FC_WAVES, cap = 2048 / mt;
        if (gy > cap) gy = cap;
        if (gy < 1) gy = 1;
        hipLaunchKernelGGL(vjf_fc_weights_kernel, dim3(mt, gy), dim3(VJF_FC_THREADS), lds_w, s, wa);
        VJF_HIP(hipGetLastError());
        VjfFcArgs a{};
        a.x_in = t0 == 0 ? x0 : x + (size_t)t0 * B * dout;
        a.u = u ? u + (size_t)t0 * B * du : nullptr;
        a.e = s_noise ? s_noise + (size_t)t0 * B * dout : nullptr;
        a.c = centroid; a.logw = logwidth; a.W = W; a.tr_logvar = tr_logvar;
        a.x0_out = t0 == 0 ? x : nullptr;
        a.x_out = x + (size_t)(t0 + 1) * B * dout;
        a.Tc = Tc; a.B = B; a.n = n; a.d = d; a.dout = dout;
        auto launch = [&](auto kernel) {
            allow_lds(kernel, lds);
            hipLaunchKernelGGL(kernel, dim3((B + 15) / 16), dim3(VJF_FC_THREADS), lds, s, a);
        };
        if (la && dout <= 16) launch(vjf_fc_rollout_kernel<1, true>);
        else if (la) launch(vjf_fc_rollout_kernel<2, true>);
        else if (cl) launch(vjf_fc_rollout_kernel<0, true>);
        else launch(vjf_fc_rollout_kernel<0, false>);
        VJF_HIP(hipGetLastError());
    }
    return 0;
}

namespace {
// Chunks of vjf_forecast_ens: Sc members x Tc steps whose weight samples take at most kFcScratchBytes and whose states (Tc + 1 rows
// of B dout floats per member) at most kFeStateBytes; where one member-step is more than a cap, the chunk is that one member-step.
// As many members side by side as the caps allow while a chunk keeps kFeMinChunk steps (a launch per chunk of steps is worth that
// many), the member chunks levelled.  VJF_FE_MEMBERS / VJF_FC_CHUNK (tests) ask for fewer members / steps per chunk.
constexpr size_t kFeStateBytes = (size_t)32 << 20;
constexpr int kFeMaxMembers = 4096, kFeMinChunk = 16;
struct FeChunks { int Sc, Tc; };
FeChunks fe_chunks(int T, int S, int B, int n, int dout) {
    const size_t wstep = (size_t)n * dout * 4, xstep = (size_t)B * dout * 4;
    // steps per chunk that `sc` members leave room for: sc tc samples within kFcScratchBytes and sc (tc + 1) rows within
    // kFeStateBytes; 0 where not even one step of `sc` members fits
    auto steps = [&](int sc) {
        const size_t w = kFcScratchBytes / wstep / sc, rows = kFeStateBytes / xstep / sc, x = rows > 1 ? rows - 1 : 0;
        size_t t = w < x ? w : x;
        t = t > (size_t)kFcMaxChunk ? (size_t)kFcMaxChunk : t;
        return (int)(t > (size_t)T ? (size_t)T : t);
    };
    // members that `tc` steps leave room for (0: not one)
    auto members = [&](int tc) {
        const size_t w = kFcScratchBytes / wstep / tc, x = kFeStateBytes / xstep / ((size_t)tc + 1);
        return w < x ? w : x;
    };
    const int want = T < kFeMinChunk ? T : kFeMinChunk;
    int sc = S < kFeMaxMembers ? S : kFeMaxMembers;
    if (steps(sc) < want) {                              // fewer members, so that a chunk keeps `want` steps; else as many as one step allows
        size_t m = members(want);
        if (m < 1) m = members(1);
        sc = m < 1 ? 1 : (m < (size_t)sc ? (int)m : sc);
    }
    const int nch = (S + sc - 1) / sc;
    sc = (S + nch - 1) / nch;
    const char* me = getenv("VJF_FE_MEMBERS");
    if (me && atoi(me) >= 1 && atoi(me) < sc) sc = atoi(me);
    int tc = steps(sc);
    if (tc < 1) tc = 1;                                  // (sc = 1 here: one member-step, more than a cap)
    const char* ce = getenv("VJF_FC_CHUNK");
    if (ce && atoi(ce) >= 1 && atoi(ce) < tc) tc = atoi(ce);
    return FeChunks{sc, tc};
}
// min(a b per, cap), at least `least`, without overflow
size_t fe_capped(int a, int64_t b, size_t per, size_t cap, size_t least) {
    const size_t room = cap / per;
    const size_t v = (size_t)a * (size_t)b <= room ? (size_t)a * (size_t)b * per : cap;
    return v < least ? least : v;
}
// [weight samples of a chunk + four rows of padding (fc_scratch_bytes)] [states of a chunk]: whatever chunking the call takes
size_t fe_w_bytes(int T, int S, int n, int dout) {
    const size_t wstep = (size_t)n * dout * 4;
    return (fe_capped(S, T, wstep, kFcScratchBytes, wstep) + (size_t)4 * dout * 4 + 255) / 256 * 256;
}
size_t fe_x_bytes(int T, int S, int B, int dout) {
    const size_t xstep = (size_t)B * dout * 4;
    return (fe_capped(S, (int64_t)T + 1, xstep, kFeStateBytes, 2 * xstep) + 255) / 256 * 256;
}
}  // namespace

int vjf_forecast_ens_scratch_size(int32_t T, int32_t S, int32_t B, int32_t n, int32_t dout, int64_t* bytes) {
    if (!bytes || T < 0 || S < 1 || B < 1 || n < 1 || dout < 1) return fail(-20, "vjf_forecast_ens_scratch_size: bad argument");
    *bytes = (int64_t)(fe_w_bytes(T < 1 ? 1 : T, S, n, dout) + fe_x_bytes(T, S, B, dout));
    return 0;
}

int vjf_forecast_ens_chunks(int32_t T, int32_t S, int32_t B, int32_t n, int32_t dout, int32_t* members, int32_t* steps) {
    if (!members || !steps || T < 1 || S < 1 || B < 1 || n < 1 || dout < 1) return fail(-20, "vjf_forecast_ens_chunks: bad argument");
    const FeChunks ch = fe_chunks(T, S, B, n, dout);
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
    hipStream_t s = (hipStream_t)stream;
    const int du = d - dout;
    if (!dec_W) dy = 0;
    if (vjf_fc_lds_floats(n, d, dout, false) * 4 > kMaxLds - 1024) return fail(-11, "vjf_forecast_ens: n=%d, d=%d too large", n, d);
    // the forms of the roll-out as vjf_forecast_seq chooses them; VJF_FC_CENTROID_LDS=0 also takes the decoder out of LDS and
    // VJF_FC_LOOKAHEAD=0 the batched staging out of the moments kernel (tests: the forms for large shapes, at any shape)
    const bool cl = vjf_fc_lds_floats(n, d, dout, true) * 4 <= kMaxLds - 1024 && fc_env_on("VJF_FC_CENTROID_LDS");
    const bool la = cl && n <= 64 * VJF_FC_KQ && dout <= 32 && fc_env_on("VJF_FC_LOOKAHEAD");
    const int mb = vjf_fe_lds_floats(dout, VJF_FE_BATCH, false) * 4 <= kMaxLds / 4 && fc_env_on("VJF_FC_LOOKAHEAD") ? VJF_FE_BATCH : 1;
    const bool dl = dy > 0 && vjf_fe_lds_floats(dout, mb, true) * 4 <= kMaxLds / 2 && fc_env_on("VJF_FC_CENTROID_LDS");
    const size_t lds_m = vjf_fe_lds_floats(dout, mb, dl) * 4;
    if (lds_m > kMaxLds - 1024) return fail(-11, "vjf_forecast_ens: dout=%d too large", dout);
    const size_t lds = vjf_fc_lds_floats(n, d, dout, cl) * 4, lds_w = (size_t)n * VJF_LDT * 4;
    const size_t wstep = (size_t)n * dout, xstep = (size_t)B * dout, ystep = (size_t)B * dy;
    const int tiles = (B + 15) / 16, mt = (n + 15) / 16, zg = ((dout + 15) / 16 + (dy + 15) / 16 + VJF_FE_GROUP - 1) / VJF_FE_GROUP;

    // rows r0 .. r0 + rows - 1 of the outputs from `rows` rows of states of members ms0 .. ms0 + Sc - 1
    auto moments = [&](const float* xs, size_t xs_ms, int r0, int rows, int ms0, int Sc) {
        VjfFeMomArgs m{};
        m.xs = xs; m.xs_ms = xs_ms; m.dec_W = dec_W; m.dec_b = dec_b;
        m.x_mean = x_mean + (size_t)r0 * xstep; m.x_var = x_var + (size_t)r0 * xstep;
        m.y_mean = dy ? y_mean + (size_t)r0 * ystep : nullptr; m.y_var = dy ? y_var + (size_t)r0 * ystep : nullptr;
        m.Sc = Sc; m.ms0 = ms0; m.S = S; m.last = ms0 + Sc == S; m.B = B; m.dout = dout; m.dy = dy; m.mb = mb;
        if (dl) {
            allow_lds(vjf_fe_moments_kernel<true>, lds_m);
            hipLaunchKernelGGL(vjf_fe_moments_kernel<true>, dim3(tiles, rows, zg), dim3(VJF_FE_THREADS), lds_m, s, m);
        } else {
            allow_lds(vjf_fe_moments_kernel<false>, lds_m);
            hipLaunchKernelGGL(vjf_fe_moments_kernel<false>, dim3(tiles, rows, zg), dim3(VJF_FE_THREADS), lds_m, s, m);
        }
    };
    if (T == 0) {                                        // nothing to roll out: the moments of the starts (x_members is not written)
        moments(x0, (size_t)x0_member_stride, 0, 1, 0, S);
        VJF_HIP(hipGetLastError());
        return 0;
    }
    const FeChunks ch = fe_chunks(T, S, B, n, dout);
    if ((size_t)ch.Sc * ch.Tc * wstep * 4 + (size_t)4 * dout * 4 > fe_w_bytes(T, S, n, dout) ||
        (size_t)ch.Sc * (ch.Tc + 1) * xstep * 4 > fe_x_bytes(T, S, B, dout))
        return fail(-11, "vjf_forecast_ens: a chunk of %d members x %d steps is beyond the scratch", ch.Sc, ch.Tc);
    float* W = (float*)scratch;
    float* X = (float*)((char*)scratch + fe_w_bytes(T, S, n, dout));
    // the members' states of a chunk: in x_members where they are kept, else in the scratch, (ch.Tc + 1) rows per member
    const size_t xs_ms = x_members ? (size_t)(T + 1) * xstep : (size_t)(ch.Tc + 1) * xstep;
    allow_lds(vjf_fe_weights_kernel, lds_w);
    for (int32_t ms0 = 0; ms0 < S; ms0 += ch.Sc) {
        const int Sc = S - ms0 < ch.Sc ? S - ms0 : ch.Sc;
        int Tp = 0;                                      // steps of the previous chunk
        for (int32_t t0 = 0; t0 < T; t0 += ch.Tc) {
            const int Tc = T - t0 < ch.Tc ? T - t0 : ch.Tc;
            VjfFeWeightArgs wa{w_mean, w_chol, w_noise + ((size_t)ms0 * T + t0) * wstep, W, (size_t)T * wstep, Sc, Tc, n, dout};
            const int64_t nq = (int64_t)Sc * Tc;
            int64_t gy = (nq + VJF_FC_WAVES - 1) / VJF_FC_WAVES, cap = 2048 / mt;
            if (gy > cap) gy = cap;
            if (gy < 1) gy = 1;
            hipLaunchKernelGGL(vjf_fe_weights_kernel, dim3(mt, (unsigned)gy), dim3(VJF_FC_THREADS), lds_w, s, wa);
            VJF_HIP(hipGetLastError());
            // row 0 of the chunk's states is x[t0] (the start, or the previous chunk's last row), rows 1 .. Tc are x[t0 + 1 ..]
            float* rows = x_members ? x_members + (size_t)ms0 * xs_ms + (size_t)t0 * xstep : X;
            VjfFeArgs e{};
            VjfFcArgs& a = e.a;
            if (t0 == 0) { a.x_in = x0 + (size_t)ms0 * x0_member_stride; e.x_in_ms = (size_t)x0_member_stride; a.x0_out = rows; e.x0_out_ms = xs_ms; }
            else { a.x_in = x_members ? rows : X + (size_t)Tp * xstep; e.x_in_ms = xs_ms; a.x0_out = nullptr; }
            a.u = u ? u + (size_t)t0 * B * du : nullptr;
            a.e = s_noise ? s_noise + ((size_t)ms0 * T + t0) * xstep : nullptr; e.e_ms = (size_t)T * xstep;
            a.c = centroid; a.logw = logwidth; a.W = W; e.W_ms = (size_t)Tc * wstep; a.tr_logvar = tr_logvar;
            a.x_out = rows + xstep; e.x_out_ms = xs_ms;
            a.Tc = Tc; a.B = B; a.n = n; a.d = d; a.dout = dout;
            auto launch = [&](auto kernel) {
                allow_lds(kernel, lds);
                hipLaunchKernelGGL(kernel, dim3(tiles, Sc), dim3(VJF_FC_THREADS), lds, s, e);
            };
            if (la && dout <= 16) launch(vjf_fe_rollout_kernel<1, true>);
            else if (la) launch(vjf_fe_rollout_kernel<2, true>);
            else if (cl) launch(vjf_fe_rollout_kernel<0, true>);
            else launch(vjf_fe_rollout_kernel<0, false>);
            VJF_HIP(hipGetLastError());
            if (t0 == 0) moments(rows, xs_ms, 0, Tc + 1, ms0, Sc);
            else moments(rows + xstep, xs_ms, t0 + 1, Tc, ms0, Sc);
            VJF_HIP(hipGetLastError());
            Tp = Tc;
        }
    }
    return 0;
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
    hipStream_t s = (hipStream_t)stream;
    VjfPlan P; rls_plan(n, dout, &P);
    const size_t lds = vjf_serial_lds_floats(P) * 4;
    if (lds > kMaxLds - 1024) return fail(-11, "vjf_blr_rls: n=%d too large for the single-workgroup RLS kernel", n);
    RlsCarve c{};
    float* red = nullptr;
    if (int rc = rls_statistics(P, scratch, x, centroid, logwidth, target, B, n, d, dout, s, &c, &red)) return rc;
    char* ws = (char*)scratch;
    allow_lds(vjf_rls_kernel, lds);
    VjfRlsArgs a{};
    a.Pm = w_precision; a.Wm = w_mean; a.Wc = w_chol; a.Lm = w_pchol;
    a.G = red + P.red_G; a.FDX = red + P.red_FDX; a.v = v; a.work = (float*)(ws + c.work); a.status = status;
    a.n = n; a.dout = dout; a.shrink = shrink;
    hipLaunchKernelGGL(vjf_rls_kernel, dim3(1), dim3(VJF_K2_THREADS), lds, s, a);
    VJF_HIP(hipGetLastError());
    return 0;
}

int vjf_kalman_scratch_size(int32_t B, int32_t n, int32_t dout, int64_t* bytes) {
    if (!bytes || B < 1 || n < 1 || dout < 1) return fail(-20, "vjf_kalman_scratch_size: bad argument");
    const size_t nn = ((size_t)n * (n > dout ? n : dout) * 4 + 255) / 256 * 256;
    *bytes = (int64_t)(rls_carve(B, n, dout, nullptr).total + 6 * nn);
    return 0;
}

int vjf_blr_kalman(const float* x, const float* target, const float* v, float diffusion, const float* centroid, const float* logwidth,
                   float* w_mean, float* w_chol, void* scratch, uint32_t* status, int32_t B, int32_t n, int32_t d, int32_t dout,
                   void* stream) {
    if (!x || !target || !v || !centroid || !logwidth || !w_mean || !w_chol || !scratch) return fail(-1, "vjf_blr_kalman: null tensor");
    if (B < 1 || n < 1 || d < 1 || dout < 1) return fail(-20, "vjf_blr_kalman: bad shape");
    if (!(diffusion >= 0.f)) return fail(-25, "vjf_blr_kalman: diffusion needs to be non-negative");   // module.py:127
    hipStream_t s = (hipStream_t)stream;
    VjfPlan P; rls_plan(n, dout, &P);
    const size_t lds = vjf_serial_lds_floats(P) * 4;
    if (lds > kMaxLds - 1024) return fail(-11, "vjf_blr_kalman: n=%d too large for the single-workgroup kernel", n);
    RlsCarve c{};
    float* red = nullptr;
    if (int rc = rls_statistics(P, scratch, x, centroid, logwidth, target, B, n, d, dout, s, &c, &red)) return rc;
    char* ws = (char*)scratch;
    allow_lds(vjf_kalman_kernel, lds);
    const size_t nn = ((size_t)n * (n > dout ? n : dout) * 4 + 255) / 256 * 256;
    VjfKalmanArgs a{};
    a.Wm = w_mean; a.Wc = w_chol; a.G = red + P.red_G; a.Fy = red + P.red_FDX; a.v = v;
    for (int q = 0; q < 6; ++q) a.T[q] = (float*)(ws + c.total + (size_t)q * nn);
    a.Dinv = (float*)(ws + c.work);
    a.status = status; a.n = n; a.dout = dout; a.diffusion = diffusion;
    hipLaunchKernelGGL(vjf_kalman_kernel, dim3(1), dim3(VJF_K2_THREADS), lds, s, a);
    VJF_HIP(hipGetLastError());
    return 0;
}

namespace {
// vjf_recognition_forward(_act): act null or Tanh -> the Tanh kernel
int recognition_forward(const char* who, const float* y, const float* u, const float* mu_s, const float* lv_s, const float* const* rec_W,
                        const float* const* rec_b, const float* mean_W, const float* lv_W, const float* lv_b, float* mu_t,
                        float* lv_t, int32_t B, int32_t ydim, int32_t udim, int32_t xdim, int32_t n_hidden,
                        const int32_t* hidden, const VjfAct* act, void* stream) {
    if (!y || !mu_s || !lv_s || !rec_W || !rec_b || !mean_W || !lv_W || !lv_b || !mu_t || !lv_t || !hidden)
        return fail(-1, "%s: null tensor", who);
    if (udim > 0 && !u) return fail(-21, "%s: u is required when udim > 0", who);
    if (n_hidden < 1 || n_hidden > VJF_MAX_HIDDEN) return fail(-3, "%s: n_hidden=%d", who, n_hidden);
    if (B < 1) return fail(-20, "%s: bad shape", who);
    VjfRecArgs a{};
    a.y = y; a.u = u; a.mu_s = mu_s; a.lv_s = lv_s; a.mean_W = mean_W; a.lv_W = lv_W; a.lv_b = lv_b; a.mu_t = mu_t; a.lv_t = lv_t;
    a.B = B; a.dy = ydim; a.du = udim; a.dz = xdim; a.L = n_hidden;
    int hmax = 0;
    for (int l = 0; l < n_hidden; ++l) { a.W[l] = rec_W[l]; a.b[l] = rec_b[l]; a.h[l] = hidden[l]; if (hidden[l] > hmax) hmax = hidden[l]; }
    const size_t lds = (size_t)VJF_LDT * (ydim + udim + 2 * xdim + 2 * hmax) * 4;
    if (lds > kMaxLds - 1024) return fail(-10, "%s: layer widths do not fit LDS", who);
    with_act_kernel(act ? *act : VjfAct{VJF_ACT_TANH, 0.f, 0.f}, vjf_recognition_kernel, vjf_recognition_act_kernel, [&](auto kernel, auto... tail) {
        allow_lds(kernel, lds);
        hipLaunchKernelGGL(kernel, dim3((B + 15) / 16), dim3(VJF_K1_THREADS), lds, (hipStream_t)stream, a, hmax, tail...);
    });
    VJF_HIP(hipGetLastError());
    return 0;
}
}  // namespace

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
    hipLaunchKernelGGL(vjf_loss_kernel, dim3(VJF_LOSS_BLOCKS), dim3(256), 0, (hipStream_t)stream, 0, m1, lv1, m2, lv2, logvar, out, B, d, loss_slot());
    VJF_HIP(hipGetLastError());
    return 0;
}

int vjf_gaussian_entropy(const float* lv, float* out, int32_t B, int32_t d, void* stream) {
    if (!lv || !out) return fail(-1, "vjf_gaussian_entropy: null tensor");
    if (B < 1 || d < 1) return fail(-20, "vjf_gaussian_entropy: bad shape");
    hipLaunchKernelGGL(vjf_loss_kernel, dim3(VJF_LOSS_BLOCKS), dim3(256), 0, (hipStream_t)stream, 1, lv, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, out, B, d, loss_slot());
    VJF_HIP(hipGetLastError());
    return 0;
}

int vjf_poisson_loss(const float* eta, const float* target, float* out, int32_t B, int32_t d, void* stream) {
    if (!eta || !target || !out) return fail(-1, "vjf_poisson_loss: null tensor");
    if (B < 1 || d < 1) return fail(-20, "vjf_poisson_loss: bad shape");
    hipLaunchKernelGGL(vjf_loss_kernel, dim3(VJF_LOSS_BLOCKS), dim3(256), 0, (hipStream_t)stream, 2, eta, (const float*)nullptr, target,
                       (const float*)nullptr, (const float*)nullptr, out, B, d, loss_slot());
    VJF_HIP(hipGetLastError());
    return 0;
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
