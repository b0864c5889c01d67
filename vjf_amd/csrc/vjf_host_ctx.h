// vjf_host_ctx.h -- host side of vjf_abi.hip: errors, the RCCL loader, what the contexts of a device share, the workspace carve, the
// context itself (its typed workspace accessors), and the choice of kernel instantiations.  Included by vjf_abi.hip only.
#pragma once

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define VJF_HIP(call)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return fail(-100, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Launch; with `stop` non-null the event rides on the kernel's own completion signal (no marker packet behind it)
#define VJF_LAUNCH(kernel, grid, block, lds, st, stop, ...)                                             \
    do {                                                                                               \
        if (stop) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)(lds), st, nullptr, stop, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);                            \
    } while (0)

// ---- RCCL, resolved at run time from the copy already in the process (torch's) or librccl.so: the library has no link-time
//      dependency on it, and a single-GPU user never touches it
struct VjfNcclId { char internal[128]; };
typedef int (*nccl_get_unique_id_t)(VjfNcclId*);
typedef int (*nccl_comm_init_rank_t)(void**, int, VjfNcclId, int);
typedef int (*nccl_comm_destroy_t)(void*);
typedef int (*nccl_all_reduce_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_group_t)();
typedef int (*nccl_comm_count_t)(void*, int*);
typedef const char* (*nccl_err_t)(int);
struct VjfNccl {
    nccl_get_unique_id_t get_unique_id; nccl_comm_init_rank_t comm_init_rank; nccl_comm_destroy_t comm_destroy;
    nccl_all_reduce_t all_reduce; nccl_group_t group_start, group_end; nccl_err_t err;
    nccl_comm_count_t comm_count;
    bool ok;
};
constexpr int kNcclFloat = 7, kNcclSum = 0;        // ncclFloat32, ncclSum (rccl.h)
const VjfNccl& nccl() {
    static VjfNccl n = [] {
        VjfNccl v{};
        void* h = RTLD_DEFAULT;
        if (!dlsym(h, "ncclAllReduce")) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return v;
        v.get_unique_id = (nccl_get_unique_id_t)dlsym(h, "ncclGetUniqueId");
        v.comm_init_rank = (nccl_comm_init_rank_t)dlsym(h, "ncclCommInitRank");
        v.comm_destroy = (nccl_comm_destroy_t)dlsym(h, "ncclCommDestroy");
        v.all_reduce = (nccl_all_reduce_t)dlsym(h, "ncclAllReduce");
        v.group_start = (nccl_group_t)dlsym(h, "ncclGroupStart");
        v.group_end = (nccl_group_t)dlsym(h, "ncclGroupEnd");
        v.err = (nccl_err_t)dlsym(h, "ncclGetErrorString");
        v.comm_count = (nccl_comm_count_t)dlsym(h, "ncclCommCount");
        v.ok = v.get_unique_id && v.comm_init_rank && v.comm_destroy && v.all_reduce && v.group_start && v.group_end;
        return v;
    }();
    return n;
}
#define VJF_NCCL(call)                                                                           \
    do {                                                                                         \
        int e_ = (call);                                                                         \
        if (e_ != 0) return fail(-110, "%s failed: %s", #call, nccl().err ? nccl().err(e_) : "rccl error"); \
    } while (0)

// ---- the environment variables the library reads, and when (tests flip the per-call ones between calls)
//   vjf_ctx_create:    VJF_HANDOFF_ACQUIRE, VJF_COLLECTIVES;  vjf_comm_init: VJF_DEBUG_FAKE_WORLD
//   every call:        VJF_DEBUG_REFUSE_COOP, VJF_DEBUG_ABSENT, VJF_DEBUG_INJECT (filter_seq_mega), VJF_DEBUG_RLSC_ABSENT (launch_rlsb),
//                      VJF_SEQ_CHUNK (seq_chunk), VJF_DEBUG_TWO_TIMELINE (filter_seq_two); the chaos build: VJF_CHAOS_* (chaos_refresh);
//                      VJF_FC_CHUNK, VJF_FE_MEMBERS (the entry points vjf_forecast_seq / _ens / _ens_chunks, which hand them to the planners),
//                      VJF_FC_LOOKAHEAD, VJF_FC_CENTROID_LDS (fc_forms / fe_mom_forms, called by those entry points; vjf_host_forecast.h);
//                      VJF_FC_CHUNK, VJF_FC_LOOKAHEAD, VJF_FC_CENTROID_LDS also by vjf_tangent_rollout / _plan (handed to tg_plan, tg_chunk)
//   once per process:  VJF_RLS_COLUMN_LAUNCHES (launch_rlsb), VJF_NO_MOMENTS_ROLE (mega_shape)

constexpr size_t kMaxLds = 160 * 1024;

// ---- what the contexts of a process share, per device
//  * the chain of one-launch grids: such a grid must be resident as a whole (every workgroup wants a whole compute unit's LDS), so
//    two of them -- two models on two streams -- must never be dispatched side by side: each launch waits for the completion event
//    of the previous one, whatever context and stream that came from.  While a device has a single context with the route the
//    stream's own order does this and no event is used; the second context's creation synchronises the device once and switches
//    the chain on for good.
//  * a page of pinned host memory through which a launch that has given up a wait tells the host (VJF_MIRROR_SLOT, vjf_plan.h; the waits themselves: vjf_handoff.h).
struct DevShared {
    std::mutex mu;
    int mega_ctxs = 0;          // live contexts whose plan the one-launch route serves
    bool chained = false;
    hipEvent_t last = nullptr;  // completion of the most recent one-launch grid on this device
    hipStream_t last_stream = nullptr;
    bool last_valid = false;
    unsigned* mirror_h = nullptr;   // the page of pinned host memory (VJF_MIRROR_WORDS words) ...
    unsigned* mirror_d = nullptr;   // ... as the device addresses it
};
constexpr int kMaxDevices = 64;
DevShared g_dev[kMaxDevices];
DevShared* dev_shared(int device) { return device >= 0 && device < kMaxDevices ? &g_dev[device] : nullptr; }

int plan_for(const char* who, const vjf_config* cfg, VjfPlan* P) {
    const int rc = vjf_make_plan(cfg, P);
    return rc ? fail(rc, "%s: invalid config (%d)", who, rc) : 0;
}

int split_for(int B) {
    int s = B / 256;
    if (s < 1) s = 1;
    if (s > 64) s = 64;
    return s;
}

void build_jobs(const VjfPlan& P, std::vector<VjfJob>& jobs) {
    jobs.clear();
    // kind 0: lower tiles of E^T E that touch Phi columns
    const int nt = P.ldE / VJF_TILE;
    for (int ti = 0; ti < nt; ++ti)
        for (int tj = 0; tj <= ti; ++tj) {
            if (tj * VJF_TILE >= P.n) continue;                 // dx x dx tiles are not needed
            if (ti * VJF_TILE >= P.n + P.dz) continue;          // pure padding rows
            VjfJob j{};
            j.kind = 0; j.xc = ti * VJF_TILE; j.yc = tj * VJF_TILE; j.xn = VJF_TILE; j.yn = VJF_TILE;
            j.ti = ti; j.tj = tj; j.dst = 0; j.ld = 0; j.ncol_w = 0; j.dst_b = -1;
            jobs.push_back(j);
        }
    // kind 1: DEL[:, xcol..+M]^T ACT[:, ycol..+K+1]  ->  weight (M,K) + bias (M)
    auto tensor_of = [&](int slot) {
        for (int t = 0; t < P.n_train; ++t) if (P.tr_off[t] == P.off[slot]) return t;
        return -1;
    };
    auto grad = [&](int xcol, int M, int ycol, int K, int slotW, int slotB) {
        const int offW = P.off[slotW] - P.train_off;
        const int offB = slotB >= 0 ? P.off[slotB] - P.train_off : -1;
        const int tW = tensor_of(slotW), tB = slotB >= 0 ? tensor_of(slotB) : -1;
        const int ncols = K + 1;
        for (int ri = 0; ri * VJF_TILE < M; ++ri)
            for (int ci = 0; ci * VJF_TILE < ncols; ++ci) {
                VjfJob j{};
                j.kind = 1;
                j.xc = xcol + ri * VJF_TILE; j.xn = M - ri * VJF_TILE < VJF_TILE ? M - ri * VJF_TILE : VJF_TILE;
                j.yc = ycol + ci * VJF_TILE; j.yn = ncols - ci * VJF_TILE < VJF_TILE ? ncols - ci * VJF_TILE : VJF_TILE;
                j.dst = offW + ri * VJF_TILE * K + ci * VJF_TILE;
                j.ld = K;
                int nw = K - ci * VJF_TILE;
                j.ncol_w = nw < 0 ? 0 : (nw > VJF_TILE ? VJF_TILE : nw);
                j.dst_b = offB >= 0 ? offB + ri * VJF_TILE : -1;
                j.tw = tW; j.tb = tB;
                jobs.push_back(j);
            }
    };
    int prev = P.din;
    for (int l = 0; l < P.L; ++l) {
        grad(P.colD_da[l], P.h[l], P.colA_act[l], prev, VJF_SLOT_REC_W0 + 2 * l, VJF_SLOT_REC_B0 + 2 * l);
        prev = P.h[l];
    }
    grad(P.colD_dmu, P.dz, P.colA_act[P.L], prev, VJF_SLOT_MEAN_W, -1);
    grad(P.colD_dlv, P.dz, P.colA_act[P.L], prev, VJF_SLOT_LV_W, VJF_SLOT_LV_B);
    grad(P.colD_dpy, P.dy, P.colA_xt, P.dz, VJF_SLOT_DEC_W, VJF_SLOT_DEC_B);
}

// ---- the one-launch route (vjf_mega_kernel.h): which plans it serves and how the grid's workgroups are dealt to its roles
constexpr size_t kMegaLds = kMaxLds - 512;             // dynamic LDS of every workgroup of the launch (one workgroup per CU)
constexpr int kMegaMaxTrialWg = 256, kMegaMaxGramWg = 64;
struct MegaShape { int n_rls, n_trial, n_gram, n_prep, n_sgd, ntiles, gram_rows, n_mom; };
constexpr int kMegaRefused = 1 << 20;                  // filter_seq_mega: the grid cannot be resident as a whole (not an error code of the ABI)

bool mega_plan_ok(const VjfPlan& P) {
    const int nbl = (P.n + 31) / 32;
    if (!vjf_chol_lds_ok(P) || P.dz > 16 || nbl > VJF_CHOL_MAXBLK) return false;          // LDS Cholesky loop + y / W and inverse loops
    if (vjf_chol_lds_bytes(P, 16) > kMegaLds) return false;                               // vjf_chol_loop<16>
    if (vjf_post_lds_bytes(P) > kMegaLds) return false;
    if ((size_t)vjf_mega_trial_lds(P).total * 4 > kMegaLds) return false;                 // 32 trials' working set
    if (vjf_mega_gram_lds_floats(P) * 4 > kMegaLds || vjf_mega_prep_lds_floats(P) * 4 > kMegaLds) return false;
    if (vjf_mega_mom_lds_floats(P) * 4 > kMegaLds) return false;
    if (P.du > 16) return false;                                                         // (one element of a 32 x du tile per thread)
    if (nbl * (nbl + 1) / 2 > VJF_MG_WAVES * VJF_MG_MAXQ) return false;
    return true;
}

bool mega_shape(const VjfPlan& P, int B, int ncu, uint32_t flags, MegaShape* m) {
    // one workgroup per compute unit: the RLS loops and the operand role have fixed sizes; the trial role gets 128 / 227 of the
    // rest (one 32-trial tile per workgroup at 256 CUs and 4096 trials), then the SGD role (below), the Gram role whatever remains
    const int nbl = (P.n + 31) / 32;
    const bool rls = (flags & (VJF_FLAG_UPDATE | VJF_FLAG_WARM_UP)) == VJF_FLAG_UPDATE;   // (else: no RLS, Gram, operand roles)
    m->n_rls = rls ? 2 + 2 * nbl : 0;
    m->n_prep = rls ? (P.n + 15) / 16 : 0;
    m->ntiles = (B + VJF_MG_TR - 1) / VJF_MG_TR;
    m->n_mom = 0;
    const int rest = ncu - m->n_rls - m->n_prep;
    if (rest < 3) return false;
    if (!rls) {
        // trial + SGD roles only: the SGD role as many workgroups as its fewest rounds of slab loads need (they also build the
        // parameter image at the start of the launch), the trial role the rest
        const int quads = vjf_mega_slab_layout(P).len / 4, gpw = VJF_MG_THREADS / 8;
        int want = (quads + gpw - 1) / gpw;
        if (!(flags & VJF_FLAG_SGD) && want > 16) want = 16;          // (no gradient steps: these only build the parameter image at the start)
        if (want > rest / 4) want = rest / 4;
        if (want < 1) want = 1;
        m->n_sgd = want;
        int cap = rest - m->n_sgd;
        if (cap > kMegaMaxTrialWg) cap = kMegaMaxTrialWg;
        m->n_trial = m->ntiles < cap ? m->ntiles : cap;
        m->n_gram = 0; m->gram_rows = 0;
        // the moments role (vjf_mega_moments): the compute units that are left, when they can keep up -- a tile takes such a workgroup
        // about as long as the rest of the step takes the trial role, so at most two tiles each; else the trial role forms its
        // moments itself
        {
            static const bool off = getenv("VJF_NO_MOMENTS_ROLE") != nullptr;    // (A/B)
            int nm = rest - m->n_sgd - m->n_trial;
            if (nm > m->ntiles) nm = m->ntiles;
            if (!(flags & (VJF_FLAG_SGD | VJF_FLAG_UPDATE))) nm += m->n_sgd;        // (the image builders go on as moments workgroups)
            if (nm > m->ntiles) nm = m->ntiles;
            if (!off && nm >= 1 && 2 * nm >= m->ntiles && m->ntiles <= VJF_MG_TAG_TILES && m->n_trial == m->ntiles) m->n_mom = nm;
            if (m->n_mom > 0 && m->n_sgd > m->n_mom && !(flags & (VJF_FLAG_SGD | VJF_FLAG_UPDATE))) m->n_sgd = m->n_mom;
        }
        return true;
    }
    int cap_t = rest * 128 / 227;
    if (cap_t < 1) cap_t = 1;
    if (cap_t > kMegaMaxTrialWg) cap_t = kMegaMaxTrialWg;
    m->n_trial = m->ntiles < cap_t ? m->ntiles : cap_t;
    if (m->ntiles > cap_t) {
        // More tiles than the trial role's usual share of the chip (B > 4096 at 256 compute units: BASELINE configs[3] on ONE GPU has
        // 1024): the step is then the trial role's tiles in sequence (~41 us each) plus the SGD role's loop, and the other roles have
        // slack -- the SGD role may take two or three rounds of slab loads (+7 us each, once per step), the Gram role several
        // passes of rows (22 us each, a step ahead).  The fewest tiles per trial workgroup that leave those two enough workgroups:
        const int quads = vjf_mega_slab_layout(P).len / 4, gpw = VJF_MG_THREADS / 8, want = (quads + gpw - 1) / gpw;
        int big_sgd = 0, big_gram = 0;
        for (int ntl = (m->ntiles + cap_t - 1) / cap_t; ntl >= 1; --ntl) {
            int nt = (m->ntiles + ntl - 1) / ntl;
            if (nt > kMegaMaxTrialWg || nt > rest - 2) break;
            bool found = false;
            for (int rounds = 1; rounds <= 3 && !found; ++rounds) {
                const int ns = (want + rounds - 1) / rounds;
                int ng = rest - nt - ns;
                if (ng > kMegaMaxGramWg) ng = kMegaMaxGramWg;
                if (ng < nbl * (nbl + 1) / 2) continue;                        // (one Gram workgroup per lower tile at least: the slab sum's shares)
                const int passes = ((B + ng - 1) / ng + VJF_MG_GROWS - 1) / VJF_MG_GROWS;
                const double cycle = 41.0 * ntl + 12.0 + 7.0 * (rounds - 1), gram = 22.0 * passes + 17.0;
                if (gram <= 0.95 * cycle) { m->n_trial = nt; big_sgd = ns; big_gram = ng; found = true; }
            }
            if (!found) break;
        }
        if (big_sgd > 0) {
            m->n_sgd = big_sgd; m->n_gram = big_gram;
            m->gram_rows = ((B + m->n_gram - 1) / m->n_gram + 1) & ~1;
            return true;
        }
    }
    const int left = rest - m->n_trial;                                               // >= 2
    // SGD role: one 8-lane group per quad of the late slab and ROUND of slab loads; its time is the bytes of the slabs over the
    // compute units it has (a unit takes in ~33 GB/s of slabs written on other XCDs), so the fewest rounds win.  The Gram role
    // runs a step ahead with slack: if a second pass of rows per Gram workgroup (fewer of them) saves the SGD role a round, take
    // it; the SGD role then gets just the workgroups that round count needs, the Gram role the rest.
    const int quads = vjf_mega_slab_layout(P).len / 4, gpw = VJF_MG_THREADS / 8;          // lane groups per workgroup
    auto rounds = [&](int nwg) { return (quads + gpw * nwg - 1) / (gpw * nwg); };
    auto clampg = [&](int g) { if (g > left / 2) g = left / 2; return g < 1 ? 1 : g; };
    const int want = (quads + gpw - 1) / gpw;
    const int g1 = clampg((B + VJF_MG_GROWS - 1) / VJF_MG_GROWS), g2 = clampg((B + 2 * VJF_MG_GROWS - 1) / (2 * VJF_MG_GROWS));
    const int n1 = want < left - g1 ? want : left - g1, n2 = want < left - g2 ? want : left - g2;
    const int r = rounds(n2 < 1 ? 1 : n2) < rounds(n1 < 1 ? 1 : n1) ? rounds(n2 < 1 ? 1 : n2) : rounds(n1 < 1 ? 1 : n1);
    m->n_sgd = (quads + gpw * r - 1) / (gpw * r);                                         // the fewest workgroups with that many rounds
    if (m->n_sgd > left - g2) m->n_sgd = left - g2;
    if (m->n_sgd < 1) m->n_sgd = 1;
    m->n_gram = (B + 63) / 64;
    // (at least one Gram workgroup per lower tile of Phi^T Phi, rows or not: the slab sum deals its quads over the role's
    //  workgroups, two per thread and ROUND TRIP -- one workgroup alone took ten of them for the ten tiles of RBF(100), and at
    //  one trial that loop, 35 us, was the step; compute units are idle at such batch sizes)
    { const int ntri = nbl * (nbl + 1) / 2; if (m->n_gram < ntri) m->n_gram = ntri; }
    if (m->n_gram > left - m->n_sgd) m->n_gram = left - m->n_sgd;
    if (m->n_gram > kMegaMaxGramWg) m->n_gram = kMegaMaxGramWg;
    if (m->n_gram < 1) m->n_gram = 1;
    m->gram_rows = ((B + m->n_gram - 1) / m->n_gram + 1) & ~1;
    return true;
}

struct Carve {
    size_t pscr; size_t mg_mom, mg_xt, mg_early, mg_late, mg_gslab, mg_cnt, mg_stamps, mg_pidx, mg_cidx, mg_grp, mg_img, mg_pmsave; size_t E, E2, ACT, DEL, partial, partial2, slabs, red, red2, red3, tbig, wide, work, jobs, aux, post, lscr, flags, resid, total;
};

Carve carve_ws(const VjfPlan& P, int max_batch, int njobs) {
    Carve c{};
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = (o + bytes + 255) / 256 * 256; return at; };
    c.E = take((size_t)max_batch * P.ldE * 4);
    c.E2 = take((size_t)max_batch * P.ldE * 4);            // odd steps' E rows in the multi-stream sequence
    c.ACT = take((size_t)max_batch * P.ldA * 4);
    c.DEL = take((size_t)max_batch * P.ldD * 4);
    c.partial = take(((size_t)max_batch / 4 + 2) * RS_N * 4);
    c.partial2 = take(((size_t)max_batch / 4 + 2) * RS_N * 4);
    c.slabs = take((size_t)njobs * split_for(max_batch) * 1024 * 4);
    c.red = take((size_t)P.red_len * 4);
    c.red2 = take((size_t)P.red_len * 4);                  // RLS statistics of even / odd steps in the multi-stream sequence
    c.red3 = take((size_t)P.red_len * 4);
    c.tbig = take(P.n > 32 * VJF_CHOL_MAXBLK ? (size_t)((P.n + 31) / 32) * 1024 * 4 * 3 : 16);   // multi-launch RLS: the diagonal blocks of L, two sets of column sums
    // GEMM-per-layer trial path (working set beyond LDS): [xs|u], pt.mean, pt.logvar, decoder output, Phi w_chol per trial
    c.wide = take(vjf_trial_mfma_lds_floats(P) * 4 > kMaxLds - 1024 ? (size_t)max_batch * (P.dxu + P.dz + 1 + P.dy + P.n) * 4 + 1024 : 16);
    c.work = take(vjf_serial_work_floats(P) * 4 + 10 * 256);  // + 10 x 32 u64 diagnostic stamps (a ring over the steps of a sequence)
    c.post = take((size_t)((P.n + 31) / 32) * 1024 * 4 + VJF_RESID_BLOCKS * 8 + 64);   // Dinv blocks | resid partials | ok flag
    c.flags = take(256);                                   // column flags of the Cholesky -> post hand-off (a block of their own)
    c.lscr = take((size_t)P.n * P.n * 4);                  // L, column by column, from the Cholesky kernel to the post kernel
    c.pscr = take((size_t)(VJF_CHOL_MAXBLK * (VJF_CHOL_MAXBLK + 1) / 2) * 1024 * 4);   // lower blocks of P, from one Cholesky kernel to the next
    if (mega_plan_ok(P)) {                                 // slabs of the one-launch route, sized for the largest role counts
        const int nbl = (P.n + 31) / 32;
        const size_t slab_len = (size_t)vjf_mega_slab_layout(P).len;
        c.mg_early = take((size_t)2 * kMegaMaxTrialWg * ((size_t)((P.n + 3) & ~3) * 16 + 8) * 4);   // (two sets: even / odd steps)
        c.mg_late = take((size_t)kMegaMaxTrialWg * (slab_len + 8 * VJF_MG_RING) * 4);
        c.mg_gslab = take((size_t)kMegaMaxGramWg * (nbl * (nbl + 1) / 2) * 1024 * 4);
        c.mg_cnt = take((size_t)2 * MG_C_WORDS * 4);           // two counter blocks: a launch runs on one and zeroes the other for the next
        c.mg_stamps = take((32 * 32 + kMegaMaxTrialWg * 8) * 8);   // ring of role stamps | 8 words per trial workgroup (last step)
        c.mg_pidx = take(slab_len * 4); c.mg_cidx = take(slab_len * 4); c.mg_grp = take((size_t)(VJF_GT_AT((int)slab_len) + vjf_mega_grad_tiles(P, nullptr)) * 4);   // (+ the step's gradient tiles)
        c.mg_img = take((size_t)vjf_mega_trial_lds(P, (int)(kMegaLds / 4) - 8).th_len * 4 + 64);   // the parameters in the trial role's LDS layout
        c.mg_pmsave = take((size_t)max_batch * (P.dz + 1) * 4);
        c.mg_xt = take((size_t)P.n * P.n * 4);               // row-major L^-1 (= w_chol^T) for the trial role's 16-byte operand loads
        {   // moments role -> trial role: [tile][step parity][(2 dz + 1) x 32]
            int nt = (max_batch + VJF_MG_TR - 1) / VJF_MG_TR;
            if (nt > VJF_MG_TAG_TILES) nt = VJF_MG_TAG_TILES;
            c.mg_mom = take((size_t)nt * 2 * (2 * P.dz + 1) * VJF_MG_TR * 4);
        }
    }
    c.jobs = take((size_t)njobs * sizeof(VjfJob));
    c.aux = take((size_t)P.aux_len * 4);
    // multi-launch RLS on a stream of its own (filter_seq_two): Phi W of the state-noise update, beside the trial chain's DEL rows
    c.resid = take(P.n > 32 * VJF_CHOL_MAXBLK ? (size_t)max_batch * P.dz * 4 : 16);
    c.total = o;
    return c;
}

template <class K>
void allow_lds(K kernel, size_t bytes) {
    // raise the dynamic-LDS cap (kernels here use up to ~150 KiB of the CU's 160 KiB); a refusal is
    // not fatal by itself -- the launch reports it -- so clear the sticky error state
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    (void)hipGetLastError();
}

}  // namespace

struct vjf_ctx {
    vjf_config cfg{};
    VjfPlan plan{};
    float* state = nullptr;
    char* ws = nullptr;
    int64_t ws_bytes = 0;
    hipStream_t stream = nullptr;
    Carve cv{};
    int njobs = 0;
    size_t lds_k2 = 0;
    bool post_kernels = false;  // RLS tail (inverse, solve, residual) on many CUs beside / after the Cholesky kernel
    size_t lds_post = 0;
    bool mfma_trial = false;    // 16 trials' working set fits LDS: matrix-core trial kernel of the per-step routes
    size_t lds_k1m = 0;
    bool stamps = false;        // diagnostic: s_memrealtime phase stamps
    bool stamps_keep_overlap = false;
    bool fast_chol = false;     // n_rbf <= 224: prep kernel + LDS-resident MFMA Cholesky; else the generic serial kernel / multi-launch RLS
    size_t lds_chol = 0;
    int n_ejobs = 0;            // jobs [0, n_ejobs) are the E^T E tiles, the rest gradient tiles
    bool overlap = true;        // 1: single rank -> the one-launch route, ranks -> the three-stream per-step route; 0: one-stream order
    bool handoff_acquire = false;  // VJF_HANDOFF_ACQUIRE=1: the one-launch route's waits acquire at agent scope beside the sc1 loads (default: sc1 loads alone)
    bool force_streams = false; // vjf_set_overlap(ctx, 3): the three-stream per-step route on a single rank too (A/B measurements)
    bool mega_ok = false;       // the plan fits the one-launch route (vjf_mega_kernel.h)
    bool mega_plan = false;     // mega_plan_ok(plan): the route's tables exist (mega_ok also needs the residency check of the context's kernels)
    VjfAct act{VJF_ACT_TANH, 0.f, 0.f};   // activation of the recognition layers (vjf_set_activation; VJF_ACT_TANH: the Tanh kernels)
    bool ran = false;           // a vjf_filter_* call has run on the context (vjf_set_activation is refused from then on)
    int ncu = 0;                // compute units of the device: the one-launch grid has one workgroup per CU
    int mega_wg_per_cu = 0;     // workgroups of vjf_mega_kernel a compute unit can hold (occupancy query): the residency check of the route
    int lite_wg_per_cu = 0;     // the same for vjf_mega_lite_kernel (the launches without an RLS update)
    unsigned mega_launches = 0; // launches of vjf_mega_kernel so far: launch k counts in counter block k & 1
    hipStream_t stream2 = nullptr, stream3 = nullptr;
    hipEvent_t ev_s = nullptr, ev_c = nullptr;
    hipEvent_t ev_f[2] = {}, ev_r[2] = {}, ev_b[2] = {}, ev_g[2] = {};   // (ev_g: the RLS statistics) two-stream route of the multi-launch RLS plans: forward half / RLS update / backward half of even, odd steps
    unsigned epoch = 0;         // launches of the Cholesky / post pair so far (the hand-off flags carry it)
    unsigned k1_count = 0;      // workgroups of the matrix-core trial kernel (whole step or backward half) launched so far
    unsigned post_count = 0;    // workgroups of the post kernel launched so far
    unsigned fwd_count = 0;     // workgroups of forward halves launched with a completion count
    unsigned stats_count = 0;   // steps whose RLS statistics the three-stream route has launched (host mirror of flag word kStatsWord)
    unsigned start_count = 0;   // host mirror of the post kernel's "workgroups started" count
    bool mega_counted = false;  // counted in its device's DevShared::mega_ctxs
    bool on_mega = false;       // the context's last sequence ran on the one-launch route (a timed-out wait then makes it leave the route)
    void* comm_a = nullptr; void* comm_b = nullptr;   // RCCL communicators of the two chains of the three-stream route (null: single rank)
    int world = 1;
    int collectives = 2;        // sums over ranks per step on the in-library route: 2 (default) [grad | loss sums] and [G | Phi^T dx | sums], one on each
                                // chain of the three-stream schedule; 1 ONE all-reduce of the whole reduce buffer (SURVEY 8e's layout) between the
                                // trial-parallel and the serial half of a step, on one stream (vjf_set_collectives)
    int fake_world = 1;         // test hook (VJF_DEBUG_FAKE_WORLD=k at vjf_comm_init, one-rank communicators): behave as rank 0 of k ranks that
                                // all hold the same trials -- every all-reduced buffer is multiplied by k and B_total = k B

    // ---- the workspace, typed: the only place that adds an offset of the carve to `ws`.  A region of the carve under its own name;
    //      `gen`: the buffers that alternate between even and odd steps of the multi-stream sequences
    template <class T> T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
#define VJF_WS_REGION(T, name) T* name() const { return at<T>(cv.name); }
    VJF_WS_REGION(float, ACT) VJF_WS_REGION(float, DEL) VJF_WS_REGION(float, slabs) VJF_WS_REGION(float, tbig) VJF_WS_REGION(float, wide)
    VJF_WS_REGION(float, work) VJF_WS_REGION(float, aux) VJF_WS_REGION(float, lscr) VJF_WS_REGION(float, pscr) VJF_WS_REGION(float, resid)
    VJF_WS_REGION(float, red)                                               // gradients + loss sums, or the whole reduce buffer
    VJF_WS_REGION(VjfJob, jobs)
    VJF_WS_REGION(float, mg_mom) VJF_WS_REGION(float, mg_xt) VJF_WS_REGION(float, mg_early) VJF_WS_REGION(float, mg_late) VJF_WS_REGION(float, mg_gslab)
    VJF_WS_REGION(float, mg_img) VJF_WS_REGION(float, mg_pmsave) VJF_WS_REGION(int, mg_pidx) VJF_WS_REGION(int, mg_cidx) VJF_WS_REGION(int, mg_grp)
#undef VJF_WS_REGION
    int* mg_gtab() const { return mg_grp() + VJF_GT_AT(vjf_mega_slab_layout(plan).len); }   // the gradient-tile table, behind the group words
    float* E(int gen = 0) const { return at<float>(gen ? cv.E2 : cv.E); }
    float* partial(int gen = 0) const { return at<float>(gen ? cv.partial2 : cv.partial); }
    float* red_rls(int gen) const { return at<float>(gen ? cv.red3 : cv.red2); }   // RLS statistics of even / odd steps
    float* status_word() const { return state + plan.off[VJF_SLOT_SCALARS] + VJF_SC_STATUS; }   // VJF_STATUS_* bits, as a float
    unsigned* flag_words() const { return at<unsigned>(cv.flags); }         // the flag block (vjf_host_launch.h names its words)
    // the `post` region: Dinv blocks | residual partials | ok flag
    size_t dinv_bytes() const { return (size_t)((plan.n + 31) / 32) * 1024 * 4; }
    float* dinv() const { return at<float>(cv.post); }
    double* resid_partial() const { return at<double>(cv.post + dinv_bytes()); }
    int* ok_flag() const { return at<int>(cv.post + dinv_bytes() + VJF_RESID_BLOCKS * 8); }
    // the two stamps areas (used with `stamps` on): a ring of 10 x 32 words behind the serial kernel's work floats, the one-launch route's
    unsigned long long* step_stamps() const { return at<unsigned long long>(cv.work + vjf_serial_work_floats(plan) * 4); }
    unsigned long long* mega_stamps() const { return at<unsigned long long>(cv.mg_stamps); }
    unsigned* mega_counters(unsigned launch) const { return at<unsigned>(cv.mg_cnt) + (size_t)(launch & 1u) * MG_C_WORDS; }   // launch k counts in block k & 1
};

namespace {
// ---- which kernel an activation uses.  Tanh has kernels of its own (separate kernels, not a run-time branch: vjf_trial_mfma_body.h
//      says why); every other activation runs the act instantiation, whose signature ends with the VjfAct.  `f` is called with the kernel,
//      and with the VjfAct behind it for an act instantiation: f(kernel, tail...) launches with `tail...` as the last arguments.
template <class KT, class KA, class F>
auto with_act_kernel(const VjfAct& act, KT tanh_kernel, KA act_kernel, F&& f) {
    if (act.kind == VJF_ACT_TANH) return f(tanh_kernel);
    return f(act_kernel, act);
}
template <class F> auto with_trial_kernel(const VjfAct& a, F&& f) { return with_act_kernel(a, vjf_trial_mfma_kernel<>, vjf_trial_mfma_kernel<VjfAct>, f); }
template <class F> auto with_mega_kernel(const VjfAct& a, F&& f) { return with_act_kernel(a, vjf_mega_kernel, vjf_mega_act_kernel, f); }
template <class F> auto with_lite_kernel(const VjfAct& a, F&& f) { return with_act_kernel(a, vjf_mega_lite_kernel, vjf_mega_lite_act_kernel, f); }

// ---- the instantiations of the Cholesky kernels that serve dz (vjf_chol_dzp).  vjf_rls_pair_kernel has none for 32: it is launched
//      for dz <= 16 only.  (The tables name the instantiations in the order the code object has always held them.)
struct CholKernels { void (*chol)(VjfPlan, VjfCholArgs); void (*pair)(VjfPlan, VjfCholArgs, VjfPostArgs); };
CholKernels chol_kernels(int dz) {
    static const decltype(CholKernels::chol) chol[5] = {vjf_chol_lds_kernel<4>, vjf_chol_lds_kernel<8>, vjf_chol_lds_kernel<12>,
                                                        vjf_chol_lds_kernel<16>, vjf_chol_lds_kernel<32>};
    static const decltype(CholKernels::pair) pair[5] = {vjf_rls_pair_kernel<4>, vjf_rls_pair_kernel<8>, vjf_rls_pair_kernel<12>,
                                                        vjf_rls_pair_kernel<16>, nullptr};
    const int dzp = vjf_chol_dzp(dz), i = dzp <= 16 ? dzp / 4 - 1 : 4;
    return CholKernels{chol[i], pair[i]};
}

// The residency check of the one-launch route, made on the kernels the context will launch (vjf_mega_kernel / vjf_mega_lite_kernel,
// or their act instantiations for another activation): workgroups per compute unit from the occupancy query; a context whose full
// grid cannot be resident takes the per-step route.
void mega_residency(vjf_ctx* c) {
    c->mega_ok = c->mega_plan;
    c->mega_wg_per_cu = 0; c->lite_wg_per_cu = 0;
    if (!c->mega_ok) return;
    auto per_cu = [](auto kernel, auto...) {
        allow_lds(kernel, kMegaLds);
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, VJF_MG_THREADS, kMegaLds) != hipSuccess) { (void)hipGetLastError(); nb = 0; }
        return nb;
    };
    c->mega_wg_per_cu = with_mega_kernel(c->act, per_cu);
    if (c->mega_wg_per_cu < 1) c->mega_ok = false;
    c->lite_wg_per_cu = with_lite_kernel(c->act, per_cu);
}
// Count the context in its device's live one-launch contexts (d->mu held) while it is on that route: from the second one on, their
// resident grids are chained (whichever kernels they run).
void count_mega(vjf_ctx* c, DevShared* d) {
    if (c->mega_counted && !c->mega_ok) {
        c->mega_counted = false;
        if (d->mega_ctxs > 0) --d->mega_ctxs;
    }
    if (c->mega_ok && !c->mega_counted) {
        c->mega_counted = true;
        if (++d->mega_ctxs == 2 && !d->chained) {
            (void)hipDeviceSynchronize();                           // (the first context's launches so far carry no event)
            if (!d->last) (void)hipEventCreateWithFlags(&d->last, hipEventDisableTiming);
            d->chained = d->last != nullptr;
        }
    }
}
// A valid vjf_activation -> *out (0), else < 0 with vjf_last_error set (include/vjf_hip.h: the supported set and its parameters)
int act_check(const vjf_activation* a, const char* who, VjfAct* out) {
    if (!a) return fail(-1, "%s: null activation", who);
    const float p0 = a->p0, p1 = a->p1;
    switch (a->kind) {
        case VJF_ACT_TANH: case VJF_ACT_RELU: case VJF_ACT_SIGMOID: break;
        case VJF_ACT_LEAKY_RELU:
            if (!(p0 >= 0.f && std::isfinite(p0))) return fail(-31, "%s: LeakyReLU negative_slope=%g (needs a finite slope >= 0)", who, p0);
            break;
        case VJF_ACT_ELU:
            if (!(p0 > 0.f && std::isfinite(p0))) return fail(-31, "%s: ELU alpha=%g (needs a finite alpha > 0)", who, p0);
            break;
        case VJF_ACT_SOFTPLUS:
            if (!(p0 > 0.f && std::isfinite(p0))) return fail(-31, "%s: Softplus beta=%g (needs a finite beta > 0)", who, p0);
            if (!(p1 >= 20.f)) return fail(-31, "%s: Softplus threshold=%g (needs >= 20)", who, p1);
            break;
        case VJF_ACT_HARDTANH:
            if (!(std::isfinite(p0) && std::isfinite(p1) && p0 < p1)) return fail(-31, "%s: Hardtanh min_val=%g max_val=%g (needs finite min_val < max_val)", who, p0, p1);
            break;
        default: return fail(-30, "%s: activation kind %d (supported: VJF_ACT_TANH .. VJF_ACT_HARDTANH)", who, (int)a->kind);
    }
    *out = VjfAct{a->kind, p0, p1};
    return 0;
}
struct SlabTables { std::vector<int> pidx, cidx, grp; };
SlabTables slab_tables(const VjfPlan& P, const VjfMegaTrialLds& Lo, const VjfMegaSlab& SL) {
    // the late slab's tables (vjf_mega_slab_layout): per float the parameter it is the gradient of and that parameter's copy
    // for the trial role -- its place in the image of the LDS region (vjf_mega_trial_lds) when the parameters fit there, else
    // in the transposed aux copies; per quad the optimizer group
    SlabTables T;
    std::vector<int>&pidx = T.pidx, &cidx = T.cidx, &grpv = T.grp;
    pidx.assign((size_t)SL.len, -1); cidx.assign((size_t)SL.len, -1); grpv.assign((size_t)SL.len / 4, 0);
    std::vector<int> img_of((size_t)P.train_len, -1), aux_of((size_t)P.train_len, -1), dec_of((size_t)P.train_len, 0);
    auto place = [&](int slot, int rows, int cols, int at, int ld) {
        const int o = P.off[slot] - P.train_off;
        for (int r = 0; r < rows; ++r)
            for (int cc = 0; cc < cols; ++cc) img_of[(size_t)o + (size_t)r * cols + cc] = at - Lo.th0 + r * ld + cc;
    };
    int prev = P.din;
    for (int l = 0; l < P.L; ++l) {
        place(VJF_SLOT_REC_W0 + 2 * l, P.h[l], prev, Lo.th_w[l], Lo.th_ldw[l]);
        place(VJF_SLOT_REC_B0 + 2 * l, 1, P.h[l], Lo.th_b[l], P.h[l]);
        prev = P.h[l];
    }
    place(VJF_SLOT_MEAN_W, P.dz, prev, Lo.th_head, Lo.th_ldh);
    place(VJF_SLOT_LV_W, P.dz, prev, Lo.th_head + P.dz * Lo.th_ldh, Lo.th_ldh);
    place(VJF_SLOT_LV_B, 1, P.dz, Lo.th_bl, P.dz);
    place(VJF_SLOT_DEC_W, P.dy, P.dz, Lo.th_dec, Lo.th_ldd);
    place(VJF_SLOT_DEC_B, 1, P.dy, Lo.th_bd, P.dy);
    for (int t = 0; t < P.n_train; ++t) {
        const int o = P.tr_off[t] - P.train_off, rows = P.tr_rows[t], cols = P.tr_cols[t];
        for (int el = 0; el < rows * cols; ++el) {
            const int r = el / cols, cc = el - r * cols;
            dec_of[(size_t)o + el] = P.tr_dec[t] ? 1 : 0;
            aux_of[(size_t)o + el] = P.tr_aux[t] >= 0 ? P.tr_aux[t] + cc * P.tr_auxld[t] + P.tr_auxcol[t] + r : -1;
        }
    }
    // block b of the slab: weight (M, Kin) [+ bias (M)] stored as rows j = 0 .. Kin - 1 [, Kin] of ldm columns m
    auto block = [&](int b, int slotW, int slotB, int M, int Kin) {
        const int ow = P.off[slotW] - P.train_off, ob = slotB >= 0 ? P.off[slotB] - P.train_off : -1;
        for (int j = 0; j < SL.rows[b]; ++j)
            for (int m2 = 0; m2 < SL.ldm[b]; ++m2) {
                const size_t at = (size_t)SL.off[b] + (size_t)j * SL.ldm[b] + m2;
                int pe = -1;
                if (m2 < M) pe = j < Kin ? ow + m2 * Kin + j : (ob >= 0 ? ob + m2 : -1);
                pidx[at] = pe;
                if (pe >= 0) {
                    cidx[at] = Lo.theta ? img_of[(size_t)pe] : aux_of[(size_t)pe];
                    grpv[at / 4] = dec_of[(size_t)pe];
                }
            }
    };
    const int hL = P.h[P.L - 1];
    block(0, VJF_SLOT_DEC_W, VJF_SLOT_DEC_B, P.dy, P.dz);
    block(1, VJF_SLOT_MEAN_W, -1, P.dz, hL);
    block(2, VJF_SLOT_LV_W, VJF_SLOT_LV_B, P.dz, hL);
    for (int l = P.L - 1; l >= 0; --l) block(3 + (P.L - 1 - l), VJF_SLOT_REC_W0 + 2 * l, VJF_SLOT_REC_B0 + 2 * l, P.h[l], l > 0 ? P.h[l - 1] : P.din);
    return T;
}
// A wait of an earlier call of this context gave up (the device said so through the host page, vjf_plan.h): this call must not
// build on its results.  One plain load of host memory in the usual case.
int refuse_if_poisoned(vjf_ctx* c, const char* who) {
    DevShared* d = dev_shared(c->cfg.device);
    float* p = c->status_word();
    if (!d || !d->mirror_h || __atomic_load_n(d->mirror_h + VJF_MIRROR_SLOT(p), __ATOMIC_RELAXED) == 0u) return 0;
    float v = 0.f;                                                 // (this context's own word: the slot may be another's)
    VJF_HIP(hipMemcpyAsync(&v, p, 4, hipMemcpyDeviceToHost, c->stream));
    VJF_HIP(hipStreamSynchronize(c->stream));
    const unsigned st = (unsigned)v;
    if (!(st & VJF_STATUS_WAIT_MASK)) return 0;
    if (c->on_mega) c->mega_ok = false;                            // (the one-launch route did not hold on this device: per-step kernels from here)
    return fail(-30, "%s: a device-side wait of an earlier call of this context timed out (status 0x%x%s); its outputs and what it left "
                     "of the state are not to be used -- read the status (vjf_get_status), restore the state, run again", who, st,
                (st & VJF_STATUS_NOT_RESIDENT) ? ": the grid was not resident as a whole, the state is untouched" : "");
}
}  // namespace
