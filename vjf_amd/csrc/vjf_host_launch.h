// vjf_host_launch.h -- host side of vjf_abi.hip: the flag block, the view of a sequence, and the helpers that enqueue the kernels of
// the per-step routes.  Included by vjf_abi.hip behind vjf_host_ctx.h.
#pragma once

namespace {
int refresh_aux(vjf_ctx* c, hipStream_t st = nullptr) {
    if (!c->mfma_trial && !c->mega_ok) return 0;
    hipLaunchKernelGGL(vjf_aux_kernel, dim3(32), dim3(256), 0, st ? st : c->stream, c->plan, (const float*)c->state, c->aux());
    VJF_HIP(hipGetLastError());
    return 0;
}

// the context's device for the duration of an entry point; the caller's current device is put back on the way out
struct DeviceGuard {
    int prev = -1, dev;
    explicit DeviceGuard(int d) : dev(d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); }
    ~DeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};

// ---- words of the flag block (vjf_ctx::flag_words, 64 of them) of the per-step routes
// [0 .. VJF_CHOL_MAXBLK + 1]: the column flags of L, written by the Cholesky workgroup, waited for by the y / W and inverse workgroups
constexpr int kCholRunWord = VJF_CHOL_MAXBLK + 2;         // Cholesky kernel: its epoch once its operands are loaded; the scalar workgroup of the prep kernel waits
constexpr int kK1DoneWord = 16;                           // trial kernel: += 1 per workgroup (whole step, backward half); the y / W workgroup waits before it writes W
constexpr int kPostStartedWord = 24;                      // post kernel: += 1 per workgroup as it starts; the scalar workgroup of the prep kernel waits
constexpr int kPostDoneWord = 32;                         // post kernel: += 1 per workgroup at its end; the next backward half waits
constexpr int kFwdDoneWord = 48;                          // forward halves launched with a count: += 1 per workgroup; the gate kernel of the statistics waits
constexpr int kReplayMaskWord = 56, kReplayRhoWord = 57;   // words of the flag block no hand-off uses
constexpr int kStatsWord = 58;                            // three-stream route: RLS statistics (summed over ranks) of how many steps are in memory
constexpr int kRankTokenWord = 60;                        // three-stream route, ranks: two floats the ranks all-reduce to enter a sequence together (60, 61)
constexpr unsigned kScAll = (1u << RS_N) - 1u, kScNone = 0u;
constexpr unsigned kScRls = 1u << RS_SDX2;                 // the one loss sum the RLS chain reads

// ---- a sequence of T steps as the caller holds it: y (T, B, dy), u (T, B, du) or null, eps (T, 2, B, dz), mu / lv (T, B, dz), the
//      prior mu0 / lv0 (B, dz) or null, loss (T, 4) or null
struct SeqView {
    int32_t B; size_t sy, su, sz;                          // floats per step of y, u, and mu / lv / one draw of eps
    const float* y; const float* u; const float* eps; const float* mu0; const float* lv0; float* mu; float* lv; float* loss;
    // the steps from t0 on: step t0's predecessor is the posterior of step t0 - 1 (the prior pointers for t0 = 0)
    SeqView from(int t0) const {
        SeqView s = *this;
        s.y = y + t0 * sy; s.u = u ? u + t0 * su : nullptr; s.eps = eps + (size_t)t0 * 2 * sz;
        if (t0) { s.mu0 = mu + (size_t)(t0 - 1) * sz; s.lv0 = lv + (size_t)(t0 - 1) * sz; }
        s.mu = mu + (size_t)t0 * sz; s.lv = lv + (size_t)t0 * sz; s.loss = loss_at(t0);
        return s;
    }
    float* loss_at(int t) const { return loss ? loss + 4 * (size_t)t : nullptr; }
    // step t's tensors (the pointer fields and B of a VjfTrialArgs; trial_args fills in the rest)
    VjfTrialArgs step(int t) const {
        const SeqView s = from(t);
        return one_step(B, s.y, s.u, s.mu0, s.lv0, s.eps, s.eps + sz, s.mu, s.lv);
    }
    static VjfTrialArgs one_step(int32_t B, const float* y, const float* u, const float* mu_s, const float* lv_s, const float* eps_s, const float* eps_t, float* mu_t, float* lv_t) {
        VjfTrialArgs a{};
        a.y = y; a.u = u; a.mu_s = mu_s; a.lv_s = lv_s; a.eps_s = eps_s; a.eps_t = eps_t; a.mu_t = mu_t; a.lv_t = lv_t; a.B = B;
        return a;
    }
};
SeqView seq_view(const vjf_ctx* c, int32_t B, const float* y, const float* u, const float* eps, const float* mu0, const float* lv0, float* mu, float* lv, float* loss) {
    return SeqView{B, (size_t)B * c->plan.dy, (size_t)B * c->plan.du, (size_t)B * c->plan.dz, y, u, eps, mu0, lv0, mu, lv, loss};
}

int check_step_args(vjf_ctx* c, const VjfTrialArgs& s) {
    if (s.B < 1 || s.B > c->cfg.max_batch) return fail(-20, "vjf_filter: B=%d outside [1, max_batch=%d]", s.B, c->cfg.max_batch);
    if (!s.y || !s.eps_s || !s.eps_t || !s.mu_t || !s.lv_t) return fail(-1, "vjf_filter: null tensor");
    if (c->plan.du > 0 && !s.u) return fail(-21, "vjf_filter: u is required when udim > 0");
    if ((s.mu_s == nullptr) != (s.lv_s == nullptr)) return fail(-22, "vjf_filter: mu_s and lv_s must both be given or both be null");
    return 0;
}

// a step's tensors + the context's buffers (`gen`: the even / odd set of E rows and partials)
VjfTrialArgs trial_args(vjf_ctx* c, const VjfTrialArgs& step, uint32_t flags, int gen = 0) {
    VjfTrialArgs a = step;
    a.state = c->state; a.flags = flags;
    a.E = c->E(gen); a.ACT = c->ACT(); a.DEL = c->DEL(); a.partial = c->partial(gen);
    return a;
}

int trial_blocks(const vjf_ctx* c, int B) { return c->mfma_trial ? (B + 15) / 16 : (B + 3) / 4; }   // (wide path: 4 trials per loss workgroup)

// one GEMM of the wide routes: a narrow output (N <= 128) splits K over the wavefronts of 32 x 32-tile workgroups; else 128 x 128 or
// 128 x 64 tiles when the shape fills the chip with them, else the 64 x 64 kernel
void launch_wide_gemm(const VjfWideGemm& g0, hipStream_t st) {
    VjfWideGemm g = g0;
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
    // 16-byte loads: aligned rows whose extent along the contiguous direction is a multiple of 4
    g.va = (g.lda % 4 == 0) && al16(g.A) && ((g.ta ? g.M : g.K) % 4 == 0);
    g.vb = (g.ldb % 4 == 0) && al16(g.Bm) && ((g.nt ? g.K : g.N) % 4 == 0);
    const int tm = (g.M + 127) / 128;
    if (g.N <= 128)
        hipLaunchKernelGGL(vjf_skinny_gemm_kernel<8>, dim3((g.M + 31) / 32, (g.N + 31) / 32), dim3(512), 0, st, g);
    else if (!g.ta && g.va && g.vb && g.M >= 256 && g.N >= 256 && tm * ((g.N + 127) / 128) >= 192) {
        const dim3 grid((g.N + 127) / 128, tm);
        if (g.nt) hipLaunchKernelGGL((vjf_wide_gemm3_kernel<128, 16, 4, false, true>), grid, dim3(512), 0, st, g);
        else hipLaunchKernelGGL((vjf_wide_gemm3_kernel<128, 16, 4, false, false>), grid, dim3(512), 0, st, g);
    } else if (!g.ta && g.va && g.vb && g.M >= 256 && g.N >= 64 && tm * ((g.N + 63) / 64) >= 32) {
        const dim3 grid((g.N + 63) / 64, tm);
        if (g.nt) hipLaunchKernelGGL((vjf_wide_gemm3_kernel<64, 32, 4, false, true>), grid, dim3(512), 0, st, g);
        else hipLaunchKernelGGL((vjf_wide_gemm3_kernel<64, 32, 4, false, false>), grid, dim3(512), 0, st, g);
    }
    else
        hipLaunchKernelGGL(vjf_wide_gemm_kernel, dim3((g.N + 63) / 64, (g.M + 63) / 64), dim3(256), 0, st, g);
}

// the element-wise activation passes of the wide route (vjf_wide_act_kernel) ...
void launch_wide_act_pass(const vjf_ctx* c, VjfWideAct w, hipStream_t st) {
    w.act = c->act;
    const size_t total = (size_t)w.M * w.N;
    const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(vjf_wide_act_kernel, dim3(grid), dim3(256), 0, st, w);
}
// ... X <- act(X) ...
void launch_wide_act(const vjf_ctx* c, float* X, int ldx, int M, int N, hipStream_t st) {
    VjfWideAct w{};
    w.X = X; w.ldx = ldx; w.M = M; w.N = N; w.mode = WACT_FWD;
    launch_wide_act_pass(c, w, st);
}
// ... and X <- X act'(H); a replay's only when *ok is non-zero
void launch_wide_act_dh(const vjf_ctx* c, float* X, int ldx, const float* H, int ldh, int M, int N, const int* ok, hipStream_t st) {
    VjfWideAct w{};
    w.X = X; w.ldx = ldx; w.H = H; w.ldh = ldh; w.M = M; w.N = N; w.mode = WACT_DH; w.ok = ok;
    launch_wide_act_pass(c, w, st);
}

// K1 of the per-step routes, whole or in halves (VjfTrialMfmaArgs::part)
enum TrialPart { kWholeStep = 0, kForwardHalf = 1, kBackwardHalf = 2 };
struct TrialOpts {
    bool count = false;                     // a forward half: count its workgroups in kFwdDoneWord; a replay: count it in kK1DoneWord
    const unsigned* rls_done = nullptr; unsigned rls_target = 0;   // a backward half waits in-kernel for *rls_done >= rls_target
    TrialOpts& counted() { count = true; return *this; }
    TrialOpts& after_rls(const unsigned* word, unsigned target) { rls_done = word; rls_target = target; return *this; }
};
int launch_trial(vjf_ctx* c, const VjfTrialArgs& a, TrialPart part, hipStream_t st, const TrialOpts& o = TrialOpts()) {
    const VjfPlan& P = c->plan;
    const int nblk = trial_blocks(c, a.B);
    if (c->mfma_trial) {
        VjfTrialMfmaArgs m{};
        m.t = a; m.aux = c->aux(); m.part = part;
        m.rls_done = o.rls_done; m.rls_target = o.rls_target;
        if (a.replay) {                                            // the backward half again; counted only where an RLS update on another
            m.part = kBackwardHalf;                                // stream must not overwrite W, w_chol, sigma under it (o.count)
            if (o.count) m.done = c->flag_words() + kK1DoneWord;
        } else {
            m.done = c->flag_words() + kK1DoneWord;
            if (part != kForwardHalf) c->k1_count += (unsigned)nblk;
            if (part == kForwardHalf && o.count) { m.fwd_done = c->flag_words() + kFwdDoneWord; c->fwd_count += (unsigned)nblk; }
            m.stamps = c->stamps ? c->step_stamps() : nullptr;
        }
        with_trial_kernel(c->act, [&](auto kernel, auto... tail) {    // (the matrix-core trial kernel of the context's activation)
            hipLaunchKernelGGL(kernel, dim3(nblk), dim3(VJF_K1M_THREADS), c->lds_k1m, st, c->plan, m, tail...);
        });
    } else {
        // working set beyond LDS: one GEMM over all trials per layer (vjf_trial_wide.h)
        VjfWideArgs w{};
        w.t = a;
        const size_t Bz = (size_t)a.B;
        w.XU = c->wide(); w.PM = w.XU + Bz * P.dxu; w.PY = w.PM + Bz * P.dz + ((Bz + 3) / 4) * 4; w.Z = w.PY + Bz * P.dy;
        const float* S = c->state;
        const bool act = c->act.kind != VJF_ACT_TANH;             // (the layers' activation: a pass behind the plain epilogues)
        const int* okw = a.replay ? (const int*)a.replay_mask : nullptr;
        auto gemm = [&](const float* A_, int lda, const float* Bm, int ldb, float* C_, int ldc, int N, int K, int nt, int epi,
                        const float* bias = nullptr, const float* src = nullptr, int lds = 0) {
            VjfWideGemm g{};
            g.A = A_; g.lda = lda; g.Bm = Bm; g.ldb = ldb; g.C = C_; g.ldc = ldc; g.M = a.B; g.N = N; g.K = K; g.nt = nt; g.epi = epi;
            g.bias = bias; g.src = src; g.lds = lds; g.src_scale = 1.f; g.eps_t = a.eps_t; g.lv_t = a.lv_t;
            g.ok = a.replay ? (const int*)a.replay_mask : nullptr;     // (a replay's launches do nothing when the word is 0)
            launch_wide_gemm(g, st);
        };
        const int gx = 1024;
        // part 1: everything up to the decoder (no use of W, w_chol, sigma); part 2: predictive moments, losses, backward; 0: both
        if (!a.replay && part != kBackwardHalf) {                              // (a replay: what the backward half reads stays in place)
        hipLaunchKernelGGL(vjf_wide_in_kernel, dim3(a.B < 2048 ? a.B : 2048), dim3(256), 0, st, P, w);
        hipLaunchKernelGGL(vjf_wide_rbf_kernel, dim3((P.n + 255) / 256, (a.B + 15) / 16), dim3(256), 0, st, P, w);
        int kin = P.din;
        for (int l = 0; l < P.L; ++l) {                            // h_l = tanh(h_{l-1} W_l^T + b_l)   (recognition.py:31-36)
            gemm(a.ACT + P.colA_act[l], P.ldA, S + P.off[VJF_SLOT_REC_W0 + 2 * l], kin, a.ACT + P.colA_act[l + 1], P.ldA, P.h[l], kin, 1,
                 act ? WEPI_BIAS : WEPI_TANH_BIAS, S + P.off[VJF_SLOT_REC_B0 + 2 * l]);
            if (act) launch_wide_act(c, a.ACT + P.colA_act[l + 1], P.ldA, a.B, P.h[l], st);   // (other activations)
            kin = P.h[l];
        }
        if (P.off[VJF_SLOT_LV_W] == P.off[VJF_SLOT_MEAN_W] + P.dz * kin) {   // the heads' weights lie one behind the other: ONE product, N = 2 dz
            VjfWideGemm g{};
            g.A = a.ACT + P.colA_act[P.L]; g.lda = P.ldA; g.Bm = S + P.off[VJF_SLOT_MEAN_W]; g.ldb = kin; g.C = a.mu_t; g.C2 = a.lv_t; g.ldc = P.dz;
            g.M = a.B; g.N = 2 * P.dz; g.K = kin; g.nt = 1; g.epi = WEPI_HEADS; g.bias = S + P.off[VJF_SLOT_LV_B];
            launch_wide_gemm(g, st);
        } else {
        gemm(a.ACT + P.colA_act[P.L], P.ldA, S + P.off[VJF_SLOT_MEAN_W], kin, a.mu_t, P.dz, P.dz, kin, 1, WEPI_NONE);
        gemm(a.ACT + P.colA_act[P.L], P.ldA, S + P.off[VJF_SLOT_LV_W], kin, a.lv_t, P.dz, P.dz, kin, 1, WEPI_BIAS, S + P.off[VJF_SLOT_LV_B]);
        }
        hipLaunchKernelGGL(vjf_wide_mid_kernel, dim3(gx), dim3(256), 0, st, P, w);
        gemm(a.ACT + P.colA_xt, P.ldA, S + P.off[VJF_SLOT_DEC_W], P.dz, w.PY, P.dy, P.dy, P.dz, 1, WEPI_BIAS, S + P.off[VJF_SLOT_DEC_B]);
        }
        if (part == kForwardHalf) { VJF_HIP(hipGetLastError()); return 0; }
        if (!a.replay) {
        gemm(a.E, P.ldE, S + P.off[VJF_SLOT_W_MEAN], P.dz, w.PM, P.dz, P.dz, P.n, 0, WEPI_ADD_SRC, nullptr, w.XU, P.dxu);
        gemm(a.E, P.ldE, S + P.off[VJF_SLOT_W_CHOL], P.n, w.Z, P.n, P.n, P.n, 0, WEPI_NONE);
        }
        hipLaunchKernelGGL(vjf_wide_loss_kernel, dim3((a.B + 3) / 4), dim3(256), 0, st, P, w);
        // backward: dxt = dpy C into dmu / dlv; dh_L = dmu Wm + dlv Wl; da_l = (da_{l+1} W_{l+1}) (1 - h_l^2)
        gemm(a.DEL + P.colD_dpy, P.ldD, S + P.off[VJF_SLOT_DEC_W], P.dz, a.DEL + P.colD_dmu, P.ldD, P.dz, P.dy, 0, WEPI_SEED);
        const int hL = P.h[P.L - 1];
        if (P.off[VJF_SLOT_LV_W] == P.off[VJF_SLOT_MEAN_W] + P.dz * hL && P.colD_dlv == P.colD_dmu + P.dz)
            // the two heads' weights lie one behind the other in the state, their seeds side by side in DEL: ONE product with K = 2 dz
            gemm(a.DEL + P.colD_dmu, P.ldD, S + P.off[VJF_SLOT_MEAN_W], hL, a.DEL + P.colD_da[P.L - 1], P.ldD, hL, 2 * P.dz, 0,
                 act ? WEPI_NONE : WEPI_DTANH, nullptr, a.ACT + P.colA_act[P.L], P.ldA);
        else {
        gemm(a.DEL + P.colD_dmu, P.ldD, S + P.off[VJF_SLOT_MEAN_W], hL, a.DEL + P.colD_da[P.L - 1], P.ldD, hL, P.dz, 0, WEPI_NONE);
        if (act)                                                   // (dh += dlv Wl, in place: C is its own source)
            gemm(a.DEL + P.colD_dlv, P.ldD, S + P.off[VJF_SLOT_LV_W], hL, a.DEL + P.colD_da[P.L - 1], P.ldD, hL, P.dz, 0, WEPI_ADD_SRC, nullptr,
                 a.DEL + P.colD_da[P.L - 1], P.ldD);
        else
        gemm(a.DEL + P.colD_dlv, P.ldD, S + P.off[VJF_SLOT_LV_W], hL, a.DEL + P.colD_da[P.L - 1], P.ldD, hL, P.dz, 0, WEPI_ADDC_DTANH, nullptr,
             a.ACT + P.colA_act[P.L], P.ldA);
        }
        if (act) launch_wide_act_dh(c, a.DEL + P.colD_da[P.L - 1], P.ldD, a.ACT + P.colA_act[P.L], P.ldA, a.B, hL, okw, st);
        for (int l = P.L - 1; l >= 1; --l) {
            gemm(a.DEL + P.colD_da[l], P.ldD, S + P.off[VJF_SLOT_REC_W0 + 2 * l], P.h[l - 1], a.DEL + P.colD_da[l - 1], P.ldD, P.h[l - 1], P.h[l], 0,
                 act ? WEPI_NONE : WEPI_DTANH, nullptr, a.ACT + P.colA_act[l], P.ldA);
            if (act) launch_wide_act_dh(c, a.DEL + P.colD_da[l - 1], P.ldD, a.ACT + P.colA_act[l], P.ldA, a.B, P.h[l - 1], okw, st);
        }
    }
    VJF_HIP(hipGetLastError());
    return 0;
}

// Gram tiles of a range of the context's jobs and their slab reduction into `red` (with the loss sums of `sc_mask`)
enum GramJobs { kGramAll, kGramStats, kGramGrads };       // every job | the E^T E tiles (RLS statistics) | the gradient tiles
struct GramOpts {
    int gen = 0;                            // the even / odd set of E rows and partials
    const unsigned* run_if = nullptr;       // both launches do nothing when the word is 0 (a replay)
    unsigned* done_count = nullptr;         // see VjfReduceArgs (njobs + (sc_mask ? 1 : 0) arrivals)
    GramOpts& rows(int g) { gen = g; return *this; }
    GramOpts& only_if(const unsigned* word) { run_if = word; return *this; }
    GramOpts& count_into(unsigned* word) { done_count = word; return *this; }
};
int launch_gram(vjf_ctx* c, int B, GramJobs which, unsigned sc_mask, float* red, hipStream_t st, const GramOpts& o = GramOpts()) {
    const VjfPlan& P = c->plan;
    const int job0 = which == kGramGrads ? c->n_ejobs : 0, njobs = which == kGramAll ? c->njobs : which == kGramStats ? c->n_ejobs : c->njobs - c->n_ejobs;
    const int nsplit = split_for(B);
    VjfGramArgs g{};
    g.jobs = c->jobs(); g.E = c->E(o.gen); g.ACT = c->ACT(); g.DEL = c->DEL(); g.slabs = c->slabs();
    g.B = B; g.nsplit = nsplit; g.job0 = job0;
    g.rows_per_split = ((B + nsplit - 1) / nsplit + 7) / 8 * 8;
    g.run_if = o.run_if;
    hipLaunchKernelGGL(vjf_gram_kernel, dim3(njobs * nsplit), dim3(VJF_GRAM_THREADS), 0, st, P, g);
    VJF_HIP(hipGetLastError());
    VjfReduceArgs r{};
    r.jobs = g.jobs; r.slabs = g.slabs; r.partial = c->partial(o.gen); r.red = red;
    r.njobs = njobs; r.nsplit = nsplit; r.nblocks_k1 = trial_blocks(c, B); r.job0 = job0; r.sc_mask = sc_mask; r.run_if = o.run_if;
    r.done_count = o.done_count;
    hipLaunchKernelGGL(vjf_gram_reduce_kernel, dim3(njobs + (sc_mask ? 1 : 0)), dim3(VJF_REDUCE_THREADS), 0, st, P, r);
    VJF_HIP(hipGetLastError());
    return 0;
}

// The prep grid: the RLS operand rows (P += G/v, g), and clip + SGD with the scalar workgroup
enum PrepWhich { kPrepAll = 0, kPrepOperands = 1, kPrepSgd = 2 };
enum ReplayPass { kNoReplay = 0, kReplayFollows = 1, kReplayedPass = 2 };   // the first pass with a replay behind it | the pass behind the replay
struct PrepOpts {
    float* loss4 = nullptr;
    ReplayPass replay = kNoReplay;
    // the scalar workgroup ends only once the step's Cholesky kernel runs (*run_word >= run_epoch) and its post workgroups are resident
    const unsigned* run_word = nullptr; unsigned run_epoch = 0; const unsigned* start_count = nullptr; unsigned start_target = 0;
    const unsigned* wait_count = nullptr; unsigned wait_target = 0;   // the operand kernel waits in-kernel for *wait_count
    PrepOpts& loss(float* p) { loss4 = p; return *this; }
    PrepOpts& pass(ReplayPass r) { replay = r; return *this; }
    PrepOpts& end_when_rls_resident(const unsigned* run, unsigned epoch, const unsigned* started, unsigned target) { run_word = run; run_epoch = epoch; start_count = started; start_target = target; return *this; }
    PrepOpts& after(const unsigned* word, unsigned target) { wait_count = word; wait_target = target; return *this; }
};
int launch_prep(vjf_ctx* c, int32_t B_total, uint32_t flags, const float* red, PrepWhich which, hipStream_t st, const PrepOpts& o = PrepOpts()) {
    const VjfPlan& P = c->plan;
    VjfPrepArgs p{};
    p.state = c->state; p.red = red; p.gbuf = c->work(); p.aux = c->aux();
    p.loss4 = o.loss4; p.B_total = B_total; p.flags = flags;
    p.n_rowblk = (P.n + VJF_PREP_ROWS - 1) / VJF_PREP_ROWS;
    p.n_sgdblk = (P.train_len + 1023) / 1024;
    p.run_word = o.run_word; p.run_epoch = o.run_epoch; p.start_count = o.start_count; p.start_target = o.start_target;
    p.wait_count = o.wait_count; p.wait_target = o.wait_target;
    if (o.replay != kNoReplay) {
        p.replay_mask = c->flag_words() + kReplayMaskWord; p.replay_rho = (float*)c->flag_words() + kReplayRhoWord;
        p.replay_pass = o.replay == kReplayedPass ? 1 : 0;
    }
    if (which != kPrepSgd && P.dz > 16) {                      // (the matrix-core operand kernel holds one 16-column tile of W)
        p.bid0 = 0;
        const int grid = which == kPrepOperands ? p.n_rowblk : p.n_rowblk + p.n_sgdblk + 1;
        hipLaunchKernelGGL(vjf_prep_kernel, dim3(grid), dim3(256), 0, st, P, p);
        VJF_HIP(hipGetLastError());
        return 0;
    }
    if (which != kPrepSgd) {                                   // RLS operands: g and P += G/v, 16 rows per workgroup
        const size_t lds = vjf_prepg_lds_bytes(P);
        hipLaunchKernelGGL(vjf_prepg_kernel, dim3((P.n + 15) / 16), dim3(256), lds, st, P, p);
        VJF_HIP(hipGetLastError());
        if (which == kPrepOperands) return 0;
    }
    p.bid0 = p.n_rowblk;                                       // clip + SGD and the scalars
    hipLaunchKernelGGL(vjf_prep_kernel, dim3(p.n_sgdblk + 1), dim3(256), 0, st, P, p);
    VJF_HIP(hipGetLastError());
    return 0;
}

// state-noise update (model.py:373-377) from the residual itself, on a rank that holds every trial: R = Phi W with the GEMM kernel
// (into the DEL rows, free once the gradient sums -- and a replay's -- are formed, or a buffer of the caller's), then sum (dx - R)^2
void launch_resid_direct(const vjf_ctx* c, const VjfTrialArgs& ta, float* R, const VjfResidArgs& ra, hipStream_t st) {
    const VjfPlan& P = c->plan;
    VjfWideGemm g{};
    g.A = ta.E; g.lda = P.ldE; g.Bm = c->state + P.off[VJF_SLOT_W_MEAN]; g.ldb = P.dz; g.C = R; g.ldc = P.dz;
    g.M = ta.B; g.N = P.dz; g.K = P.n; g.epi = WEPI_NONE;
    launch_wide_gemm(g, st);
    hipLaunchKernelGGL(vjf_resid_direct_kernel, dim3(VJF_RESID_BLOCKS), dim3(256), 0, st, P, ra, (const float*)ta.E, (const float*)R, ta.B);
}

// Cholesky + RLS tail + state-noise update of one step.  kRlsOneGrid (three-stream route): the whole update -- Cholesky workgroup,
// y / W workgroup, inverse workgroups -- goes out as ONE launch on `st`, whose workgroups hand the columns of L to each other through
// flags (all of them belong to one grid; the operand kernel precedes it in `st`, so g is in place), and the route has cleared the
// unused triangles of w_chol / w_pchol itself (no_triclean).  `ta`: the trial-parallel half's arguments when this rank holds ALL trials.
enum RlsForm { kRlsSeparate, kRlsOneGrid };
int launch_rls(vjf_ctx* c, int32_t B_total, uint32_t flags, const float* red, hipStream_t st, RlsForm form, const VjfTrialArgs* ta = nullptr) {
    const VjfPlan& P = c->plan;
    const bool one_launch = form == kRlsOneGrid, no_triclean = one_launch;
    if (!(flags & VJF_FLAG_UPDATE)) return 0;
    VjfCholArgs a{};
    a.state = c->state; a.red = red; a.gbuf = c->work(); a.B_total = B_total; a.flags = flags;
    a.stamps = c->stamps ? c->step_stamps() : nullptr;
    const int nbl = (P.n + 31) / 32;
    unsigned* colflags = c->flag_words();
    a.post = c->post_kernels ? 1 : 0; a.dinv_out = c->dinv(); a.ok_out = c->ok_flag(); a.lscr = c->lscr();
    a.flags_out = colflags; a.epoch = ++c->epoch; a.no_triclean = no_triclean ? 1 : 0;
    a.pscr = c->pscr();
    const bool rls = !(flags & VJF_FLAG_WARM_UP);
    const bool pair = one_launch && c->post_kernels && rls && P.dz <= 16;
    if (!pair) {
        hipLaunchKernelGGL(chol_kernels(P.dz).chol, dim3(1), dim3(VJF_CHOL_THREADS), c->lds_chol, st, P, a);
        VJF_HIP(hipGetLastError());
    }
    if (!c->post_kernels) return 0;
    VjfResidArgs ra{};
    ra.state = c->state; ra.red = red; ra.partial = c->resid_partial(); ra.B_total = B_total; ra.flags = flags;
    if (rls) {
        // inverse column halves + the y / W workgroup, which also carries the state-noise update
        VjfPostArgs pa{};
        pa.state = c->state; pa.dinv = a.dinv_out; pa.gbuf = a.gbuf; pa.lscr = a.lscr;
        pa.flags = colflags; pa.epoch = a.epoch; pa.status = c->status_word();
        pa.k1_done = c->mfma_trial ? colflags + kK1DoneWord : nullptr; pa.k1_target = c->k1_count;
        pa.done = colflags + kPostDoneWord; pa.started = colflags + kPostStartedWord; c->post_count += (unsigned)(2 * nbl + 1);
        c->start_count += (unsigned)(2 * nbl + 1);
        pa.red = red; pa.B_total = B_total; pa.fold_sigma = 1; pa.acquire = c->handoff_acquire ? 1 : 0; pa.stamps = a.stamps;
        // Fewer trials than features on a rank that holds them all (the rows of [Phi | dx] are in the workspace): the new weights
        // reproduce dx almost exactly, and the quadratic form of the statistics, sum|dx|^2 - 2 tr(W^T Phi^T dx) + tr(W^T G W),
        // loses the residual under the fp32 rounding of its terms (sigma 1e-5 off where the reference's arithmetic is at 1e-6).
        // The residual is then formed as the reference forms it, dx - Phi W (vjf/model.py:373-374), behind the update: three
        // short launches on a route that is launch-bound anyway.
        const bool direct = ta && !pair && B_total < P.n && ta->B == B_total;
        if (direct) pa.fold_sigma = 0;
        if (pair) {
            pa.role = 2;
            hipLaunchKernelGGL(chol_kernels(P.dz).pair, dim3(2 + 2 * nbl), dim3(VJF_CHOL_THREADS), c->lds_chol, st, P, a, pa);
        } else {
            hipLaunchKernelGGL(vjf_rls_post_kernel, dim3(2 * nbl + 1), dim3(VJF_POST_THREADS), c->lds_post, st, P, pa);
        }
        VJF_HIP(hipGetLastError());
        if (direct) {
            launch_resid_direct(c, *ta, ta->DEL, ra, st);          // (DEL is free: the gradient sums -- and a replay's -- are formed)
            hipLaunchKernelGGL(vjf_sigma_kernel, dim3(1), dim3(64), 0, st, P, ra, (const int*)nullptr, 1);
            VJF_HIP(hipGetLastError());
        }
    } else {
        hipLaunchKernelGGL(vjf_resid_kernel, dim3(VJF_RESID_BLOCKS), dim3(256), 0, st, P, ra);
        hipLaunchKernelGGL(vjf_sigma_kernel, dim3(1), dim3(64), 0, st, P, ra, (const int*)nullptr, 0);
        VJF_HIP(hipGetLastError());
    }
    return 0;
}

// sum over ranks, in place (no communicator: nothing to do).  Test hook: fake_world identical ranks, the sum times their number
int all_reduce_sum(const vjf_ctx* c, float* p, size_t nfl, void* comm, hipStream_t st) {
    if (!comm) return 0;
    VJF_NCCL(nccl().all_reduce(p, p, nfl, kNcclFloat, kNcclSum, comm, st));
    if (c->fake_world > 1) hipLaunchKernelGGL(vjf_scale_kernel, dim3(64), dim3(256), 0, st, p, (float)c->fake_world, (int)nfl);
    return 0;
}

// K1 + Gram + slab reduce.  `aux_fresh`: the transposed weight copies are known to match the state blob.
int launch_local(vjf_ctx* c, const VjfTrialArgs& step, uint32_t flags, bool aux_fresh) {
    int rc = check_step_args(c, step);
    if (rc) return rc;
    c->on_mega = false;
    if (c->mfma_trial && !aux_fresh) { rc = refresh_aux(c); if (rc) return rc; }
    rc = launch_trial(c, trial_args(c, step, flags), kWholeStep, c->stream);
    if (rc) return rc;
    return launch_gram(c, step.B, kGramAll, kScAll, c->red(), c->stream);
}

// the backward half again with the seeds of the dropped loss components at zero (the verdict of the first pass is in the flag block)
VjfTrialArgs replay_args(const vjf_ctx* c, VjfTrialArgs a) {
    a.replay = 1;
    a.replay_mask = c->flag_words() + kReplayMaskWord;
    a.replay_rho = (const float*)c->flag_words() + kReplayRhoWord;
    return a;
}

int ensure_stream2(vjf_ctx* c) {
    if (c->stream2) return 0;                  // (reached from vjf_filter_seq only: its DeviceGuard holds the context's device)
    VJF_HIP(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    VJF_HIP(hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking));
    VJF_HIP(hipEventCreate(&c->ev_c));
    VJF_HIP(hipEventCreate(&c->ev_s));          // (default flags: the events are attached to kernel launches)
    for (int i = 0; i < 2; ++i)
        for (hipEvent_t* ev : {c->ev_f, c->ev_r, c->ev_b, c->ev_g}) VJF_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    return 0;
}

// The RLS update for feature counts beyond one compute unit's LDS (vjf_rlsb_kernels.h) and the state-noise update, on stream `st`
struct RlsbOpts {
    const VjfTrialArgs* ta = nullptr;       // the trial-parallel half's arguments when this rank holds every trial, else null
    hipEvent_t before_write = nullptr;      // the stream waits for it before the update's first store to the state: the readers on another stream
    float* resid = nullptr;                 // B x dz floats for Phi W (default: the trial chain's DEL rows)
    bool resident = false;                  // the column sequence as one resident launch (vjf_rlsc_loop_kernel): beside other streams' kernels
    RlsbOpts& all_trials(const VjfTrialArgs* a) { ta = a; return *this; }
    RlsbOpts& beside_trial_chain(hipEvent_t readers_done, float* phi_w) { before_write = readers_done; resid = phi_w; resident = true; return *this; }
};
int launch_rlsb(vjf_ctx* c, int32_t B_total, uint32_t flags, const float* red, hipStream_t st, const RlsbOpts& o = RlsbOpts()) {
    const VjfPlan& P = c->plan;
    const VjfTrialArgs* ta = o.ta;
    const int nbl = (P.n + 31) / 32;
    float* work = c->work();
    VjfRlsbArgs a{};
    a.state = c->state; a.red = red; a.Lw = c->lscr();
    a.X = work; a.gbuf = work + (size_t)P.n * P.n; a.ybuf = a.gbuf + (size_t)P.n * P.dz;
    a.Dinv = c->dinv(); a.Ld = c->tbig(); a.Pacc = a.Ld + (size_t)nbl * 1024; a.ok = c->ok_flag();
    { const char* ab = getenv("VJF_DEBUG_RLSC_ABSENT"); a.absent_wg = ab ? atoi(ab) : 0; }
    const bool rls = !(flags & VJF_FLAG_WARM_UP);
    if (rls) {
        const int gx = 512;
        auto gemm = [&](const float* A_, int lda, int ta, const float* Bm, int ldb, float* C_, int ldc, int M, int N, int K, const int* ok) {
            VjfWideGemm g{};
            g.A = A_; g.lda = lda; g.ta = ta; g.Bm = Bm; g.ldb = ldb; g.C = C_; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.nt = 0;
            g.epi = WEPI_NONE; g.ok = ok;
            launch_wide_gemm(g, st);
        };
        const float* Sx = c->state;
        gemm(Sx + P.off[VJF_SLOT_W_PREC], P.n, 0, Sx + P.off[VJF_SLOT_W_MEAN], P.dz, a.gbuf, P.dz, P.n, P.dz, P.n, nullptr);   // P W
        hipLaunchKernelGGL(vjf_rlsb_prep_kernel, dim3(gx), dim3(256), 0, st, P, a);
        // block column k of L and block row k - 1 of X = L^-1 per launch (the block-upper part of X stays zero: the solves
        // below read all of it)
        VJF_HIP(hipMemsetAsync(a.X, 0, (size_t)P.n * P.n * 4, st));
        // (alone on the chip the launches are the faster form: 937 against 1017 us a step at config E, a step barrier costs more than
        //  a dispatch; beside the trial chain both give 770-780 us, the resident form with a third of the host's enqueue time)
        static const bool per_column = getenv("VJF_RLS_COLUMN_LAUNCHES") != nullptr;   // (A/B)
        if (o.resident && !per_column && 2 * nbl - 1 <= c->ncu)
            hipLaunchKernelGGL(vjf_rlsc_loop_kernel, dim3(2 * nbl - 1), dim3(VJF_RLSC_THREADS), 0, st, P, a, (unsigned*)(a.ok + 4));
        else
        for (int k = 0; k <= nbl; ++k) {
            a.k = k;
            const int ncol = nbl - k, grid = ncol + (ncol > 1 ? ncol - 1 : 0) + (k > 1 ? k - 1 : 0);
            hipLaunchKernelGGL(vjf_rlsc_col_kernel, dim3(grid), dim3(VJF_RLSC_THREADS), 0, st, P, a);
        }
        gemm(a.X, P.n, 0, a.gbuf, P.dz, a.ybuf, P.dz, P.n, P.dz, P.n, a.ok);                                      // y = X g
        if (o.before_write) VJF_HIP(hipStreamWaitEvent(st, o.before_write, 0));
        gemm(a.X, P.n, 1, a.ybuf, P.dz, c->state + P.off[VJF_SLOT_W_MEAN], P.dz, P.n, P.dz, P.n, a.ok);          // W = X^T y
        hipLaunchKernelGGL(vjf_rlsb_final_kernel, dim3(gx), dim3(256), 0, st, P, a);
        VJF_HIP(hipGetLastError());
    }
    else if (o.before_write) VJF_HIP(hipStreamWaitEvent(st, o.before_write, 0));
    VjfResidArgs ra{};
    ra.state = c->state; ra.red = red; ra.partial = c->resid_partial(); ra.B_total = B_total; ra.flags = flags;
    if (ta) {
        launch_resid_direct(c, *ta, o.resid ? o.resid : ta->DEL, ra, st);
    } else {
        // ranks holding shards: the same sum as the quadratic form of the reduced statistics, T = G W with the GEMM kernel (y's
        // buffer is free again), contraction in fp64
        VjfWideGemm g{};
        g.A = red + P.red_G; g.lda = P.n; g.Bm = c->state + P.off[VJF_SLOT_W_MEAN]; g.ldb = P.dz; g.C = a.ybuf; g.ldc = P.dz;
        g.M = P.n; g.N = P.dz; g.K = P.n; g.epi = WEPI_NONE;
        launch_wide_gemm(g, st);
        hipLaunchKernelGGL(vjf_resid_dot_kernel, dim3(VJF_RESID_BLOCKS), dim3(256), 0, st, P, ra, (const float*)a.ybuf);
    }
    hipLaunchKernelGGL(vjf_sigma_kernel, dim3(1), dim3(64), 0, st, P, ra, (const int*)nullptr, ta ? 1 : 0);
    VJF_HIP(hipGetLastError());
    return 0;
}

// After the SGD pass of a one-rank step: the backward half with the seeds of the dropped loss components at zero, the gradient
// sums, and the SGD pass from them -- every launch returns at once unless the first pass found a non-finite component
// (vjf/model.py:138-149; the one-launch route does the same inside its grid).
int launch_replay(vjf_ctx* c, const VjfTrialArgs& a0, int32_t B_total, uint32_t flags, hipStream_t st, int gen = 0) {
    const VjfTrialArgs a = replay_args(c, a0);
    int rc = launch_trial(c, a, kBackwardHalf, st);
    if (rc) return rc;
    if ((rc = launch_gram(c, a.B, kGramGrads, kScNone, c->red(), st, GramOpts().rows(gen).only_if(a.replay_mask)))) return rc;
    return launch_prep(c, B_total, flags, c->red(), kPrepSgd, st, PrepOpts().pass(kReplayedPass));
}
}  // namespace
