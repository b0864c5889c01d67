// vjf_mega_trial.h -- the trial role of the one-launch route (vjf_mega_kernel.h).
#pragma once
#include "vjf_mega_common.h"

// ------------------------------------------------------------------------------------------------ trial role
// RLS = true: the training step (sgd + update, no warm-up) beside the RLS, Gram and operand roles -- every mode switch below is a
// compile-time constant and the code is what it was before the other flag sets existed.  RLS = false (vjf_mega_lite_kernel: trial
// and SGD roles only): warm-up, update=False, sgd=False, read from the launch's flags.
//
// ACT = true (vjf_mega_act_kernel, vjf_mega_lite_act_kernel): the recognition layers' activation is `act` (vjf_act.h), read from
// the launch's arguments, in place of tanh; ACT = false is the Tanh code and ignores `act`.
template <bool RLS, bool ACT = false>
__device__ __forceinline__ void vjf_mega_trial(const VjfPlan& P, const VjfMegaArgs& A, float* smem, const int wg, const VjfAct act = VjfAct{}) {
    constexpr int LD = VJF_MG_LD, NW = VJF_MG_WAVES, NT = VJF_MG_THREADS, TR = VJF_MG_TR;
    // the variance and mean products with their k range split into full and partial steps (mg_var2): the Tanh training kernel only -- the
    // kernels of the other activations have no registers for it, and vjf_mega_lite_kernel (whose moments role forms these products at
    // the sizes that matter) ran 0.3 - 1.6 us a step slower in warm-up with it (profiles/var_interior_isa.txt, var_interior_ab.txt)
    constexpr bool VSPLIT = RLS && !ACT;
    // the gradient tiles walked from the plan's tile table (mg_grad_walk) instead of one loop per tensor: the Tanh training kernel only
    // (profiles/grad_tiles_isa.txt); the other kernels keep grad_tensor / mg_grad_tile
    constexpr bool GTAB = RLS && !ACT;
    const int tid0 = threadIdx.x;
    const int dz = P.dz, dy = P.dy, du = P.du, n = P.n, din = P.din, dxu = P.dxu;
    const float* S = A.state;
    float* SCW = A.state + P.off[VJF_SLOT_SCALARS];
    // what the steps of this launch do (vjf/model.py:179-221: the flags of VJF.filter).  mode_rls: the RLS roles, the Gram and the
    // operand role exist; without them (warm-up, update=False) W, w_chol are constants of the launch and sigma -- if it moves at all
    // (warm-up) -- comes from the SGD role with the parameters
    const bool do_sgd = RLS || (A.flags & VJF_FLAG_SGD) != 0u, do_upd = RLS || (A.flags & VJF_FLAG_UPDATE) != 0u;
    const bool warm = !RLS && (A.flags & VJF_FLAG_WARM_UP) != 0u;
    constexpr bool mode_rls = RLS;                     // (the host sends a launch with do_upd && !warm to the full kernel only)
    const bool gated = RLS || do_sgd || do_upd;        // something another role produces changes between steps
    const bool want_resid = !RLS && do_upd && warm;
    // a moments role (vjf_mega_moments) forms the features and the predictive moments of this role's tiles a step ahead: this
    // role then neither forms features nor walks L^-1
    const bool use_mom = !RLS && A.n_mom > 0;
    const unsigned m_dy = mg_magic(dy), m_dz = mg_magic(dz), m_du = mg_magic(du > 0 ? du : 1);
    const VjfMegaTrialLds Lo = vjf_mega_trial_lds<false>(P, A.lds_floats);
    const bool tl = Lo.theta != 0;                    // the optimised parameters are staged in LDS once per step
    float* s_cen = smem + Lo.cen; float* s_iw = smem + Lo.iw;
    float* s_in = smem + Lo.in; float* s_xu = smem + Lo.xu; float* s_phi = smem + Lo.phi; float* s_act = smem + Lo.act;
    float* s_dd = smem + Lo.dd;
    float* s_mu = smem + Lo.mu; float* s_lv = smem + Lo.lv; float* s_xt = smem + Lo.xt; float* s_e2 = smem + Lo.e2; float* s_pm = smem + Lo.pm;
    float* s_dmu = smem + Lo.dmu; float* s_dlv = smem + Lo.dlv; float* s_dx = smem + Lo.dx;
    float* s_py = smem + Lo.py; float* s_dpy = smem + Lo.dpy;
    float* s_one = smem + Lo.one; float* s_zero = smem + Lo.zero;
    float* s_sc = smem + Lo.sc; float* s_red = smem + Lo.red; float* s_plv = smem + Lo.plv; float* s_wg = smem + Lo.wg;
    const bool compact = dy >= P.hmax;
    float* s_d0 = compact ? s_py : s_dd;               // compact: written only after the losses have consumed s_py
    float* s_d1 = compact ? s_dd : s_dd + P.hmax * LD; // used only when n_hidden > 1
    float* s_part = smem + Lo.part;                    // partial tiles of the K-split products (heads, pt.mean)
    constexpr int part_rows = VJF_MG_WAVES * 16;
    int mean_nsl = 1;
    __shared__ unsigned s_try[2];
    unsigned* cnt = A.cnt;
    const unsigned npost = (unsigned)(A.n_rls - 1);
    float* late = A.slab_late + (size_t)wg * A.late_len;
    const int ldn = (n + 3) & ~3;                      // early slab: [16 columns][ldn] Phi^T dx (transposed), then the scalars
    const size_t sy = (size_t)A.B * dy, su = (size_t)A.B * du, sz = (size_t)A.B * dz;
    int ntl = 0;
    for (int tile = wg; tile < A.ntiles; tile += A.n_trial) ++ntl;
    bool tri_launch = false;                           // a launch without an RLS update: its constant w_chol was SEEN to be upper triangular (below)

    const int npad = (n + 3) & ~3;
    mg_stage_centres(P, S, s_cen, s_iw, tid0);
    if (tid0 < LD) s_zero[tid0] = 0.f;
    __syncthreads();

    // A step whose loss has a non-finite component (model.py:138-145) is REPLAYED: the SGD role sees the sums only when every
    // workgroup's backward pass is done, publishes which components to drop and leaves the parameters alone; the trial role finds
    // that word when it fetches the parameters for the next step, runs the flagged step's forward and backward pass again --
    // same parameters, same inputs, the predictive mean / variance it saved, the dropped components' seeds exactly zero --, hands
    // over a second late slab, waits for the SGD role's (unconditional) step on it and only then starts over with the next step.
    // Nothing of this costs the usual step anything but one more word read beside rho.  Step index T is the gate alone.
    float sig_prev = 0.f, rho_prev = 0.f;
    unsigned nredo = 0;
    unsigned ring_seen = 0u;                           // a launch without parameter updates: the count of summed steps as last looked at
    for (int t = 0; t <= A.T; ++t) {
      bool replay = false, replayed = false;
      unsigned rbits = 0;
      for (;;) {
        const int ts = replay ? t - 1 : t;             // the step whose inputs this pass stages
        bool want_replay = false;
        // (the thread index is made opaque at every phase boundary: what the compiler derives from it -- dozens of per-thread LDS and
        //  memory offsets, one set per loop of the step -- is then formed in the phase that uses it instead of at the top of the step,
        //  where it was kept, and spilled to scratch memory, across the whole step)
        int tid = tid0, lane, wave;
        MG_PHASE();
        const int tc = min(ts, A.T - 1);               // (the gate pass of step T stages nothing)
        const float* y_t = A.y + (size_t)tc * sy;
        const float* u_t = A.u ? A.u + (size_t)tc * su : nullptr;
        const float* mu_s = tc ? A.mu + (size_t)(tc - 1) * sz : A.mu0;
        const float* lv_s = tc ? A.lv + (size_t)(tc - 1) * sz : A.lv0;
        const float* eps_s = A.eps + (size_t)tc * 2 * sz;
        const float* eps_t = eps_s + sz;
        float* mu_t = A.mu + (size_t)tc * sz;
        float* lv_t = A.lv + (size_t)tc * sz;
        const bool prior = (mu_s == nullptr);
        const bool m_r = !(rbits & 1u), m_d = !(rbits & 2u), m_h = !(rbits & 4u);   // components kept (all of them unless replaying)
        // early slabs alternate between two sets: the operand role may read step t's long after this workgroup has started
        // step t + 1 (it also waits for the Gram of step t); step t + 2 starts behind the RLS update of step t, which consumed them
        float* early = A.slab_early + ((size_t)(tc & 1) * A.n_trial + wg) * A.early_len;
        VJF_MG_STAMP(0);
        if (tid < 16) s_wg[tid] = 0.f;
        float sig = sig_prev, rho = rho_prev;          // (a replayed pass: the values its step ran with)
        bool tri = false, rls_in = replay;
        // the parameters of step t - 1 (the SGD role's write-through stores) and its verdict on that step's loss
        // One lane polls the SGD role's count; once it is there it looks -- once -- at the RLS roles' count of the same step, and
        // at the verdict word.  No acquire: what the trial role takes from other roles (the parameter image, W, w_chol, sigma, rho)
        // it reads with sc1 loads behind this poll and the workgroup barrier (MI355X guide, "sc1 loads in place of the acquire").
        bool rls_now = false;
        auto gate = [&]() {
            if (t > 0) {
                vjf_chaos(tid, cnt + MG_C_SGD, 1);
                if (tid == 0) {
                    const bool there = vjf_poll_count<RLS ? VJF_POLL_SLEEP : VJF_POLL_SLEEP_LITE>(cnt + MG_C_SGD, (unsigned)t * (unsigned)(RLS ? A.n_sgd : A.n_sgd_live), SCW + VJF_SC_STATUS);
                    const bool rls = !rls_in && (int)(__hip_atomic_load(cnt + MG_C_PDONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - (unsigned)t * npost) >= 0;
                    const unsigned mw = __hip_atomic_load(cnt + MG_C_MASK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (!tl || (A.flags & VJF_FLAG_HANDOFF_ACQUIRE)) {         // (parameters read from the state with plain loads; or the conservative hand-off)
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    }
                    s_try[0] = (there ? 1u : 0u) | (rls ? 2u : 0u);
                    s_try[1] = mw;
                    if (!there) vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_GATE);
                    vjf_s_abort_word = (!there || vjf_abort_seen(SCW + VJF_SC_STATUS)) ? 1 : 0;   // (one verdict for the workgroup: vjf_abort_wg)
                }
                __syncthreads(); MG_PHASE();
                rls_now = (s_try[0] & 2u) != 0u;
                const unsigned mw = s_try[1];
                if (!replayed && (mw >> 8) == (unsigned)t) { rbits = mw & 7u; want_replay = true; }
            }
        };
        if (ts >= A.T && gated) gate();                // (behind the last step: only that)
        int it = 0;
        for (int tile = wg; tile < A.ntiles && ts < A.T; tile += A.n_trial, ++it) {
            const bool first = it == 0, last = it == ntl - 1;
            const int b0 = tile * TR;
            const int nb = min(TR, A.B - b0);
            __syncthreads(); MG_PHASE();                           // (the previous tile's readers of the LDS matrices are done)
            // ---- stage 0: inputs.  A tile's rows of y / u / mu_s / lv_s / eps are contiguous in memory: flat coalesced reads, all of a
            //      thread's loads in flight before its first (transposed) LDS write
            {
                auto cell = [&](const float* src, int d, unsigned md, int e, float& v, int& at) {   // element e of a (TR, d) tile -> value, LDS offset
                    const int b = mg_div(e, md), c2 = e - b * d;
                    v = (src != nullptr && b < nb) ? src[(size_t)b0 * d + e] : 0.f;
                    at = c2 * LD + b;
                };
                float vy[4], vs[4], vu = 0.f; int ay[4], as[4], au = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) { vy[q] = 0.f; ay[q] = -1; if (tid + q * NT < TR * dy) cell(y_t, dy, m_dy, tid + q * NT, vy[q], ay[q]); }
                const bool sm = tid < TR * dz;                                  // (dz <= 16: one element of each small tile per thread)
                if (sm) {
                    cell(prior ? nullptr : mu_s, dz, m_dz, tid, vs[0], as[0]);
                    cell(prior ? nullptr : lv_s, dz, m_dz, tid, vs[1], as[1]);
                    cell(eps_s, dz, m_dz, tid, vs[2], as[2]);
                    cell(eps_t, dz, m_dz, tid, vs[3], as[3]);
                    if (prior) {
                        const int j = tid - mg_div(tid, m_dz) * dz;
                        vs[0] = S[P.off[VJF_SLOT_PRIOR_MEAN] + j]; vs[1] = S[P.off[VJF_SLOT_PRIOR_LOGVAR] + j];
                    }
                }
                if (du > 0 && tid < TR * du) cell(u_t, du, m_du, tid, vu, au);
#pragma unroll
                for (int q = 0; q < 4; ++q) if (ay[q] >= 0) s_in[ay[q]] = vy[q];
                if (sm) {
                    s_in[(dy + du) * LD + as[0]] = vs[0];
                    s_in[(dy + du + dz) * LD + as[1]] = vs[1];
                    s_xt[as[2]] = vs[2];                                        // eps_s parked in s_xt
                    s_e2[as[3]] = vs[3];
                }
                if (du > 0 && tid < TR * du) s_in[dy * LD + au] = vu;
                for (int e0 = tid + 4 * NT; e0 < TR * dy; e0 += 4 * NT) {       // (wide observations: further rounds of four)
#pragma unroll
                    for (int q = 0; q < 4; ++q) { vy[q] = 0.f; ay[q] = -1; if (e0 + q * NT < TR * dy) cell(y_t, dy, m_dy, e0 + q * NT, vy[q], ay[q]); }
#pragma unroll
                    for (int q = 0; q < 4; ++q) if (ay[q] >= 0) s_in[ay[q]] = vy[q];
                }
            }
            if (tid < LD) s_one[tid] = tid < nb ? 1.f : 0.f;
            __syncthreads(); MG_PHASE();
            if (first) VJF_MG_STAMP(20);
            {
                for (int e = tid; e < TR * dxu; e += NT) {
                    const int c = e >> 5, b = e & 31;
                    float v;
                    if (c < dz) v = fmaf(s_xt[c * LD + b], expf(0.5f * s_in[(dy + du + dz + c) * LD + b]), s_in[(dy + du + c) * LD + b]);
                    else v = s_in[(dy + c - dz) * LD + b];
                    s_xu[c * LD + b] = v;
                }
                __syncthreads(); MG_PHASE();
                if (first) VJF_MG_STAMP(21);
                // ---- stage 1: RBF features (functional.py:11-22); a replayed pass needs none (its predictive mean / variance are saved)
                if (!replay && !use_mom)
                for (int e = tid; e < TR * n; e += NT) {
                    const int k = e >> 5, b = e & 31;
                    float d2 = 0.f;
                    for (int c = 0; c < dxu; ++c) { const float d = s_xu[c * LD + b] - s_cen[c * npad + k]; d2 = fmaf(d, d, d2); }
                    s_phi[k * LD + b] = expf(d2 * s_iw[k]);
                }
                __syncthreads(); MG_PHASE();
            }
            if (first) VJF_MG_STAMP(2);
            // ---- the RLS update of the previous step (W, w_chol, sigma: write-through stores of the RLS roles), if it is complete
            //      already: its acquire and the L2 warm-up then cost nothing on the path parameters -> forward -> backward.  If not,
            //      the same happens behind the forward pass (below): the values read are the same either way.
            if (first && !replay) {
                rls_in = t == 0 || !mode_rls;
                // (no parameter updates at all: nothing holds this role back between steps but the ring of loss sums -- the role
                //  that sums them must be through with the slot this step will write)
                // (the count only grows: what the last look saw usually covers the next ~30 steps -- a look per step was a memory round
                //  trip and a barrier, 1.2 us of a 20-us step)
                if (!gated && t >= VJF_MG_RING && (int)(ring_seen - (unsigned)(t - VJF_MG_RING + 1) * (unsigned)A.n_sgd_live) < 0) {
                    const unsigned need = (unsigned)(t - VJF_MG_RING + 1) * (unsigned)A.n_sgd_live;
                    vjf_chaos(tid, cnt + MG_C_SGD, 1);
                    if (tid == 0) {
                        bool there = false;
                        unsigned v = 0u;
                        for (unsigned spins = 0; spins < VJF_WAIT_SPINS; ++spins) {       // (its own loop, not vjf_poll_count: the count it saw is kept, ring_seen)
                            v = __hip_atomic_load(cnt + MG_C_SGD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if ((int)(v - need) >= 0) { there = true; break; }
                            if ((spins & 255u) == 255u && vjf_abort_seen(SCW + VJF_SC_STATUS)) break;
                            __builtin_amdgcn_s_sleep(RLS ? VJF_POLL_SLEEP : VJF_POLL_SLEEP_LITE);
                        }
                        if (!there) vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_GATE);
                        s_try[1] = v;
                        vjf_s_abort_word = (!there || vjf_abort_seen(SCW + VJF_SC_STATUS)) ? 1 : 0;
                    }
                    __syncthreads();
                    ring_seen = s_try[1];
                    if (vjf_abort_wg()) return;
                }
                if (t > 0 && mode_rls) {
                    if (tid == 0) {
                        const bool there = (int)(__hip_atomic_load(cnt + MG_C_PDONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - (unsigned)t * npost) >= 0;
                        if (there && (A.flags & VJF_FLAG_HANDOFF_ACQUIRE)) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
                        s_try[0] = there ? 1u : 0u;
                    }
                    __syncthreads(); MG_PHASE();
                    rls_in = s_try[0] != 0u;
                    if (rls_in) mg_warm(A.xt, P.n * P.n, wg, tid);
                }
                if (rls_in) {
                    sig = vjf_ld_sc1(S + P.off[VJF_SLOT_TR_LOGVAR]);
                    tri = tri_launch || vjf_ld_sc1(SCW + VJF_SC_TRI_CLEAN) != 0.f;  // w_chol known upper triangular
                }
                if (t == 0) {                                                 // (the row-major copy of L^-1 of this launch: the inverse loops' first act)
                    if (!mode_rls) {
                        // no RLS roles in this launch: w_chol is a constant of it, and the trial workgroups transpose a share each
                        // (and look at what they move: the state's triangle flag is only set by an RLS update -- a model that has never had
                        //  one, torch.eye (module.py:52), or a state that was just loaded would pay the full square in every variance
                        //  product of the launch although its w_chol is triangular.  A nonzero below the diagonal is counted in the word
                        //  behind the hand-off's own; both travel with the same signal)
                        const float* Wc = S + P.off[VJF_SLOT_W_CHOL];
                        float* xtw = const_cast<float*>(A.xt);
                        bool below = false;
                        for (int e = wg * NT + tid; e < n * n; e += A.n_trial * NT) {
                            const int k = e / n, j = e - k * n;
                            const float v = Wc[e];
                            below = below || (k > j && v != 0.f);
                            vjf_st_wt(xtw + (size_t)j * n + k, v);
                        }
                        if (__syncthreads_or(below ? 1 : 0) && tid == 0) __hip_atomic_fetch_add(cnt + MG_C_XT + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        vjf_wg_signal_wt(cnt + MG_C_XT, tid);
                    }
                    if (!vjf_wg_wait_sc1<RLS ? VJF_POLL_SLEEP : VJF_POLL_SLEEP_LITE>(cnt + MG_C_XT, (unsigned)(mode_rls ? A.n_rls - 2 : A.n_trial), tid, SCW + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u))
                        vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_K1);
                    if (vjf_abort_wg()) return;
                    if (!mode_rls) {
                        tri_launch = __hip_atomic_load(cnt + MG_C_XT + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
                        tri = tri || tri_launch;
                    }
                }
            }
            // (the two halves of stage 2 as routines: the training kernel runs them behind the RLS hand-off, where they always were;
            //  a launch without an RLS update has W, w_chol as constants and runs them BEFORE the gate, in the shadow of the SGD role)
            auto moments_a = [&]() {
            // ---- stage 2: predictive variance sum_j (Phi w_chol)_j^2 (module.py:75-76) and pt.mean = xs + Phi W (module.py:77)
            if (!replay) {
                const __amdgpu_buffer_rsrc_t r_xt = VSPLIT ? vjf_rsrc(A.xt, (size_t)n * n) : vjf_rsrc(A.xt);   // (bounded: rows >= n of the last row tile load zeros, see mg_var2)
                const float* Wm = S + P.off[VJF_SLOT_W_MEAN];
                const int ntile = (n + 15) >> 4;
                float v2a = 0.f, v2b = 0.f;
                // pt.mean: dz <= 16 rows = one tile, K = n: every wavefront takes a K slice behind its variance tiles; the slice's
                // operand loads (at most 16 k-steps when n <= 512) go out now, in front of the variance tiles' own
                const int nsl = min(NW, part_rows / 16);
                const int msl = nsl - 1 - wave;                                // (the last wavefronts have the lightest variance shares)
                const int mper = (((n + 3) >> 2) + nsl - 1) / nsl * 4;
                const int mkb = msl * mper, mke = min(n, (msl + 1) * mper);
                const bool mpre = wave < nsl && ((mke - mkb + 3) >> 2) <= 16;
                float am[16];
                if (mpre && mke > mkb) mg_mma2_ld16(am, Wm, dz, dz, 0, mkb, mke, 0, lane);
                // tiles in descending cost, dealt to the wavefronts in a snake so that the triangular work balances; a wavefront's tiles of
                // two rounds go through mg_var2 as one stream of operand batches
                for (int r = 0; r * NW < ntile; r += 2) {
                    int j0p[2], Kp[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int rr = r + h, idx = (rr & 1) ? rr * NW + NW - 1 - wave : rr * NW + wave;
                        const int tt = ntile - 1 - idx;
                        j0p[h] = (idx < ntile) ? tt * 16 : -1;                  // rows j0 .. j0 + 15 of L^-1 = columns of w_chol
                        Kp[h] = tri ? min(n, tt * 16 + 16) : n;
                    }
                    if (j0p[0] < 0) { j0p[0] = j0p[1]; Kp[0] = Kp[1]; j0p[1] = -1; }
                    mg_var2<VSPLIT>(v2a, v2b, r_xt, n, j0p[0], Kp[0], j0p[1], Kp[1], s_phi, lane);
                }
                if (first) VJF_MG_STAMP(22);
                v2a += __shfl_xor(v2a, 16, 64); v2a += __shfl_xor(v2a, 32, 64);
                v2b += __shfl_xor(v2b, 16, 64); v2b += __shfl_xor(v2b, 32, 64);
                if (lane < 16) { s_red[wave * TR + lane] = v2a; s_red[wave * TR + 16 + lane] = v2b; }
                if (wave < nsl) {
                    const int sl = msl;
                    vjf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                    if (mpre) { if (mke > mkb) mg_mma2_mm16<VSPLIT>(acc0, acc1, am, s_phi, dz, 0, mkb, mke, 0, lane); }
                    else mg_mma2(acc0, acc1, Wm, dz, dz, 0, s_phi, mkb, mke, lane);
                    float* pr = s_part + (size_t)(sl * 16 + 4 * (lane >> 4)) * LD + (lane & 15);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { pr[r * LD] = acc0[r]; pr[r * LD + 16] = acc1[r]; }
                }
                mean_nsl = nsl;
            }
            __syncthreads(); MG_PHASE();
            };
            auto moments_b = [&]() {
            if (!replay) {
                if (tid < TR) {
                    float v = 0.f;
                    for (int w = 0; w < NW; ++w) v += s_red[w * TR + tid];
                    s_plv[tid] = logf(v);
                }
                for (int e = tid; e < TR * dz; e += NT) {
                    const int j = e >> 5, b = e & 31;
                    float v = 0.f;
                    for (int sl = 0; sl < mean_nsl; ++sl) v += s_part[(size_t)(sl * 16 + j) * LD + b];
                    s_pm[j * LD + b] = s_xu[j * LD + b] + v;
                    // warm-up: Phi W for the residual dx - Phi W of the state-noise update (model.py:373-374; W is the launch's constant),
                    // parked in the dmu rows until the loss stage, which has dx, sums the squares
                    if (want_resid) s_dmu[j * LD + b] = v;
                }
            }
            __syncthreads(); MG_PHASE();
            };
            // (the slab traffic of a step flows through the same L2s and pushes L^-1 out of some of them: the workgroups of an XCD bring it
            //  back together, a sixteenth each, before they all walk it -- measured without: one XCD's workgroups 12 us late at the gate)
            if (!RLS && !replay && first && !use_mom) { mg_warm(A.xt, P.n * P.n, wg, tid); mg_warm(S + P.off[VJF_SLOT_W_MEAN], (P.n * P.dz) & ~3, wg, tid); }
            if (!RLS && !replay && !use_mom) { moments_a(); moments_b(); }
            if (!RLS && !replay && first) VJF_MG_STAMPW(2);   // (diagnostic: when this workgroup reached the gate)
            // ---- theta of the previous step.  Nothing above depends on it: the inputs and the features of a step are ready before the
            //      parameters are
            if (first && !replay) {
                if (gated) gate();
                if (gated && t > 0 && vjf_abort_wg()) return;
                if (want_replay) break;                                        // (uniform: every thread read the same word)
                if (t > 0 && !tl) {
                    mg_warm(A.aux, P.aux_len, wg, tid);                        // (see mg_warm)
                    mg_warm(S + P.train_off, P.train_len, wg, tid);
                }
            }
            float4 wv[2];
            const bool warm_now = first && !replay && rls_now && !rls_in;      // the RLS update landed while this workgroup waited for the parameters
            if (first && !replay) rho = vjf_ld_sc1(S + P.off[VJF_SLOT_LIK_LOGVAR]);  // (the SGD role's)
            if (first && !replay && !mode_rls) sig = vjf_ld_sc1(S + P.off[VJF_SLOT_TR_LOGVAR]);   // (warm-up: the SGD role's too; else a constant)
            if (warm_now) {
                mg_warm_issue(A.xt, P.n * P.n, wg, tid, wv);
                sig = vjf_ld_sc1(S + P.off[VJF_SLOT_TR_LOGVAR]);
                tri = vjf_ld_sc1(SCW + VJF_SC_TRI_CLEAN) != 0.f;
                rls_in = true;
            }
            if (first && tl && !replay && t == 0) {                            // (the image of this launch: the SGD role's first act)
                if (!vjf_wg_wait_sc1<RLS ? VJF_POLL_SLEEP : VJF_POLL_SLEEP_LITE>(cnt + MG_C_IMG, (unsigned)A.n_sgd, tid, SCW + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u))
                    vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_GATE);
                if (vjf_abort_wg()) return;
            }
            if (first && tl && !replay && (gated || t == 0)) {                 // (a replayed pass: they are in LDS, untouched since its step; a launch
                                                                               //  that updates nothing: they are the launch's constants, staged once)
                // the parameters of this step into LDS: the image the SGD role keeps has the layout of the region, so this is a flat
                // 16-byte copy with all of a thread's loads in flight -- one round trip
                const __amdgpu_buffer_rsrc_t r_img = vjf_rsrc(A.img);
                float4* dst = reinterpret_cast<float4*>(smem + Lo.th0);
                const int n4 = Lo.th_len >> 2;
                for (int q0 = tid; q0 < n4; q0 += 8 * NT) {
                    float4 v[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) if (q0 + q * NT < n4) v[q] = vjf_ld4_sc1(r_img, (q0 + q * NT) * 4);
#pragma unroll
                    for (int q = 0; q < 8; ++q) if (q0 + q * NT < n4) dst[q0 + q * NT] = v[q];
                }
                __syncthreads(); MG_PHASE();
            }
            if (warm_now) mg_warm_retire(wv);
            if (first) { VJF_MG_STAMP(1); VJF_MG_STAMPX(27, -1); VJF_MG_STAMPW(0); }
            if (first && A.stamps && tid == 0 && t == A.T - 1 && !replay) {
                unsigned xcc;
                unsigned hwid;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
                A.stamps[1024 + (size_t)wg * 8 + 6] = (xcc & 15u) | ((unsigned long long)hwid << 8);
                A.stamps[1024 + (size_t)wg * 8 + 7] = rls_in ? 1u : 0u;
            }
            // ---- stage 3: recognition forward (recognition.py:31-42)
            {
                const float* xin = s_in;
                int kin = din, aoff = 0;
                for (int l = 0; l < P.L; ++l) {
                    const float* WT = A.aux + P.aux_recT[l];                   // (kin, hl)
                    int th_w = 0, th_ldw = 0, th_b = 0;
                    if (tl) mg_theta_layer(P, Lo.th0, l, th_w, th_ldw, th_b);
                    // (bias values through a select of two TYPED loads, never a load through a selected pointer: a pointer that is LDS on
                    //  one side and memory on the other is a generic one, and the aperture test the backend builds for it is the instruction
                    //  this compiler rejects -- "V_CMP_NE_U32_e32 0, $src_shared_base", found with -mllvm -verify-machineinstrs)
                    const float* bias_l = smem + th_b; const float* bias_g = S + P.off[VJF_SLOT_REC_B0 + 2 * l];
                    float* out = s_act + aoff * LD;
                    const int hl = P.h[l], mt = (hl + 15) >> 4;
                    for (int tt = wave; tt < mt; tt += NW) {
                        vjf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                        if (tl) mg_mma2_lds<false>(acc0, acc1, smem + th_w, th_ldw, hl, tt * 16, xin, 0, kin, lane);
                        else mg_mma2(acc0, acc1, WT, hl, hl, tt * 16, xin, 0, kin, lane);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int f = tt * 16 + 4 * (lane >> 4) + r;
                            if (f < hl) {
                                const float bf = tl ? ((mg_lds_cf*)bias_l)[f] : ((mg_glb_cf*)bias_g)[f];
                                if (ACT) {
                                    out[f * LD + (lane & 15)] = vjf_act_fwd(act, acc0[r] + bf);
                                    out[f * LD + 16 + (lane & 15)] = vjf_act_fwd(act, acc1[r] + bf);
                                } else {
                                    out[f * LD + (lane & 15)] = mg_tanh(acc0[r] + bf);
                                    out[f * LD + 16 + (lane & 15)] = mg_tanh(acc1[r] + bf);
                                }
                            }
                        }
                    }
                    __syncthreads(); MG_PHASE();
                    xin = out; kin = hl; aoff += hl;
                }
                if (first) VJF_MG_STAMP(23);
                // heads: 2 dz <= 32 rows = at most two 16-row tiles -- the K range is split over the wavefronts, partial tiles meet in
                // LDS (s_part: a region that is free until the losses / the backward pass) and are summed in slice order
                const float* HT = A.aux + P.aux_headT;                         // (hL, 2dz): mean rows then logvar rows
                const int mt = (2 * dz + 15) >> 4;
                const int nsl = min(NW / mt, part_rows / (16 * mt));
                if (wave < mt * nsl) {
                    const int tt = wave / nsl, sl = wave - tt * nsl;
                    const int per = (((kin + 3) >> 2) + nsl - 1) / nsl * 4;
                    vjf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                    if (tl) mg_mma2_lds<false>(acc0, acc1, smem + Lo.th_head, Lo.th_ldh, 2 * dz, tt * 16, xin, sl * per, min(kin, (sl + 1) * per), lane);
                    else mg_mma2(acc0, acc1, HT, 2 * dz, 2 * dz, tt * 16, xin, sl * per, min(kin, (sl + 1) * per), lane);
                    float* pr = s_part + (size_t)((sl * mt + tt) * 16 + 4 * (lane >> 4)) * LD + (lane & 15);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { pr[r * LD] = acc0[r]; pr[r * LD + 16] = acc1[r]; }
                }
                __syncthreads(); MG_PHASE();
                if (first) VJF_MG_STAMP(24);
                const float* bl_l = smem + Lo.th_bl; const float* bl_g = S + P.off[VJF_SLOT_LV_B];
                for (int e = tid; e < TR * 2 * dz; e += NT) {
                    const int f = e >> 5, b = e & 31;
                    float v = 0.f;
                    for (int sl = 0; sl < nsl; ++sl) v += s_part[(size_t)((sl * mt + (f >> 4)) * 16 + (f & 15)) * LD + b];
                    if (f < dz) s_mu[f * LD + b] = v; else s_lv[(f - dz) * LD + b] = v + (tl ? ((mg_lds_cf*)bl_l)[f - dz] : ((mg_glb_cf*)bl_g)[f - dz]);
                }
            }
            __syncthreads(); MG_PHASE();
            if (first) VJF_MG_STAMP(3);
            // ---- stage 4: xt, dx, posterior out, py = xt C^T + d (model.py:28-30)
            for (int e = tid; e < TR * dz; e += NT) {
                const int j = e >> 5, b = e & 31;
                const float xt = fmaf(s_e2[j * LD + b], expf(0.5f * s_lv[j * LD + b]), s_mu[j * LD + b]);
                s_xt[j * LD + b] = xt;
                s_dx[j * LD + b] = b < nb ? xt - s_xu[j * LD + b] : 0.f;
            }
            if (!replay) {
                // posterior out (write-through: the Gram role forms the next step's features from it).  The tile's rows are contiguous
                // in memory: four consecutive elements per 16-byte store where the tile starts on a 16-byte boundary (a quarter of
                // the fabric writes: 82 k scalar ones per step at config B before), scalar stores for what is left over
                float* mrow = mu_t + (size_t)b0 * dz;
                float* lrow = lv_t + (size_t)b0 * dz;
                const int ne = nb * dz;
                const int n4 = ((((size_t)mrow | (size_t)lrow) & 15u) == 0) ? (ne >> 2) : 0;
                for (int e4 = tid; e4 < n4; e4 += NT) {
                    float vm[4], vl[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int e = 4 * e4 + c, b = mg_div(e, m_dz), j = e - b * dz;
                        vm[c] = s_mu[j * LD + b]; vl[c] = s_lv[j * LD + b];
                    }
                    vjf_st4_wt(mrow + 4 * e4, vm[0], vm[1], vm[2], vm[3]);
                    vjf_st4_wt(lrow + 4 * e4, vl[0], vl[1], vl[2], vl[3]);
                }
                for (int e = 4 * n4 + tid; e < ne; e += NT) {
                    const int b = mg_div(e, m_dz), j = e - b * dz;
                    vjf_st_wt(mrow + e, s_mu[j * LD + b]);
                    vjf_st_wt(lrow + e, s_lv[j * LD + b]);
                }
                // (the moments role's tag for this posterior goes out behind the decoder, below: its stores are acknowledged by then, and
                //  a drain here was 1.5 us on the path of every step; the moments role is a step ahead)
            }
            __syncthreads(); MG_PHASE();
            {
                // sum |dx|^2 per trial (16 lanes each), then the tile's sum in trial order
                constexpr int LPT = NT / TR;
                const int b = tid / LPT, sl = tid % LPT;
                float sdx2 = 0.f;
                for (int j = sl; j < dz; j += LPT) { const float dx = s_dx[j * LD + b]; sdx2 = fmaf(dx, dx, sdx2); }
                sdx2 = group_sum<LPT>(sdx2);
                if (sl == 0) s_sc[b * RS_N + RS_SDX2] = sdx2;
            }
            {
                const float* CT = A.aux + P.aux_decT;                          // (dz, dy)
                const float* d_l = smem + Lo.th_bd; const float* d_g = S + P.off[VJF_SLOT_DEC_B];
                const int mt = (dy + 15) >> 4;
                for (int tt = wave; tt < mt; tt += NW) {
                    vjf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                    if (tl) mg_mma2_lds<false>(acc0, acc1, smem + Lo.th_dec, Lo.th_ldd, dy, tt * 16, s_xt, 0, dz, lane);
                    else mg_mma2(acc0, acc1, CT, dy, dy, tt * 16, s_xt, 0, dz, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = tt * 16 + 4 * (lane >> 4) + r;
                        if (f < dy) { const float df = tl ? ((mg_lds_cf*)d_l)[f] : ((mg_glb_cf*)d_g)[f]; s_py[f * LD + (lane & 15)] = acc0[r] + df; s_py[f * LD + 16 + (lane & 15)] = acc1[r] + df; }
                    }
                }
            }
            if (first) VJF_MG_STAMP(25);
            // early slab: Phi^T dx of this tile (module.py:94), 16 features x 16 columns per MFMA tile, K = 32 trials
            if (!replay && mode_rls) {
                const int mt = (n + 15) >> 4;
                for (int tt = NW - 1 - wave; tt < mt; tt += NW) {
                    const int m0 = tt * 16, i = lane & 15, kk = lane >> 4;
                    const float* arow = ((m0 + i) < n ? s_phi + (size_t)(m0 + i) * LD : s_zero) + kk;
                    const float* brow = (i < dz ? s_dx + (size_t)i * LD : s_zero) + kk;
                    float a[8], b[8];
#pragma unroll
                    for (int s = 0; s < 8; ++s) { a[s] = arow[4 * s]; b[s] = brow[4 * s]; }
                    vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < 8; s += 2) {
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s + 1], b[s + 1], acc1, 0, 0, 0);
                    }
                    acc += acc1;
                    // [dz column][feature]: a lane's four registers are four consecutive features of one column (features >= n: the
                    // zero row of the A operand)
                    const int fq = m0 + 4 * (lane >> 4), col = lane & 15;
                    if (col < dz && fq < ldn) {
                        float* p = early + (size_t)col * ldn + fq;
                        if (!first) { acc[0] += vjf_ld_sc1(p); acc[1] += vjf_ld_sc1(p + 1); acc[2] += vjf_ld_sc1(p + 2); acc[3] += vjf_ld_sc1(p + 3); }
                        vjf_st4_wt(p, acc[0], acc[1], acc[2], acc[3]);
                    }
                }
            }
            // (a look at the RLS hand-off of the previous step by one lane in front of this barrier, where the other wavefronts are
            //  still storing their slab tiles: see fuse_fwd)
            if (tid == 0 && first && last && !replay && !rls_in)
                s_wg[15] = ((int)(__hip_atomic_load(cnt + MG_C_PDONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - (unsigned)t * npost) >= 0) ? 1.f : 0.f;
            if (use_mom && !replay) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the tile's posterior is in memory: its tag follows the barrier)
            __syncthreads(); MG_PHASE();
            if (use_mom && !replay && tid == 0) __hip_atomic_store(cnt + MG_C_TAG_POST + tile, (unsigned)(tc + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // A launch without parameter updates has nothing between its steps to hide the next step's inputs behind (2.5 us of a 20-us
            // step: y, the noise): one load per 128-byte line of them goes out here and is retired behind the moments' own loads --
            // the staging of the next step then finds them in the caches.
            float touch = 0.f;
            if (!gated && !replay && last && tc + 1 < A.T) {
                const int tn = wg;                                   // (the next step starts with this workgroup's first tile)
                const int b0n = tn * TR, nbn = min(TR, A.B - b0n);
                const int ly = (nbn * dy + 31) / 32 + 1, le = (nbn * dz + 31) / 32 + 1;
                const float* yn = A.y + (size_t)(tc + 1) * sy + (size_t)b0n * dy;
                const float* en = A.eps + (size_t)(tc + 1) * 2 * sz + (size_t)b0n * dz;
                const float* tp = nullptr;
                if (tid < ly) tp = yn + min(tid * 32, nbn * dy - 1);
                else if (tid < ly + le) tp = en + min((tid - ly) * 32, nbn * dz - 1);
                else if (tid < ly + 2 * le) tp = en + sz + min((tid - ly - le) * 32, nbn * dz - 1);
                if (tp) touch = *tp;
            }
            if (tid == 0 && !replay && mode_rls) {
                float v = 0.f;
                for (int bb = 0; bb < TR; ++bb) v += s_sc[bb * RS_N + RS_SDX2];
                s_wg[RS_SDX2] += v;
                if (last) vjf_st_wt(early + (size_t)16 * ldn + RS_SDX2, s_wg[RS_SDX2]);
            }
            if (first) VJF_MG_STAMP(26);
            // One tile per workgroup and the RLS update of the previous step still to be taken in, but there by now (config B: it
            // lands ~5 us before this point): the early slab's write-through stores are not drained here -- their acknowledgements
            // travel beside the round trips of that hand-off, below, and the "forward done" count follows there (one drain, one
            // barrier less).  If it is NOT there yet (configs whose RLS loop alone bounds the step, e.g. one trial against RBF(100):
            // the wait below lasts ~10 us) the count goes out now -- the Gram role's sums of the next step, and with them the next
            // factorisation, wait for it (measured at configs[0]: 35.2 us a step with the count behind the wait, 30.0 before it).
            const bool fuse_fwd = first && last && !replay && !rls_in && s_wg[15] != 0.f;
            if (last && !replay && !fuse_fwd && mode_rls) vjf_wg_signal_wt(cnt + MG_C_FWD, tid);
            if (first) VJF_MG_STAMP(4);
            if (last) { VJF_MG_STAMPX(28, -1); VJF_MG_STAMPW(1); }
            // ---- the RLS update of the previous step, if it had not landed before the forward pass
            float4 wv_late[2];
            bool warm_late = false;
            if (first && !rls_in) {
                if (!vjf_wg_wait_sc1<RLS ? VJF_POLL_SLEEP : VJF_POLL_SLEEP_LITE>(cnt + MG_C_PDONE, (unsigned)t * npost, tid, SCW + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u))
                    vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_K1);
                if (vjf_abort_wg()) return;
                // (sigma and the triangle flag first, then this workgroup's share of the L2 warm-up with its loads left in flight: the
                //  variance tiles' own operand loads go out behind them instead of waiting a round trip for them)
                sig = vjf_ld_sc1(S + P.off[VJF_SLOT_TR_LOGVAR]);
                tri = vjf_ld_sc1(SCW + VJF_SC_TRI_CLEAN) != 0.f;
                if (fuse_fwd) {
                    // every wavefront's stores of the forward pass (posterior, early slab) and these two loads are behind it: the count
                    // the operand and Gram roles wait for
                    vjf_chaos(tid, cnt + MG_C_FWD, 2);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                    if (tid == 0) __hip_atomic_fetch_add(cnt + MG_C_FWD, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                mg_warm_issue(A.xt, P.n * P.n, wg, tid, wv_late);
                warm_late = true;
            }
            if (first) { VJF_MG_STAMP(5); if (RLS) VJF_MG_STAMPW(2); }
            if (use_mom && !replay) {
                // the tile's moments of this step from the moments role: its tag, then pt.mean | Phi W | pt.logvar with sc1 loads
                if (!vjf_wg_wait_sc1<RLS ? VJF_POLL_SLEEP : VJF_POLL_SLEEP_LITE>(cnt + MG_C_TAG_MOM + tile, (unsigned)(tc + 1), tid, SCW + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u))
                    vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_K1);
                if (vjf_abort_wg()) return;
                const float* mb = A.mom + ((size_t)tile * 2 + (size_t)(tc & 1)) * (size_t)((2 * dz + 1) * TR);
                for (int e = tid; e < TR * (2 * dz + 1); e += NT) {
                    const int j = e >> 5, b = e & 31;
                    const float v = vjf_ld_sc1(mb + e);
                    if (j < dz) s_pm[j * LD + b] = v;
                    else if (j < 2 * dz) { if (want_resid) s_dmu[(j - dz) * LD + b] = v; }
                    else s_plv[b] = v;
                }
                __syncthreads(); MG_PHASE();
            }
            asm volatile("" ::"v"(touch));
            if (RLS) moments_a();
            if (warm_late) mg_warm_retire(wv_late);
            if (last && tid == 0 && !replay && mode_rls) __hip_atomic_fetch_add(cnt + MG_C_K1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // W, w_chol, sigma read
            if (RLS) moments_b();
            // pt.mean | pt.logvar of the tile's trials: kept for a replay of this step (by then W and w_chol have moved on)
            if (do_sgd)
            for (int e = tid; e < TR * (dz + 1); e += NT) {
                const int j = e >> 5, b = e & 31;
                if (b < nb) {
                    float* sv = A.pmsave + (size_t)(b0 + b) * (dz + 1) + j;
                    if (!replay) *sv = j < dz ? s_pm[j * LD + b] : s_plv[b];
                    else if (j < dz) s_pm[j * LD + b] = *sv;
                    else s_plv[b] = *sv;
                }
            }
            if (replay) { __syncthreads(); MG_PHASE(); }
            if (first) VJF_MG_STAMP(10);
            if (first) { VJF_MG_STAMP(6); VJF_MG_STAMPW(3); }
            // ---- stage 5: per-trial loss terms and backward seeds (no 1/B); 16 lanes per trial
            {
                constexpr int LPT = NT / TR;
                const int b = tid / LPT, s = tid % LPT;
                const bool ok = b < nb;
                float lrec = 0.f, ssey = 0.f;
                if (P.lik == VJF_LIK_GAUSSIAN) {
                    const float p = expf(-0.5f * rho), e = expf(-rho);
                    for (int i = s; i < dy; i += LPT) {
                        const float seed = vjf_gauss_recon(s_in[i * LD + b], s_py[i * LD + b], rho, p, e, lrec, ssey);
                        s_dpy[i * LD + b] = (ok && m_r) ? seed : 0.f;
                    }
                } else {
                    for (int i = s; i < dy; i += LPT) {
                        const float seed = vjf_poisson_recon(s_in[i * LD + b], s_py[i * LD + b], lrec, ssey);
                        s_dpy[i * LD + b] = (ok && m_r) ? seed : 0.f;
                    }
                }
                lrec = group_sum<LPT>(lrec);
                ssey = group_sum<LPT>(ssey);
                float ldyn = 0.f, ent = 0.f, rsd = 0.f;
                {
                    const float p = expf(-0.5f * sig), e = expf(-sig), plv = s_plv[b];
                    for (int j = s; j < dz; j += LPT) {
                        if (want_resid) { const float r = s_dx[j * LD + b] - s_dmu[j * LD + b]; rsd = fmaf(r, r, rsd); }   // (read before dmu goes there)
                        const VjfDynSeed sd = vjf_dyn_term(s_pm[j * LD + b], s_mu[j * LD + b], s_lv[j * LD + b], plv, sig, p, e, !warm && m_d, m_h, ldyn, ent);
                        s_dmu[j * LD + b] = ok ? sd.dmu : 0.f;
                        s_dlv[j * LD + b] = ok ? sd.dlv : 0.f;
                    }
                }
                ldyn = group_sum<LPT>(ldyn);
                ent = group_sum<LPT>(ent);
                if (want_resid) rsd = group_sum<LPT>(rsd);
                if (s == 0) {
                    s_sc[b * RS_N + RS_RESID] = ok ? rsd : 0.f;
                    s_sc[b * RS_N + RS_LRECON] = ok ? lrec : 0.f;
                    s_sc[b * RS_N + RS_LDYN] = ok ? ldyn : 0.f;
                    s_sc[b * RS_N + RS_ENT] = ok ? ent : 0.f;
                    s_sc[b * RS_N + RS_SSEY] = ok ? ssey : 0.f;
                }
            }
            __syncthreads(); MG_PHASE();
            if (first) VJF_MG_STAMP(31);
#ifdef VJF_EXPERIMENT_SLOW_TRIAL   /* sensitivity experiment: every trial workgroup held for this many 10-ns ticks per step */
            { const unsigned long long t0_ = wall_clock64(); while (wall_clock64() - t0_ < VJF_EXPERIMENT_SLOW_TRIAL) __builtin_amdgcn_s_sleep(1); }
#endif
            if ((tid < RS_SDX2 || (tid == RS_RESID && want_resid)) && !replay) {   // (RS_LRECON, RS_LDYN, RS_ENT, RS_SSEY; the residual)
                float v = 0.f;
                for (int bb = 0; bb < TR; ++bb) v += s_sc[bb * RS_N + tid];
                s_wg[tid] += v;
            }
            // ---- stage 6: backward.  dxt = dpy C ; dmu += dxt ; dlv += dxt eps_t exp(lv/2)/2.  Every product whose A
            //      operand comes from memory runs BEFORE the first gradient tile goes out: a load issued behind write-through stores
            //      waits for them to reach memory (vmcnt counts in order).
            if (do_sgd) {
            int gbase = 0;                                                     // running tile count: gradient tiles go round the wavefronts
            int gq = wave;                                                     // GTAB: this wavefront's next tile of the table
            auto grad_walk = [&](int seg) {                                    // its tiles of segment `seg` (ends: header words 2 ..)
                const int* gtab = A.sl_grp + VJF_GT_AT(A.slab_len);                // (the table lies behind the slab's group words)
                mg_grad_walk<false>(gtab, gq, ((mg_cst_i*)gtab)[2 + seg], smem, Lo.one, Lo.zero, late, first, lane);
            };
            auto grad_tensor = [&](const float* D, int M, const float* Bact, int Kin, int blkid) {
                int b_off, b_ldm, b_rows;
                mg_slab_block(P, blkid, b_off, b_ldm, b_rows);
                const int ntm = (M + 15) >> 4, ntj = (Kin + 1 + 15) >> 4;
                const unsigned mj = mg_magic(ntj);
                for (int q = (wave - gbase) & (NW - 1); q < ntm * ntj; q += NW) {                   // this wavefront's tiles of the tensor
                    const int tm = mg_div(q, mj), tj = q - tm * ntj;
                    mg_grad_tile(D, M, tm * 16, Bact, Kin, tj * 16, s_one, s_zero, late + b_off, b_ldm, b_rows, first, lane);
                }
                gbase += ntm * ntj;
            };
            {
                const float* C = S + P.off[VJF_SLOT_DEC_W];                    // (dy, dz): k-major for this product
                const int mt = (dz + 15) >> 4;
                // dz <= 16 rows = ONE tile: the K range (the observations) is split over the wavefronts, as the heads' is -- one wavefront
                // alone took 3.9 us for it while seven waited.  The partial tiles meet in rows that are dead here: the decoder's
                // means (consumed by the losses) or the delta buffers (written from the next stage on).
                float* s_kp = compact ? s_py : s_dd;
                const int rows_av = compact ? dy : Lo.nd * P.hmax;
                const int nslb = min(NW / mt, rows_av / (16 * mt));
                if (nslb >= 2) {
                    if (wave < mt * nslb) {
                        const int tt = wave / nslb, sl = wave - tt * nslb;
                        const int per = (((dy + 3) >> 2) + nslb - 1) / nslb * 4;
                        vjf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                        if (tl) mg_mma2_lds<true>(acc0, acc1, smem + Lo.th_dec, Lo.th_ldd, dz, tt * 16, s_dpy, sl * per, min(dy, (sl + 1) * per), lane);
                        else mg_mma2(acc0, acc1, C, dz, dz, tt * 16, s_dpy, sl * per, min(dy, (sl + 1) * per), lane);
                        float* pr = s_kp + (size_t)((sl * mt + tt) * 16 + 4 * (lane >> 4)) * LD + (lane & 15);
#pragma unroll
                        for (int r = 0; r < 4; ++r) { pr[r * LD] = acc0[r]; pr[r * LD + 16] = acc1[r]; }
                    }
                    __syncthreads(); MG_PHASE();
                    for (int e = tid; e < TR * dz; e += NT) {
                        const int j = e >> 5, b = e & 31;
                        float a = 0.f;
                        for (int sl = 0; sl < nslb; ++sl) a += s_kp[(size_t)((sl * mt + (j >> 4)) * 16 + (j & 15)) * LD + b];   // (padding trials: dpy = 0, so a = 0)
                        s_dmu[j * LD + b] += a;
                        s_dlv[j * LD + b] = fmaf(a * s_e2[j * LD + b], 0.5f * expf(0.5f * s_lv[j * LD + b]), s_dlv[j * LD + b]);
                    }
                } else
                for (int tt = wave; tt < mt; tt += NW) {
                    vjf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                    if (tl) mg_mma2_lds<true>(acc0, acc1, smem + Lo.th_dec, Lo.th_ldd, dz, tt * 16, s_dpy, 0, dy, lane);
                    else mg_mma2(acc0, acc1, C, dz, dz, tt * 16, s_dpy, 0, dy, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = tt * 16 + 4 * (lane >> 4) + r;
                        if (j < dz) {
#pragma unroll
                            for (int g = 0; g < 2; ++g) {
                                const int b = 16 * g + (lane & 15);
                                const float a = g ? acc1[r] : acc0[r];         // (padding trials: dpy = 0, so a = 0)
                                s_dmu[j * LD + b] += a;
                                s_dlv[j * LD + b] = fmaf(a * s_e2[j * LD + b], 0.5f * expf(0.5f * s_lv[j * LD + b]), s_dlv[j * LD + b]);
                            }
                        }
                    }
                }
            }
            __syncthreads(); MG_PHASE();
            if (first) VJF_MG_STAMP(7);
            {
                const int hL = P.h[P.L - 1];
                const float* Wm = S + P.off[VJF_SLOT_MEAN_W];                  // (dz, hL): k-major for dh = dmu Wm + dlv Wl
                const float* Wl = S + P.off[VJF_SLOT_LV_W];
                const float* hact = s_act + (P.hsum - hL) * LD;
                // dh_{l-1} = da_l W_l (1 - h_{l-1}^2)  into `dst`   (l = L: the heads; ACT: act'(h_{l-1}) in place of 1 - h^2)
                auto delta = [&](int l, const float* src, float* dst) {
                    const int hp = P.h[l - 1];
                    int aoff = 0;
                    for (int q = 0; q < l - 1; ++q) aoff += P.h[q];
                    const float* hprev = s_act + aoff * LD;
                    const int mt = (hp + 15) >> 4;
                    int d_w = 0, d_ldw = 0, d_b = 0;
                    if (tl && l < P.L) mg_theta_layer(P, Lo.th0, l, d_w, d_ldw, d_b);
                    for (int tt = wave; tt < mt; tt += NW) {
                        vjf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                        if (l == P.L) {
                            if (tl) {
                                mg_mma2_lds<true>(acc0, acc1, smem + Lo.th_head, Lo.th_ldh, hL, tt * 16, s_dmu, 0, dz, lane);
                                mg_mma2_lds<true>(acc0, acc1, smem + Lo.th_head + dz * Lo.th_ldh, Lo.th_ldh, hL, tt * 16, s_dlv, 0, dz, lane);
                            } else {
                                mg_mma2(acc0, acc1, Wm, hL, hL, tt * 16, s_dmu, 0, dz, lane);
                                mg_mma2(acc0, acc1, Wl, hL, hL, tt * 16, s_dlv, 0, dz, lane);
                            }
                        } else if (tl) {
                            mg_mma2_lds<true>(acc0, acc1, smem + d_w, d_ldw, hp, tt * 16, src, 0, P.h[l], lane);
                        } else {
                            mg_mma2(acc0, acc1, S + P.off[VJF_SLOT_REC_W0 + 2 * l], hp, hp, tt * 16, src, 0, P.h[l], lane);   // (h_l, h_{l-1}): k-major
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int k = tt * 16 + 4 * (lane >> 4) + r, b = lane & 15;
                            if (k < hp) {
                                const float h0 = hprev[k * LD + b], h1 = hprev[k * LD + 16 + b];
                                if (ACT) {
                                    dst[k * LD + b] = acc0[r] * vjf_act_dh(act, h0);
                                    dst[k * LD + 16 + b] = acc1[r] * vjf_act_dh(act, h1);
                                } else {
                                    dst[k * LD + b] = acc0[r] * (1.f - h0 * h0);
                                    dst[k * LD + 16 + b] = acc1[r] * (1.f - h1 * h1);
                                }
                            }
                        }
                    }
                };
                auto layer_grads = [&](int l, const float* da) {               // weights / bias of recognition layer l from da_l and its input
                    int aoff = 0;
                    for (int q = 0; q < l - 1; ++q) aoff += P.h[q];
                    grad_tensor(da, P.h[l], l > 0 ? s_act + aoff * LD : s_in, l > 0 ? P.h[l - 1] : din, 3 + (P.L - 1 - l));
                };
                delta(P.L, nullptr, s_d0);                                     // da_{L-1}
                __syncthreads(); MG_PHASE();
                if (P.L >= 2) { delta(P.L - 1, s_d0, s_d1); __syncthreads(); MG_PHASE(); } // da_{L-2}
                if (first) VJF_MG_STAMP(19);
                // gradient tiles (write-through stores into the workgroup's late slab)
                if constexpr (GTAB) grad_walk(0);
                else {
                    grad_tensor(s_dpy, dy, s_xt, dz, 0);
                    grad_tensor(s_dmu, dz, hact, hL, 1);
                    grad_tensor(s_dlv, dz, hact, hL, 2);
                    layer_grads(P.L - 1, s_d0);
                    if (P.L >= 2) layer_grads(P.L - 2, s_d1);
                }
                float* cur = s_d1; float* nxt = s_d0;                          // deeper networks: the two delta buffers alternate
                for (int l = P.L - 3; l >= 0; --l) {
                    __syncthreads(); MG_PHASE();
                    delta(l + 1, cur, nxt);
                    __syncthreads(); MG_PHASE();
                    if constexpr (GTAB) grad_walk(P.L - 2 - l);
                    else layer_grads(l, nxt);
                    float* tmp = cur; cur = nxt; nxt = tmp;
                }
            }
            }
            if (first) { VJF_MG_STAMP(8); VJF_MG_STAMPW(4); }
            if (last) {
                // the workgroup's late slab is complete: loss sums, then the signal the SGD role waits for
                __syncthreads(); MG_PHASE();
                if ((tid < RS_SDX2 || (tid == RS_RESID && want_resid)) && !replay) vjf_st_wt(late + A.slab_len + 8 * (tc % VJF_MG_RING) + tid, s_wg[tid]);
                if (gated) vjf_wg_signal_wt(cnt + (replay ? MG_C_REDO_B : MG_C_BWD), tid);
                else {
                    // No gate between the steps of this launch (nothing changes between them): the trial workgroups are not in step
                    // with each other and no role waits for them.  Each counts itself in at the step's word of a ring; the one whose
                    // add comes LAST (told by the value the add returns: every other workgroup's sums are in memory, drained before
                    // its add) sums the step's loss terms in the fixed order, writes the loss, puts the word back to 0 and counts the
                    // step as done -- the count that keeps any workgroup from running a ring's length ahead.
                    vjf_chaos(tid, cnt + MG_C_ARR, 2);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                    if (tid == 0) s_try[0] = __hip_atomic_fetch_add(cnt + MG_C_ARR + (tc % VJF_MG_RING), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == (unsigned)A.n_trial ? 1u : 0u;
                    __syncthreads(); MG_PHASE();
                    if (s_try[0]) {
                        float* s_tot = s_sc;                                   // (the per-trial terms of this workgroup's tile are summed and stored)
                        mg_sum_losses(A, tc, s_tot, tid, (float)A.B, dz, false);
                        if (tid == 0) {
                            const VjfLossVerdict v = vjf_loss_verdict(s_tot[RS_LRECON], s_tot[RS_LDYN], s_tot[RS_ENT], 1.0f / (float)A.B, warm);
                            if (A.loss) vjf_put_loss4(A.loss + 4 * (size_t)tc, v);
                            if (v.status()) vjf_status_or(SCW + VJF_SC_STATUS, v.status());
                            __hip_atomic_store(cnt + MG_C_ARR + (tc % VJF_MG_RING), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                            __hip_atomic_fetch_add(cnt + MG_C_SGD, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        __syncthreads(); MG_PHASE();
                    }
                }
                VJF_MG_STAMP(9);
                VJF_MG_STAMPX(29, 30);
                VJF_MG_STAMPW(5);
            }
        }
        VJF_MG_STAMP(18);
        if (want_replay) { replay = true; continue; }
        if (replay) {
            // the SGD role's step on the replayed late slabs; then this step starts over (inputs, features, parameters)
            ++nredo;
            if (!(tl ? vjf_wg_wait_sc1<RLS ? VJF_POLL_SLEEP : VJF_POLL_SLEEP_LITE>(cnt + MG_C_REDO_S, nredo * (unsigned)A.n_sgd, tid, SCW + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u)
                     : vjf_wg_wait(cnt + MG_C_REDO_S, nredo * (unsigned)A.n_sgd, tid, SCW + VJF_SC_STATUS)))
                vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_GATE);
            if (vjf_abort_wg()) return;
            replay = false; replayed = true; rbits = 0;
            continue;
        }
        sig_prev = sig; rho_prev = rho;
        break;
      }
    }
}
