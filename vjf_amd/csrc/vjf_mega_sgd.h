// vjf_mega_sgd.h -- the SGD role of the one-launch route (vjf_mega_kernel.h), and the parameter image of the launches without one.
#pragma once
#include "vjf_mega_common.h"

// ------------------------------------------------------------------------------------------------ SGD role
template <bool RLS>
__device__ __forceinline__ void vjf_mega_sgd(const VjfPlan& P, const VjfMegaArgs& A, float* lds, const int sw) {
    constexpr int NT = VJF_MG_THREADS;
    const int tid = threadIdx.x;
    float* s_sc = lds;                                 // RS_N loss sums
    float* S = A.state;
    float* SC = S + P.off[VJF_SLOT_SCALARS];
    const float Bf = (float)A.B, invB = 1.0f / Bf;
    // (set by the host between launches, never inside one)
    const float lr_dec = SC[VJF_SC_LR_DEC], lr_rec = SC[VJF_SC_LR_REC];
    const bool freeze = SC[VJF_SC_FREEZE_DEC] != 0.f;
    const bool tl = vjf_mega_trial_lds<false>(P, A.lds_floats).theta != 0;   // the trial role reads the LDS image (else: the state and its transposed copies)
    // the flags of VJF.filter for the steps of this launch (vjf/model.py:179-221; see vjf_mega_trial)
    const bool do_sgd = RLS || (A.flags & VJF_FLAG_SGD) != 0u, do_upd = RLS || (A.flags & VJF_FLAG_UPDATE) != 0u;
    const bool warm = !RLS && (A.flags & VJF_FLAG_WARM_UP) != 0u;
    constexpr bool mode_rls = RLS;
    const int n_live = RLS ? A.n_sgd : A.n_sgd_live;
    // a quad of the slab (four consecutive output units of one input: vjf_mega_slab_layout) per 8 lanes: lane p sums the late slabs [p npq, (p+1) npq) (16-byte loads, all in flight together with
    // the quad's old values, its table entries and the step's loss sums), then a fixed xor tree; lane 0 of the group clips and
    // steps its four parameters (vjf_sgd_step)
    const int npq = (A.n_trial + 7) >> 3, part = tid & 7;
    const int nquad = A.slab_len >> 2, qstride = (A.n_sgd * NT) >> 3;
    const int w1 = min(A.n_trial, (part + 1) * npq);
    // Every byte this role takes from the trial role (late slabs, loss sums) is read with sc1 loads behind the count's poll and the
    // workgroup barrier: no agent-scope acquire (vjf_wg_wait_sc1)
    const __amdgpu_buffer_rsrc_t r_late = vjf_rsrc(A.slab_late);
    // A lane group serves the same quads in every step: the table entries and the parameters of its first round stay in
    // registers for the whole launch (a longer parameter vector reads the later rounds' from memory each step)
    const int q00 = (sw * NT) >> 3;
    int4 k_pi, k_ci;
    int k_grp;
    float k_w[4];
    auto fetch = [&](int quad, int4& pi, int4& ci, int& grp, float (&w)[4]) {
        pi = make_int4(-1, -1, -1, -1); ci = pi; grp = 0;
        w[0] = w[1] = w[2] = w[3] = 0.f;
        if (quad < nquad && part == 0) {
            pi = *reinterpret_cast<const int4*>(A.sl_pidx + (size_t)quad * 4);
            ci = *reinterpret_cast<const int4*>(A.sl_cidx + (size_t)quad * 4);
            grp = A.sl_grp[quad];
            const float* th = S + P.train_off;
            if (pi.x >= 0) w[0] = vjf_ld_sc1(th + pi.x);                                // (this lane's own stores of the step before)
            if (pi.y >= 0) w[1] = vjf_ld_sc1(th + pi.y);
            if (pi.z >= 0) w[2] = vjf_ld_sc1(th + pi.z);
            if (pi.w >= 0) w[3] = vjf_ld_sc1(th + pi.w);
        }
    };
    fetch(q00 + (tid >> 3), k_pi, k_ci, k_grp, k_w);
    if (tl) {
        // the parameter image of this launch (the caller may have rewritten the state blob since the last one): every lane group
        // stores the parameters of its quads; the trial role waits for all of them before its first step
        auto put = [&](const int4& pi, const int4& ci, const float (&w)[4]) {
            float* img = const_cast<float*>(A.img);
            if (pi.x >= 0 && ci.x >= 0) vjf_st_wt(img + ci.x, w[0]);
            if (pi.y >= 0 && ci.y >= 0) vjf_st_wt(img + ci.y, w[1]);
            if (pi.z >= 0 && ci.z >= 0) vjf_st_wt(img + ci.z, w[2]);
            if (pi.w >= 0 && ci.w >= 0) vjf_st_wt(img + ci.w, w[3]);
        };
        put(k_pi, k_ci, k_w);
        for (int q0 = q00 + qstride; q0 < nquad; q0 += qstride) {
            int4 pi, ci; int grp; float w[4];
            fetch(q0 + (tid >> 3), pi, ci, grp, w);
            put(pi, ci, w);
        }
        vjf_wg_signal_wt(A.cnt + MG_C_IMG, tid);
    }
    if (sw >= n_live) return;                          // (no gradient steps in this launch: one workgroup sums the losses and keeps the scalars)
    unsigned nredo = 0;
    // The scalars this role's first lane keeps -- the likelihood's log-variance and its sample count; in warm-up the state noise and its
    // count -- are its own stores of the step before: read ONCE, kept in registers (a load per step was a chain of two to four
    // memory round trips, 2-4 us, on the path of every gated step: the gate waits for this workgroup too)
    float k_rho = 0.f, k_nlik = 0.f, k_sig = 0.f, k_ntr = 0.f;
    if (sw == 0 && tid == 0) {
        k_rho = vjf_ld_sc1(S + P.off[VJF_SLOT_LIK_LOGVAR]); k_nlik = vjf_ld_sc1(SC + VJF_SC_N_LIK);
        if (do_upd && warm) { k_sig = vjf_ld_sc1(S + P.off[VJF_SLOT_TR_LOGVAR]); k_ntr = vjf_ld_sc1(SC + VJF_SC_N_TR); }
    }
    for (int t = 0; t < A.T; ++t) {
      float l_recon = 0.f, l_dyn = 0.f, ent = 0.f;
      bool ok_r = true, ok_d = true, ok_h = true, grad_ok = true;
      // pass 0: the step.  A loss with a non-finite component (not all three: then the gradient is zero, model.py:206-214) leaves
      // the parameters alone and publishes which components the trial role is to drop; pass 1 steps on its replayed late slabs
      for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0) {
            if (!vjf_wg_wait_sc1<RLS ? VJF_POLL_SLEEP : VJF_POLL_SLEEP_LITE>(A.cnt + MG_C_BWD, (unsigned)(t + 1) * (unsigned)A.n_trial, tid, SC + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u))
                vjf_status_or(SC + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_RESIDENT);
        } else {
            ++nredo;
            if (!vjf_wg_wait_sc1<RLS ? VJF_POLL_SLEEP : VJF_POLL_SLEEP_LITE>(A.cnt + MG_C_REDO_B, nredo * (unsigned)A.n_trial, tid, SC + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u))
                vjf_status_or(SC + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_RESIDENT);
            grad_ok = true;
        }
        if (vjf_abort_wg()) return;                                            // (behind one of the two waits above)
        { const int wg = sw; VJF_MG_STAMP(16); }
        bool have_sums = pass == 1;
        // loss sums of the step: fp64, 32 strided partial sums per scalar, then a fixed xor tree (every SGD workgroup, for the guards)
        auto take_sums = [&]() {
            mg_sum_losses(A, t, s_sc, tid, Bf, P.dz, do_upd && warm);
            // (restates vjf_loss_verdict, and below its partial / dropped / status and vjf_put_loss4, vjf_step_math.h: through the
            //  struct vjf_mega_kernel's lane-spill count rises from 4346 to 5087, profiles/step_math_isa.txt)
            l_recon = s_sc[RS_LRECON] * invB; l_dyn = s_sc[RS_LDYN] * invB; ent = s_sc[RS_ENT] * invB;
            ok_r = isfinite(l_recon); ok_d = isfinite(l_dyn); ok_h = isfinite(ent);
            grad_ok = ok_r && ok_h && (warm || ok_d);
            have_sums = true;
        };
        // one round: the quads q0 + (tid >> 3).  (Uniform over the workgroup: the first round of a pass holds a barrier.)
        auto round = [&](int q0, const int4& pi, const int4& ci, int grp, float (&wold)[4]) {
            const int quad = q0 + (tid >> 3);
            const bool act = quad < nquad;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 tq[16];
            const int src = (act ? quad : 0) * 4;                                  // (float index into the late slabs)
#pragma unroll
            for (int q = 0; q < 16; ++q)
                tq[q] = (act && part * npq + q < w1) ? vjf_ld4_sc1(r_late, src + (part * npq + q) * A.late_len) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (!have_sums) take_sums();
            for (int wq = part * npq + 16; wq < w1; wq += 16) {                   // (more than 128 trial workgroups: further rounds)
#pragma unroll
                for (int q = 0; q < 16; ++q) { v.x += tq[q].x; v.y += tq[q].y; v.z += tq[q].z; v.w += tq[q].w; }
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    tq[q] = (act && wq + q < w1) ? vjf_ld4_sc1(r_late, src + (wq + q) * A.late_len) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) { v.x += tq[q].x; v.y += tq[q].y; v.z += tq[q].z; v.w += tq[q].w; }
            float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                vv[r] += __shfl_xor(vv[r], 1, 64);
                vv[r] += __shfl_xor(vv[r], 2, 64);
                vv[r] += __shfl_xor(vv[r], 4, 64);
            }
            if (!act || part != 0 || (grp == 1 && freeze)) return;                 // (frozen decoder)
            const int pidx[4] = {pi.x, pi.y, pi.z, pi.w}, cidx[4] = {ci.x, ci.y, ci.z, ci.w};
            float* cdst = tl ? const_cast<float*>(A.img) : A.aux;
            // the state blob itself: nobody reads these parameters from it during the launch when the trial role has the image and
            // this lane group keeps them in registers -- then it is brought up to date at the last step only
            const bool wst = !tl || q0 != q00 || t == A.T - 1;
            if (!grad_ok) {
                // no step (model.py:206-214 skips optimizer.step() for this step alone): the steps before it, which this lane group
                // has kept in registers, still have to reach the blob when this is the last step of the launch
                if (tl && q0 == q00 && t == A.T - 1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (pidx[r] >= 0) vjf_st_wt(S + P.train_off + pidx[r], wold[r]);
                }
                return;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (pidx[r] < 0) continue;                                     // (padding of the slab's rows)
                const float wn = vjf_sgd_step(wold[r], vv[r], invB, grp == 1 ? lr_dec : lr_rec);
                wold[r] = wn;
                if (wst) vjf_st_wt(S + P.train_off + pidx[r], wn);
                if (cidx[r] >= 0) vjf_st_wt(cdst + cidx[r], wn);
            }
        };
        if (!do_sgd) take_sums();
        else
        for (int q0 = q00; q0 < nquad || q0 == q00; q0 += qstride) {
            int4 pi = k_pi, ci = k_ci; int grp = k_grp;
            float w[4] = {k_w[0], k_w[1], k_w[2], k_w[3]};
            if (q0 != q00) fetch(q0 + (tid >> 3), pi, ci, grp, w);
            round(q0, pi, ci, grp, w);
            if (q0 == q00) { k_w[0] = w[0]; k_w[1] = w[1]; k_w[2] = w[2]; k_w[3] = w[3]; }
        }
        if (pass == 0 && t == 0 && mode_rls && vjf_ld_sc1(SC + VJF_SC_TRI_CLEAN) == 0.f) {
            // one-time clearing of the halves the inverse loops never write (block-lower part of w_chol, block-upper part of
            // w_pchol): every reader of the dense w_chol of step 0 has signalled its late slab
            float* Wc = S + P.off[VJF_SLOT_W_CHOL];
            float* Lm = S + P.off[VJF_SLOT_W_PCHOL];
            const int n = P.n;
            for (int e = sw * NT + tid; e < n * n; e += n_live * NT) {
                const int i = e / n, j = e - i * n;
                if ((i >> 5) < (j >> 5)) vjf_st_wt(Lm + e, 0.f);
                if ((i >> 5) > (j >> 5)) { vjf_st_wt(Wc + e, 0.f); vjf_st_wt(const_cast<float*>(A.xt) + (size_t)j * n + i, 0.f); }   // (and its row-major transpose)
            }
        }
        const unsigned bad = (ok_r ? 0u : 1u) | (ok_d ? 0u : 2u) | (ok_h ? 0u : 4u);
        // some, not all, of the components IN the loss are non-finite: the reference steps along the gradient of the others
        const bool redo = pass == 0 && do_sgd && !grad_ok && (ok_r || ok_h || (!warm && ok_d));
        if (pass == 0 && sw == 0 && tid == 0) {                                // ---- scalars: loss, likelihood log-variance
            if (redo) __hip_atomic_store(A.cnt + MG_C_MASK, ((unsigned)(t + 1) << 8) | bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!ok_r) l_recon = 0.f;
            if (!ok_d) l_dyn = 0.f;
            if (!ok_h) ent = 0.f;
            const float loss = warm ? l_recon - ent : l_recon - ent + l_dyn;
            if (A.loss) { float* l4 = A.loss + 4 * (size_t)t; l4[0] = loss; l4[1] = -l_recon; l4[2] = -l_dyn; l4[3] = ent; }
            const unsigned st = (ok_r ? 0u : VJF_STATUS_NONFINITE_RECON) | (ok_d ? 0u : VJF_STATUS_NONFINITE_DYN) |
                                (ok_h ? 0u : VJF_STATUS_NONFINITE_ENT);
            if (st) vjf_status_or(SC + VJF_SC_STATUS, st);
            if (P.lik == VJF_LIK_GAUSSIAN) {
                const float sse_y = s_sc[RS_SSEY];
                float rho = k_rho;
                if (do_sgd && ok_r) {                                          // (its gradient comes from the reconstruction term alone)
                    const float g = vjf_rho_grad(P.dy, rho, sse_y, invB);
                    rho -= SC[VJF_SC_LR_LIK] * g;
                }
                if (do_upd) {
                    const float mse = sse_y / (Bf * (float)P.dy);
                    rho = vjf_running_logvar(rho, k_nlik, VJF_LIK_VAR_CAP, Bf, mse, k_nlik);
                    vjf_st_wt(SC + VJF_SC_N_LIK, k_nlik);
                }
                k_rho = rho;
                if (do_sgd || do_upd) vjf_st_wt(S + P.off[VJF_SLOT_LIK_LOGVAR], rho);
            }
            if (do_upd && warm) {
                // warm-up: no RLS update, the state-noise running variance from the residual with the launch's W
                k_sig = vjf_running_logvar(k_sig, k_ntr, VJF_TR_VAR_CAP, Bf, s_sc[RS_RESID], k_ntr);
                vjf_st_wt(S + P.off[VJF_SLOT_TR_LOGVAR], k_sig);
                vjf_st_wt(SC + VJF_SC_N_TR, k_ntr);
            }
        }
        __syncthreads();
        vjf_wg_signal_wt(A.cnt + (pass == 0 ? MG_C_SGD : MG_C_REDO_S), tid);
        { const int wg = sw; VJF_MG_STAMP(17); }
        if (!redo) break;
      }
    }
    // (the launch's last act on the triangle flag: set once every SGD workgroup has cleared its share -- they all have signalled
    //  step 0 by then; the kernel boundary makes it visible to the next launch)
    if (sw == 0 && tid == 0 && mode_rls && SC[VJF_SC_TRI_CLEAN] == 0.f) {
        if (vjf_poll_count<2>(A.cnt + MG_C_SGD, (unsigned)n_live, nullptr)) vjf_st_wt(SC + VJF_SC_TRI_CLEAN, 1.f);
    }
}

// The parameter image of a launch without parameter updates (nothing else for an SGD role to do there): builder `sw` of `nb`
// stores the parameters of its quads of the slab tables at their places in the image (what vjf_mega_sgd does at the start of the
// other launches), then counts itself in at MG_C_IMG.
__device__ __forceinline__ void mg_build_image(const VjfPlan& P, const VjfMegaArgs& A, const int sw, const int nb) {
    constexpr int NT = VJF_MG_THREADS;
    const int tid = threadIdx.x, part = tid & 7;
    if (vjf_mega_trial_lds<false>(P, A.lds_floats).theta == 0) return;    // (the trial role reads the state itself)
    const int nquad = A.slab_len >> 2, qstride = (nb * NT) >> 3;
    const float* th = A.state + P.train_off;
    float* img = const_cast<float*>(A.img);
    for (int q0 = (sw * NT) >> 3; q0 < nquad; q0 += qstride) {
        const int quad = q0 + (tid >> 3);
        if (quad < nquad && part == 0) {
            const int4 pi = *reinterpret_cast<const int4*>(A.sl_pidx + (size_t)quad * 4);
            const int4 ci = *reinterpret_cast<const int4*>(A.sl_cidx + (size_t)quad * 4);
            if (pi.x >= 0 && ci.x >= 0) vjf_st_wt(img + ci.x, th[pi.x]);
            if (pi.y >= 0 && ci.y >= 0) vjf_st_wt(img + ci.y, th[pi.y]);
            if (pi.z >= 0 && ci.z >= 0) vjf_st_wt(img + ci.z, th[pi.z]);
            if (pi.w >= 0 && ci.w >= 0) vjf_st_wt(img + ci.w, th[pi.w]);
        }
    }
    vjf_wg_signal_wt(A.cnt + MG_C_IMG, tid);
}
