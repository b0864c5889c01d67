// vjf_rls_operands.h -- the many-workgroup kernels in front of the once-per-step serial half (n_rbf <= 224).
//
//   vjf_prep_kernel  (many workgroups): everything element-wise that the step's serial half
//       needs -- finite guards + loss, clip + SGD, likelihood running variance
//       (vjf_step_math.h), g = P W + Phi^T dx / v and
//       P += Phi^T Phi / v (module.py:94-96) -- so that ONE compute unit is left with nothing
//       but the dependent chain (vjf_chol_kernel.h).
//   vjf_prepg_kernel (ceil(n / 16) workgroups): the RLS operands g and P alone, on the matrix cores.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_gram_kernel.h"   // vjf_f32x4
#include "vjf_handoff.h"
#include "vjf_plan.h"
#include "vjf_step_math.h"

#define VJF_PREP_ROWS 1                   // rows of P per prep workgroup

// ---------------------------------------------------------------------------------------------
struct VjfPrepArgs {
    float* state;
    const float* red;
    float* gbuf;          // (n, dz) g = P W + FDX / v
    float* aux;           // transposed weight copies, kept in step with the SGD update
    float* loss4;
    int B_total;
    unsigned flags;
    int n_rowblk, n_sgdblk;
    const unsigned* wait_count;   // vjf_prepg_kernel: non-null -> W, sigma come from a kernel on another stream: wait (bounded)
    unsigned wait_target;         //   until *wait_count has reached wait_target, then acquire at agent scope
    int bid0;             // first logical workgroup of this launch: 0 (whole grid, or the RLS-operand rows only)
                          // or n_rowblk (SGD + scalars only) -- the two halves run on different streams in vjf_filter_seq
    // scalar workgroup, vjf_filter_seq only: it ends only when this step's Cholesky kernel (run_word >= run_epoch) and all of its
    // post kernel's workgroups (*start_count >= start_target) are RESIDENT.  The next backward half of the trial kernel waits
    // in-kernel for their results: it must not take the CUs they need before they are placed.
    const unsigned* run_word; unsigned run_epoch;
    const unsigned* start_count; unsigned start_target;
    unsigned* done_count;         // vjf_prepg_kernel: non-null -> += 1 per workgroup once its rows of P and g are in memory
    // Non-finite loss component (vjf/model.py:138-149) on the one-stream route: the first pass leaves the parameters alone and
    // writes the dropped components (bit 0 recon, 1 dynamics, 2 entropy; 0: nothing to replay) and the likelihood log-variance the
    // step started with; the backward half and the gradient sums run again behind it (they return at once on 0), then the second
    // pass (replay_pass) applies the step from the new sums.
    unsigned* replay_mask; float* replay_rho; int replay_pass;
};

// logical grid = n_rowblk + n_sgdblk + 1
__global__ __launch_bounds__(256) void vjf_prep_kernel(VjfPlan P, VjfPrepArgs A) {
    const int tid = threadIdx.x, bid = blockIdx.x + A.bid0;
    float* S = A.state;
    float* SC = S + P.off[VJF_SLOT_SCALARS];
    const float* RSC = A.red + P.red_SCA;                      // the loss sums (RS_LRECON .. RS_SSEY)
    const bool do_sgd = A.flags & VJF_FLAG_SGD, do_upd = A.flags & VJF_FLAG_UPDATE, warm = A.flags & VJF_FLAG_WARM_UP;
    const float Bf = (float)A.B_total, invB = 1.0f / Bf;
    const VjfLossVerdict v = vjf_loss_verdict(RSC[RS_LRECON], RSC[RS_LDYN], RSC[RS_ENT], invB, warm);
    const bool grad_ok = v.grad_ok();
    const bool replay = A.replay_mask != nullptr && v.partial(do_sgd);

    if (bid < A.n_rowblk) {                                    // ---- RLS operands: one row of P per workgroup
        if (!do_upd || warm) return;
        __shared__ float s_part[4 * 32];
        const int n = P.n, dz = P.dz, i = bid;
        const float inv_v = expf(-S[P.off[VJF_SLOT_TR_LOGVAR]]);
        const float lam = vjf_shrink_of(SC[VJF_SC_SHRINK]);
        float* Pm = S + P.off[VJF_SLOT_W_PREC];
        const float* Wm = S + P.off[VJF_SLOT_W_MEAN];
        const float* G = A.red + P.red_G;
        const float* FDX = A.red + P.red_FDX;
        // g[i][:] = sum_k lambda P[i][k] W[k][:] : thread k (n <= 224 < 256 on this path) holds one term per output,
        // then wave + workgroup reduction
        const int k = tid;
        float p = 0.f;
        if (k < n) {
            p = vjf_lam_mul(Pm[(size_t)i * n + k], lam);                   // lambda P: of the update and of g = (lambda P) W
            Pm[(size_t)i * n + k] = p + G[(size_t)i * n + k] * inv_v;      // P = lambda P + Phi^T Phi / v (module.py:96)
        }
        for (int j = 0; j < dz; ++j) {
            float v = (k < n) ? p * Wm[(size_t)k * dz + j] : 0.f;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if ((tid & 63) == 0) s_part[(tid >> 6) * 32 + j] = v;
        }
        __syncthreads();
        if (tid < dz) A.gbuf[(size_t)i * dz + tid] = ((s_part[tid] + s_part[32 + tid]) + s_part[64 + tid]) + s_part[96 + tid] + FDX[(size_t)i * dz + tid] * inv_v;
        return;
    }
    if (bid < A.n_rowblk + A.n_sgdblk) {                       // ---- clip + SGD, tensor by tensor; transposed copies follow
        if (A.replay_pass) { if (__hip_atomic_load(A.replay_mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return; }
        else if (!(do_sgd && grad_ok)) return;
        const float lr_dec = SC[VJF_SC_LR_DEC], lr_rec = SC[VJF_SC_LR_REC];
        const bool freeze = SC[VJF_SC_FREEZE_DEC] != 0.f;
        const int g0 = (bid - A.n_rowblk) * 256 + tid, gs = A.n_sgdblk * 256;
        for (int t = 0; t < P.n_train; ++t) {
            if (P.tr_dec[t] && freeze) continue;
            const float lr = P.tr_dec[t] ? lr_dec : lr_rec;
            const int rows = P.tr_rows[t], cols = P.tr_cols[t], off = P.tr_off[t];
            for (int e = g0; e < rows * cols; e += gs) {
                const float w = vjf_sgd_step(S[off + e], A.red[off - P.train_off + e], invB, lr);
                S[off + e] = w;
                if (P.tr_aux[t] >= 0) {
                    const int r = e / cols, c = e - r * cols;
                    A.aux[P.tr_aux[t] + (size_t)c * P.tr_auxld[t] + P.tr_auxcol[t] + r] = w;
                }
            }
        }
        return;
    }
    if (A.replay_pass) return;                                 // (the scalars were settled by the first pass)
    if (tid == 0) {                                            // ---- scalars: loss, likelihood log-variance
        if (A.replay_mask) {
            vjf_st_wt(A.replay_rho, S[P.off[VJF_SLOT_LIK_LOGVAR]]);
            vjf_st_wt(A.replay_mask, replay ? v.dropped() : 0u);
        }
        if (A.loss4) vjf_put_loss4(A.loss4, v);
        if (v.status()) vjf_status_or(SC + VJF_SC_STATUS, v.status());
        if (P.lik == VJF_LIK_GAUSSIAN) {
            const float sse_y = RSC[RS_SSEY];
            float rho = S[P.off[VJF_SLOT_LIK_LOGVAR]];
            if (do_sgd && (grad_ok || (replay && v.ok_r))) rho -= SC[VJF_SC_LR_LIK] * vjf_rho_grad(P.dy, rho, sse_y, invB);
            if (do_upd) {
                const float mse = sse_y / (Bf * (float)P.dy);
                float tot;
                rho = vjf_running_logvar(rho, SC[VJF_SC_N_LIK], VJF_LIK_VAR_CAP, Bf, mse, tot);
                SC[VJF_SC_N_LIK] = tot;
            }
            S[P.off[VJF_SLOT_LIK_LOGVAR]] = rho;
        }
        if (A.run_word) {
            bool there = false;
            for (unsigned spins = 0; spins < VJF_WAIT_SPINS; ++spins) {      // (its own loop, not vjf_poll_count: two words, both there at the same look)
                const unsigned r = __hip_atomic_load(A.run_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned q = __hip_atomic_load(A.start_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((int)(r - A.run_epoch) >= 0 && (int)(q - A.start_target) >= 0) { there = true; break; }
                if ((spins & 255u) == 255u && vjf_abort_seen(SC + VJF_SC_STATUS)) break;
                __builtin_amdgcn_s_sleep(2);
            }
            if (!there) vjf_status_or(SC + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_RESIDENT);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// RLS operands, 16 rows of P per workgroup (replaces the row part of vjf_prep_kernel on the fast path):
//   g[i][:] = sum_k lambda P[i][k] W[k][:] + (Phi^T dx)[i][:] / v   (module.py:94)   on v_mfma_f32_16x16x4_f32, K split over 4 wavefronts
//   P[i][:] = lambda P[i][:] + (Phi^T Phi)[i][:] / v                 (module.py:96)   on the rows just read
// (lambda: the forgetting factor, VJF_SC_SHRINK; the rows are scaled once, as they arrive)
// grid = ceil(n / 16) workgroups of 256 threads; n % 4 == 0.
#define VJF_PREPG_LDP(n) ((n) + 4)
static inline size_t vjf_prepg_lds_bytes(const VjfPlan& P) { return ((size_t)16 * VJF_PREPG_LDP(P.n) + (size_t)P.n * 17 + 4 * 16 * 17) * 4; }

__global__ __launch_bounds__(256) void vjf_prepg_kernel(VjfPlan P, VjfPrepArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const unsigned do_upd = A.flags & VJF_FLAG_UPDATE, warm = A.flags & VJF_FLAG_WARM_UP;
    if (!do_upd || warm) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = P.n, dz = P.dz, i0 = blockIdx.x * 16, ldp = VJF_PREPG_LDP(n);
    float* s_p = lds;                                  // [16][n + 4]  rows of lambda P (P before the update)
    float* s_w = s_p + 16 * ldp;                       // [n][17]      W, columns dz..15 zero
    float* s_r = s_w + (size_t)n * 17;                 // [4][16][17]  per-wavefront partial products
    float* S = A.state;
    if (A.wait_count) {
        if (tid == 0) {
            const bool there = vjf_poll_count<4>(A.wait_count, A.wait_target, nullptr);
            if (!there) vjf_status_or(S + P.off[VJF_SLOT_SCALARS] + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_OPERAND);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
    }
    // (a vector load that bypasses L1 / the scalar cache: sigma may have been written while this kernel was already waiting)
    const float inv_v = expf(-__hip_atomic_load(S + P.off[VJF_SLOT_TR_LOGVAR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const float lam = vjf_shrink_of(S[P.off[VJF_SLOT_SCALARS] + VJF_SC_SHRINK]);
    float* Pm = S + P.off[VJF_SLOT_W_PREC];
    const float* Wm = S + P.off[VJF_SLOT_W_MEAN];
    const float* G = A.red + P.red_G;
    const float* FDX = A.red + P.red_FDX;
    const int n4 = n >> 2;
    for (int e0 = tid; e0 < 16 * n4; e0 += 4 * 256) {  // 4 float4 of P and of G in flight per thread
        float4 p[4], g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = e0 + q * 256, row = e / n4, c4 = (e - row * n4) * 4;
            const bool in = e < 16 * n4 && i0 + row < n;
            const size_t off = in ? (size_t)(i0 + row) * n + c4 : 0;
            p[q] = *reinterpret_cast<const float4*>(Pm + off);
            g[q] = *reinterpret_cast<const float4*>(G + off);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            p[q].x = vjf_lam_mul(p[q].x, lam); p[q].y = vjf_lam_mul(p[q].y, lam);
            p[q].z = vjf_lam_mul(p[q].z, lam); p[q].w = vjf_lam_mul(p[q].w, lam);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = e0 + q * 256, row = e / n4, c4 = (e - row * n4) * 4;
            if (e >= 16 * n4) continue;
            const bool in = i0 + row < n;
            float* d = s_p + row * ldp + c4;
            d[0] = in ? p[q].x : 0.f; d[1] = in ? p[q].y : 0.f; d[2] = in ? p[q].z : 0.f; d[3] = in ? p[q].w : 0.f;
            if (in) {
                float4 o;
                o.x = fmaf(g[q].x, inv_v, p[q].x); o.y = fmaf(g[q].y, inv_v, p[q].y); o.z = fmaf(g[q].z, inv_v, p[q].z); o.w = fmaf(g[q].w, inv_v, p[q].w);
                float* dstp = Pm + (size_t)(i0 + row) * n + c4;
                if (A.done_count) { vjf_st_wt(dstp, o.x); vjf_st_wt(dstp + 1, o.y); vjf_st_wt(dstp + 2, o.z); vjf_st_wt(dstp + 3, o.w); }
                else *reinterpret_cast<float4*>(dstp) = o;
            }
        }
    }
    for (int e = tid; e < n * 16; e += 256) {
        const int k = e >> 4, c = e & 15;
        s_w[k * 17 + c] = c < dz ? Wm[(size_t)k * dz + c] : 0.f;
    }
    __syncthreads();
    {
        const int i = lane & 15, kk = lane >> 4;
        vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int s4 = wave; s4 < n4; s4 += 4) {        // k-step s4 covers k = 4 s4 .. 4 s4 + 3
            const float a = s_p[i * ldp + 4 * s4 + kk];
            const float b = s_w[(4 * s4 + kk) * 17 + i];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) s_r[(wave * 16 + 4 * (lane >> 4) + r) * 17 + (lane & 15)] = acc[r];   // row 4(lane>>4)+r, column lane&15
    }
    __syncthreads();
    for (int e = tid; e < 16 * 16; e += 256) {
        const int r = e >> 4, c = e & 15;
        if (c < dz && i0 + r < n) {
            const float v = ((s_r[r * 17 + c] + s_r[(16 + r) * 17 + c]) + s_r[(32 + r) * 17 + c]) + s_r[(48 + r) * 17 + c];
            const float gv = v + FDX[(size_t)(i0 + r) * dz + c] * inv_v;
            if (A.done_count) vjf_st_wt(A.gbuf + (size_t)(i0 + r) * dz + c, gv); else A.gbuf[(size_t)(i0 + r) * dz + c] = gv;
        }
    }
    if (A.done_count) vjf_wg_signal_wt(A.done_count, tid);
}
