// vjf_mega_prep.h -- the operand role of the one-launch route (vjf_mega_kernel.h).
#pragma once
#include "vjf_mega_common.h"

// ------------------------------------------------------------------------------------------------ operand role
// g = lambda P W + Phi^T dx / v and P = lambda P + Phi^T Phi / v for 16 rows (module.py:94-96); Phi^T dx = sum of the trial workgroups' early slabs
__device__ __forceinline__ void vjf_mega_prep(const VjfPlan& P, const VjfMegaArgs& A, float* lds, const int pw) {
    constexpr int NT = VJF_MG_THREADS, NW = VJF_MG_WAVES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = P.n, dz = P.dz, i0 = pw * 16, ldp = VJF_PREPG_LDP(n);
    float* s_p = lds;                                  // [16][n + 4]  rows of lambda P (P before the update)
    float* s_w = s_p + 16 * ldp;                       // [n][17]      W, columns dz..15 zero
    float* s_r = s_w + (size_t)n * 17;                 // [NW][16][17] per-wavefront partial products
    float* s_f = s_r + NW * 16 * 17;                   // [16][17]     Phi^T dx rows
    float* S = A.state;
    float* SCW = S + P.off[VJF_SLOT_SCALARS];
    const unsigned npost = (unsigned)(A.n_rls - 1);
    const unsigned* runw = A.cnt + MG_C_COLFLAGS + VJF_CHOL_MAXBLK + 2;
    // (every byte taken from other roles is read with sc1 loads behind the counts' polls and the workgroup barrier: no acquires)
    const __amdgpu_buffer_rsrc_t r_early = vjf_rsrc(A.slab_early);
    for (int t = 0; t < A.T; ++t) {
        float* red = (t & 1) ? A.red1 : A.red0;
        // (four counts, ONE acquire: behind the last of them)
        bool ok = vjf_wg_wait_sc1(A.cnt + MG_C_FWD, (unsigned)(t + 1) * (unsigned)A.n_trial, tid, SCW + VJF_SC_STATUS);
        ok = vjf_wg_wait_sc1(A.cnt + MG_C_STAT, (unsigned)(t + 1) * (unsigned)A.n_gram, tid, SCW + VJF_SC_STATUS) && ok;
        if (t > 0) ok = vjf_wg_wait_sc1(A.cnt + MG_C_PDONE, (unsigned)t * npost, tid, SCW + VJF_SC_STATUS) && ok;
        ok = vjf_wg_wait_sc1(runw, (unsigned)(t + 1), tid, SCW + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u) && ok;      // the Cholesky loop holds its operands (it reads the state's P at step 0)
        if (tid == 0 && !ok) { vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_OPERAND); vjf_s_abort_word = 1; }
        __syncthreads();                                                       // (the verdict of lane 0, for every thread alike)
        if (vjf_abort_wg()) return;
        { const int wg = pw; VJF_MG_STAMP(14); }
        // Phi^T dx rows i0 .. i0 + 15 (16 columns x 4 quads of features: the early slabs hold it transposed): 8 lanes per quad, lane p
        // sums the early slabs [p npq, (p+1) npq) (all in flight), then a fixed xor tree
        {
            const int ldn = (n + 3) & ~3;
            const float* base = A.slab_early + (size_t)(t & 1) * A.n_trial * A.early_len;
            const int npq = (A.n_trial + 7) >> 3, part = tid & 7, quad = tid >> 3;      // quad = column * 4 + feature quad
            const int c = quad >> 2, r4 = (quad & 3) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < dz && i0 + r4 < ldn) {
                const int src = (int)(base - A.slab_early) + c * ldn + i0 + r4;
                const int w1 = min(A.n_trial, (part + 1) * npq);
                for (int w0 = part * npq; w0 < w1; w0 += 16) {
                    float4 tq[16];
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        tq[q] = (w0 + q < w1) ? vjf_ld4_sc1(r_early, src + (w0 + q) * A.early_len) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int q = 0; q < 16; ++q) { v.x += tq[q].x; v.y += tq[q].y; v.z += tq[q].z; v.w += tq[q].w; }
                }
            }
            float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                vv[q] += __shfl_xor(vv[q], 1, 64);
                vv[q] += __shfl_xor(vv[q], 2, 64);
                vv[q] += __shfl_xor(vv[q], 4, 64);
            }
            if (part == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    s_f[(r4 + q) * 17 + c] = vv[q];
                    if (i0 + r4 + q < n && c < dz) vjf_st_wt(red + P.red_FDX + (size_t)(i0 + r4 + q) * dz + c, vv[q]);
                }
            }
            if (pw == 0 && tid < 64) {                                             // sum |dx|^2: one wavefront, strided partial sums, xor tree
                float q2 = 0.f;
                for (int w = tid; w < A.n_trial; w += 64) q2 += vjf_ld_sc1(base + (size_t)w * A.early_len + (size_t)16 * ldn + RS_SDX2);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) q2 += __shfl_xor(q2, o, 64);
                if (tid == 0) vjf_st_wt(red + P.red_SC + RS_SDX2, q2);
            }
        }
        const float inv_v = expf(-vjf_ld_sc1(S + P.off[VJF_SLOT_TR_LOGVAR]));
        const float lam = vjf_shrink_of(vjf_ld_sc1(SCW + VJF_SC_SHRINK));
        float* Pm = S + P.off[VJF_SLOT_W_PREC];
        const float* Wm = S + P.off[VJF_SLOT_W_MEAN];
        const float* G = red + P.red_G;
        const __amdgpu_buffer_rsrc_t r_P = vjf_rsrc(Pm), r_G = vjf_rsrc(G);
        const int n4 = n >> 2;
        const unsigned m_n4 = mg_magic(n4);
        for (int e0 = tid; e0 < 16 * n4; e0 += 4 * NT) {
            float4 p[4], g[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = e0 + q * NT, row = mg_div(e, m_n4), c4 = (e - row * n4) * 4;
                const bool in = e < 16 * n4 && i0 + row < n;
                const size_t off = in ? (size_t)(i0 + row) * n + c4 : 0;
                p[q] = vjf_ld4_sc1(r_P, (int)off);                                  // (P: this workgroup's own rows -- and the y / W loop's after a failed factorisation)
                g[q] = vjf_ld4_sc1(r_G, (int)off);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {                                      // lambda P: what the update adds to, and the P of g = (lambda P) W
                p[q].x = vjf_lam_mul(p[q].x, lam); p[q].y = vjf_lam_mul(p[q].y, lam);
                p[q].z = vjf_lam_mul(p[q].z, lam); p[q].w = vjf_lam_mul(p[q].w, lam);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = e0 + q * NT, row = mg_div(e, m_n4), c4 = (e - row * n4) * 4;
                if (e >= 16 * n4) continue;
                const bool in = i0 + row < n;
                float* d = s_p + row * ldp + c4;
                d[0] = in ? p[q].x : 0.f; d[1] = in ? p[q].y : 0.f; d[2] = in ? p[q].z : 0.f; d[3] = in ? p[q].w : 0.f;
                if (in) vjf_st4_wt(Pm + (size_t)(i0 + row) * n + c4, fmaf(g[q].x, inv_v, p[q].x), fmaf(g[q].y, inv_v, p[q].y),
                               fmaf(g[q].z, inv_v, p[q].z), fmaf(g[q].w, inv_v, p[q].w));
            }
        }
        for (int e = tid; e < n * 16; e += NT) {
            const int k = e >> 4, cc = e & 15;
            s_w[k * 17 + cc] = cc < dz ? vjf_ld_sc1(Wm + (size_t)k * dz + cc) : 0.f;
        }
        __syncthreads();
        {
            const int i = lane & 15, kk = lane >> 4;
            vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int s4 = wave; s4 < n4; s4 += NW) {       // k-step s4 covers k = 4 s4 .. 4 s4 + 3
                const float a = s_p[i * ldp + 4 * s4 + kk];
                const float b = s_w[(4 * s4 + kk) * 17 + i];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) s_r[(wave * 16 + 4 * (lane >> 4) + r) * 17 + (lane & 15)] = acc[r];
        }
        __syncthreads();
        if (tid < 256) {
            const int r = tid >> 4, cc = tid & 15;
            if (cc < dz && i0 + r < n) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) v += s_r[(w * 16 + r) * 17 + cc];
                vjf_st_wt(A.gbuf + (size_t)(i0 + r) * dz + cc, v + s_f[r * 17 + cc] * inv_v);
            }
        }
        vjf_wg_signal_wt(A.cnt + MG_C_PREP, tid);
        { const int wg = pw; VJF_MG_STAMP(15); }
    }
}
