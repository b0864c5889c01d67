// vjf_mega_gram.h -- the Gram role of the one-launch route (vjf_mega_kernel.h).
#pragma once
#include "vjf_mega_common.h"

// ------------------------------------------------------------------------------------------------ Gram role
// Phi^T Phi of event e (the features of step e), lower 32x32 tiles.  The rows of Phi are formed here, from the posterior of step
// e - 1 and the noise of step e -- operation for operation what the trial role does for its own tile (stages 0 / 1), so the two
// hold the same bits -- as soon as every trial workgroup has its forward pass of step e - 1 behind it: a step AHEAD of the RLS
// update that consumes the sum.
__device__ __forceinline__ void vjf_mega_gram(const VjfPlan& P, const VjfMegaArgs& A, float* lds, const int hg) {
    constexpr int NT = VJF_MG_THREADS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = P.n, nbl = (n + 31) / 32, ntri = nbl * (nbl + 1) / 2, ldE = P.ldE;
    const unsigned m_l4 = mg_magic(ldE >> 2);
    float* SCW = A.state + P.off[VJF_SLOT_SCALARS];
    const int dz = P.dz, du = P.du, dxu = P.dxu, npad = (n + 3) & ~3;
    float* s_rows = lds;                               // [VJF_MG_GROWS][ldE]
    int* s_tab = reinterpret_cast<int*>(s_rows + (size_t)VJF_MG_GROWS * ldE);   // tile -> (bi << 8) | bj
    float* s_cen = s_rows + (size_t)VJF_MG_GROWS * ldE + 64;                    // [dxu][npad]
    float* s_iw = s_cen + (size_t)npad * dxu;                                   // [npad]
    float* s_x = s_iw + npad;                                                   // [VJF_MG_GROWS][dxu]
    const float* S = A.state;
    mg_stage_centres(P, S, s_cen, s_iw, tid);
    const size_t sz = (size_t)A.B * dz, su = (size_t)A.B * du;
    const unsigned m_dxu = mg_magic(dxu);
    if (tid < ntri) {
        int bi = 0;
        while ((bi + 1) * (bi + 2) / 2 <= tid) ++bi;
        s_tab[tid] = (bi << 8) | (tid - bi * (bi + 1) / 2);
    }
    __syncthreads();
    const int r0 = hg * A.gram_rows, r1 = min(A.B, r0 + A.gram_rows);
    float* myslab = A.gslab + (size_t)hg * ntri * 1024;
    const __amdgpu_buffer_rsrc_t r_gslab = vjf_rsrc(A.gslab);
    const int c = lane & 31, kh = lane >> 5;
    for (int e = 0; e < A.T; ++e) {
        float* red = (e & 1) ? A.red1 : A.red0;
        const float* mu_s = e ? A.mu + (size_t)(e - 1) * sz : A.mu0;
        const float* lv_s = e ? A.lv + (size_t)(e - 1) * sz : A.lv0;
        const float* eps_s = A.eps + (size_t)e * 2 * sz;
        const float* u_e = A.u ? A.u + (size_t)e * su : nullptr;
        // (the posterior of step e - 1: write-through stores of the trial role, in memory before its early slab's signal)
        // (the slab of the previous event: every Gram workgroup has summed its share -- nothing is read behind this one: no acquire)
        if (e > 0 && !vjf_wg_wait_sc1(A.cnt + MG_C_STAT, (unsigned)e * (unsigned)A.n_gram, tid, SCW + VJF_SC_STATUS))
            vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_GATE2);
        if (e > 0 && !vjf_wg_wait_sc1(A.cnt + MG_C_FWD, (unsigned)e * (unsigned)A.n_trial, tid, SCW + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u))
            vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_GATE2);
        if (e > 0 && vjf_abort_wg()) return;
        { const int wg = hg, t = e; VJF_MG_STAMP(11); }
        vjf_f32x16 acc[VJF_MG_MAXQ];
#pragma unroll
        for (int q = 0; q < VJF_MG_MAXQ; ++q)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
        for (int c0 = r0; c0 < r1; c0 += VJF_MG_GROWS) {
            __syncthreads();
            const int l4 = ldE >> 2;
            const int ks = min(VJF_MG_GROWS / 2, (((min(VJF_MG_GROWS, r1 - c0) + 1) >> 1) + 1) & ~1);   // (a multiple of 2; rows beyond the range are zero)
            // xs = mu + eps e^{lv/2} (model.py:97-99; the prior at the first step of a run: model.py:188-190) and the inputs u
            for (int i = tid; i < VJF_MG_GROWS * dxu; i += NT) {
                const int r = mg_div(i, m_dxu), c2 = i - r * dxu, b = c0 + r;
                float v = 0.f;
                if (b < r1) {
                    if (c2 < dz) {
                        const float m = mu_s ? vjf_ld_sc1(mu_s + (size_t)b * dz + c2) : S[P.off[VJF_SLOT_PRIOR_MEAN] + c2];   // (sc1: no acquire
                        const float l = mu_s ? vjf_ld_sc1(lv_s + (size_t)b * dz + c2) : S[P.off[VJF_SLOT_PRIOR_LOGVAR] + c2]; //  behind the waits)
                        v = fmaf(eps_s[(size_t)b * dz + c2], expf(0.5f * l), m);
                    } else {
                        v = u_e[(size_t)b * du + c2 - dz];
                    }
                }
                s_x[i] = v;
            }
            __syncthreads();
            // RBF features (functional.py:11-22), four centres per thread and pass; rows beyond the range and columns beyond n: zero
            for (int i = tid; i < VJF_MG_GROWS * l4; i += NT) {
                const int r = mg_div(i, m_l4), k = (i - r * l4) * 4;
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c0 + r < r1 && k < npad) {
                    float d2[4] = {0.f, 0.f, 0.f, 0.f};
                    // (the moments role's copy of these lines, vjf_mega_moments.h, ON PURPOSE: see there -- profiles/mega_split_isa.txt, candidate 1)
                    auto dim = [&](float x, const float4& cc) {                     // (one input dimension: the trial role's order of operations)
                        float d;
                        d = x - cc.x; d2[0] = fmaf(d, d, d2[0]); d = x - cc.y; d2[1] = fmaf(d, d, d2[1]);
                        d = x - cc.z; d2[2] = fmaf(d, d, d2[2]); d = x - cc.w; d2[3] = fmaf(d, d, d2[3]);
                    };
                    int c2 = 0;
                    for (; c2 + 3 < dxu; c2 += 4) {                                  // four dimensions' LDS loads in flight together
                        const float x0 = s_x[r * dxu + c2], x1 = s_x[r * dxu + c2 + 1], x2 = s_x[r * dxu + c2 + 2], x3 = s_x[r * dxu + c2 + 3];
                        const float4 c0v = *reinterpret_cast<const float4*>(s_cen + c2 * npad + k);
                        const float4 c1v = *reinterpret_cast<const float4*>(s_cen + (c2 + 1) * npad + k);
                        const float4 c2v = *reinterpret_cast<const float4*>(s_cen + (c2 + 2) * npad + k);
                        const float4 c3v = *reinterpret_cast<const float4*>(s_cen + (c2 + 3) * npad + k);
                        dim(x0, c0v); dim(x1, c1v); dim(x2, c2v); dim(x3, c3v);
                    }
                    for (; c2 < dxu; ++c2) dim(s_x[r * dxu + c2], *reinterpret_cast<const float4*>(s_cen + c2 * npad + k));
                    const float4 iw = *reinterpret_cast<const float4*>(s_iw + k);
                    o.x = expf(d2[0] * iw.x); o.y = k + 1 < n ? expf(d2[1] * iw.y) : 0.f;
                    o.z = k + 2 < n ? expf(d2[2] * iw.z) : 0.f; o.w = k + 3 < n ? expf(d2[3] * iw.w) : 0.f;
                }
                *reinterpret_cast<float4*>(s_rows + (size_t)r * ldE + k) = o;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < VJF_MG_MAXQ; ++q) {
                const int tt = wave + VJF_MG_WAVES * q;
                if (tt < ntri) {
                    const int code = s_tab[tt], bi = code >> 8, bj = code & 255;
                    const float* pa = s_rows + (size_t)kh * ldE + bi * 32 + c;
                    const float* pb = s_rows + (size_t)kh * ldE + bj * 32 + c;
                    int s = 0;
#pragma unroll 2
                    for (; s + 8 <= ks; s += 8) {                                  // ks = k-steps (row pairs) of this pass that hold rows
                        float a[8], b[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) { a[u] = pa[(size_t)(2 * (s + u)) * ldE]; b[u] = pb[(size_t)(2 * (s + u)) * ldE]; }
#pragma unroll
                        for (int u = 0; u < 8; ++u) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc[q], 0, 0, 0);
                    }
                    for (; s < ks; s += 2) {
                        float a[2], b[2];
#pragma unroll
                        for (int u = 0; u < 2; ++u) { a[u] = pa[(size_t)(2 * (s + u)) * ldE]; b[u] = pb[(size_t)(2 * (s + u)) * ldE]; }
#pragma unroll
                        for (int u = 0; u < 2; ++u) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc[q], 0, 0, 0);
                    }
                    // the last pass of rows: the tile is final and leaves at once, 16-byte write-through stores, beside the next tile's
                    // multiply-adds.  Accumulator: column = lane & 31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5); slab element
                    // ((j*64 + lane)*4 + r) = register 4 j + r of that lane
                    if (c0 + VJF_MG_GROWS >= r1) {
                        float* sl = myslab + (size_t)tt * 1024;
#pragma unroll
                        for (int j = 0; j < 4; ++j) vjf_st4_wt(sl + (j * 64 + lane) * 4, acc[q][4 * j], acc[q][4 * j + 1], acc[q][4 * j + 2], acc[q][4 * j + 3]);
                    }
                }
            }
        }
        if (r0 >= r1) {                                                        // (a workgroup without rows: its slab is zeros)
#pragma unroll
            for (int q = 0; q < VJF_MG_MAXQ; ++q) {
                const int tt = wave + VJF_MG_WAVES * q;
                if (tt < ntri) {
                    float* sl = myslab + (size_t)tt * 1024;
#pragma unroll
                    for (int j = 0; j < 4; ++j) vjf_st4_wt(sl + (j * 64 + lane) * 4, 0.f, 0.f, 0.f, 0.f);
                }
            }
        }
        vjf_wg_signal_wt(A.cnt + MG_C_GRAM, tid);
        { const int wg = hg, t = e; VJF_MG_STAMP(12); }
        // The sums of event e go where those of event e - 2 are: the RLS update of step e - 2 must be through with them (the Cholesky
        // loop's operand load, the operand role's P += G / v, the y / W loop's tiles for the state-noise update).  The trial role's
        // forward half of step e - 1, which is all this event waited for, does not wait for that update: without this wait a late
        // RLS role -- the first steps of a process, instruction caches cold -- read sums of the wrong step.  Nothing is read behind it.
#ifndef VJF_CHAOS_OMIT_GRAM_GUARD        /* (diagnostic builds: without the wait tools/chaos_handoffs.py must report deviations) */
        if (e >= 2 && !vjf_wg_wait_sc1(A.cnt + MG_C_PDONE, (unsigned)(e - 1) * (unsigned)(A.n_rls - 1), tid, SCW + VJF_SC_STATUS))
            vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_GATE2);
#endif
        if (!vjf_wg_wait_sc1(A.cnt + MG_C_GRAM, (unsigned)(e + 1) * (unsigned)A.n_gram, tid, SCW + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u))
            vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_GATE2);
        if (vjf_abort_wg()) return;
        // this workgroup's share of the sum over the slabs: a quad of elements per 4 lanes, lane p sums the slabs [p npq, (p+1) npq)
        // (all of them in flight -- for TWO quads at a time: one round trip for the whole share at config B), then
        // (s0 + s1) + (s2 + s3): a fixed order
        {
            const int npq = (A.n_gram + 3) >> 2;
            const int part = tid & 3;
            const int qstride = (A.n_gram * NT) >> 2, nq = ntri * 256;
            const int h1 = min(A.n_gram, (part + 1) * npq);
            auto load16 = [&](float4 (&tq)[16], int quad, int h0) {
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    tq[q] = (quad < nq && h0 + q < h1) ? vjf_ld4_sc1(r_gslab, quad * 4 + (h0 + q) * ntri * 1024) : make_float4(0.f, 0.f, 0.f, 0.f);
            };
            auto add16 = [&](float4& v, const float4 (&tq)[16]) {
#pragma unroll
                for (int q = 0; q < 16; ++q) { v.x += tq[q].x; v.y += tq[q].y; v.z += tq[q].z; v.w += tq[q].w; }
            };
            auto finish = [&](int quad, float4 v) {
                float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    vv[r] += __shfl_xor(vv[r], 1, 64);
                    vv[r] += __shfl_xor(vv[r], 2, 64);
                }
                // Four consecutive quads (16 lanes) hold rows gr0 .. gr0 + 3 of four consecutive columns: a 4 x 4 transpose through
                // shuffles gives every one of them a ROW segment too, so that both triangles leave as 16-byte write-through stores
                // (the scalar form was 4 fabric writes per quad: 29 k per step, and the Cholesky loop waits for this sum).  A
                // diagonal block is written in full from both sides: its (i, j) and (j, i) sums are the same bits.
                const int a4 = (lane >> 2) & 3, lb = lane & ~15;
                float o[4];
#pragma unroll
                for (int b2 = 0; b2 < 4; ++b2) {
                    const float t0 = __shfl(vv[0], lb + 4 * b2, 64), t1 = __shfl(vv[1], lb + 4 * b2, 64);
                    const float t2 = __shfl(vv[2], lb + 4 * b2, 64), t3 = __shfl(vv[3], lb + 4 * b2, 64);
                    o[b2] = a4 == 0 ? t0 : a4 == 1 ? t1 : a4 == 2 ? t2 : t3;
                }
                if (part == 0 && quad < nq) {
                    const int idx = quad * 4, tt = idx >> 10, el = idx & 1023, code = s_tab[tt];
                    const int j = el >> 8, ln = (el >> 2) & 63;
                    const int gc = (code & 255) * 32 + (ln & 31);
                    const int gr0 = (code >> 8) * 32 + 8 * j + 4 * (ln >> 5);            // the quad: rows gr0 .. gr0 + 3 of column gc
                    if (gr0 + 3 < n && gc < n) {
                        vjf_st4_wt(red + P.red_G + (size_t)gc * n + gr0, vv[0], vv[1], vv[2], vv[3]);                // row gc, columns gr0 .. gr0 + 3
                        vjf_st4_wt(red + P.red_G + (size_t)(gr0 + a4) * n + (gc - a4), o[0], o[1], o[2], o[3]);        // row gr0 + a4, columns gc - a4 .. + 3
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int gr = gr0 + r;
                            if (gr < n && gc < n && ((code >> 8) != (code & 255) || gc <= gr)) {
                                vjf_st_wt(red + P.red_G + (size_t)gr * n + gc, vv[r]);
                                vjf_st_wt(red + P.red_G + (size_t)gc * n + gr, vv[r]);
                            }
                        }
                    }
                }
            };
            for (int quad = (hg * NT + tid) >> 2; quad < nq + qstride; quad += 2 * qstride) {   // (uniform trip count over the wavefront: shuffles inside)
                const int quadB = quad + qstride;
                float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
                float4 ta[16], tb[16];                                               // (at most 64 Gram workgroups: npq <= 16, one batch per lane)
                load16(ta, quad, part * npq); load16(tb, quadB, part * npq);
                add16(va, ta); add16(vb, tb);
                finish(quad, va); finish(quadB, vb);
            }
        }
        vjf_wg_signal_wt(A.cnt + MG_C_STAT, tid);
        { const int wg = hg, t = e; VJF_MG_STAMP(13); }
    }
}
