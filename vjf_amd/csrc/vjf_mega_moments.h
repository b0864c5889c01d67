// vjf_mega_moments.h -- the moments role of the one-launch route (vjf_mega_kernel.h).
#pragma once
#include "vjf_mega_common.h"

// ------------------------------------------------------------------------------------------------ moments role
// Launches without an RLS update (vjf_mega_lite_kernel): W and w_chol are constants, and the predictive moments of a tile at step t
// -- pt.mean = xs + Phi W, pt.logvar = log |L^-1 phi|^2 (module.py:64-77) -- depend on nothing but its posterior of step t - 1 and
// the noise.  They are a third of a trial workgroup's serial work per step (RBF features ~7 us, variance and mean ~12 us of ~52), and the
// launch has compute units to spare: these workgroups form them a step ahead, tile by tile, operation for operation what the trial role
// does (the same bits), and hand pt.mean | Phi W | pt.logvar over through memory.  One producer and one consumer per tile: step
// tags in the launch's counter block (MG_C_TAG_POST, MG_C_TAG_MOM), no counts.
static inline size_t vjf_mega_mom_lds_floats(const VjfPlan& P) {
    const size_t npad = (size_t)((P.n + 3) & ~3), LD = 65;                     // (two tiles side by side: 64 columns + 1)
    return npad * P.dxu + npad + (size_t)P.dxu * LD + (size_t)P.n * LD + (size_t)VJF_MG_WAVES * 64 + (size_t)VJF_MG_WAVES * 16 * LD + 64;
}

// one pass of the moments role: NG / 2 tiles (tile0, and tile1 when NG = 4 and tile1 >= 0) of step t, from their posterior tags to their
// moments tags
template <int NG>
__device__ __forceinline__ bool mg_moments_pass(const VjfPlan& P, const VjfMegaArgs& A, float* smem, const int t, const int tile0, const int tile1, const bool tri) {
    constexpr int LD = 16 * NG + 1, NW = VJF_MG_WAVES, NT = VJF_MG_THREADS, TR = VJF_MG_TR, NC = 16 * NG;   // NC columns = NG / 2 tiles
    const bool two = NG == 4 && tile1 >= 0;
    const int ncol = two ? NC : TR;                    // columns that hold trials (the elementwise loops stop there)
    const int tid0 = threadIdx.x;
    int tid = tid0, lane, wave;
    MG_PHASE();
    const int dz = P.dz, du = P.du, n = P.n, dxu = P.dxu, npad = (n + 3) & ~3;
    const float* S = A.state;
    float* SCW = A.state + P.off[VJF_SLOT_SCALARS];
    float* s_cen = smem; float* s_iw = s_cen + (size_t)npad * dxu;
    float* s_xu = s_iw + npad; float* s_phi = s_xu + (size_t)dxu * LD;
    float* s_red = s_phi + (size_t)n * LD; float* s_part = s_red + NW * NC;
    unsigned* cnt = A.cnt;
    const size_t sz = (size_t)A.B * dz, su = (size_t)A.B * du;
    constexpr int part_rows = VJF_MG_WAVES * 16;
    const float* mu_s = t ? A.mu + (size_t)(t - 1) * sz : A.mu0;
    const float* lv_s = t ? A.lv + (size_t)(t - 1) * sz : A.lv0;
    const float* eps_s = A.eps + (size_t)t * 2 * sz;
    const float* u_t = A.u ? A.u + (size_t)t * su : nullptr;
    // the tiles' posterior of step t - 1 (the trial role's write-through stores, then its tags)
    if (t > 0) {
        bool ok = vjf_wg_wait_sc1<VJF_POLL_SLEEP_LITE>(cnt + MG_C_TAG_POST + tile0, (unsigned)t, tid, SCW + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u);
        bool gone = vjf_abort_wg();
        if (two && !gone) { ok = vjf_wg_wait_sc1<VJF_POLL_SLEEP_LITE>(cnt + MG_C_TAG_POST + tile1, (unsigned)t, tid, SCW + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u) && ok; gone = vjf_abort_wg(); }
        if (!ok) vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_GATE2);
        if (gone) return false;
    } else __syncthreads();
    MG_PHASE();
    const int wg = tile0;                              // (diagnostic stamps: the workgroup that owns tile 0)
    VJF_MG_STAMP(11);
    // xs = mu + eps e^{lv / 2} (util.py:11-13; the prior at the first step of a run) and the inputs u: the trial role's expression
    for (int e = tid; e < NC * dxu; e += NT) {
        const int c = e / NC, col = e - c * NC, b = col & 31;
        if (col >= ncol) { s_xu[c * LD + col] = 0.f; continue; }
        const int b0 = (col < TR ? tile0 : tile1) * TR, nb = min(TR, A.B - b0);
        float v = 0.f;
        if (c < dz) {
            float m, l, ep = 0.f;
            if (mu_s) { m = b < nb ? vjf_ld_sc1(mu_s + (size_t)(b0 + b) * dz + c) : 0.f; l = b < nb ? vjf_ld_sc1(lv_s + (size_t)(b0 + b) * dz + c) : 0.f; }
            else { m = S[P.off[VJF_SLOT_PRIOR_MEAN] + c]; l = S[P.off[VJF_SLOT_PRIOR_LOGVAR] + c]; }
            if (b < nb) ep = eps_s[(size_t)(b0 + b) * dz + c];
            v = fmaf(ep, expf(0.5f * l), m);
        } else if (b < nb) v = u_t[(size_t)(b0 + b) * du + c - dz];
        s_xu[c * LD + col] = v;
    }
    __syncthreads(); MG_PHASE();
    VJF_MG_STAMP(12);
    // RBF features (functional.py:11-22): four centres per thread and column (one 16-byte LDS read of the centres per input dimension
    // instead of four 4-byte ones; per element the trial role's operations in the trial role's order: the same bits)
    for (int e = tid; e < NC * (npad >> 2); e += NT) {
        const int k4 = e / NC, col = e - k4 * NC, k = 4 * k4;
        float d2[4] = {0.f, 0.f, 0.f, 0.f};
        if (col < ncol) {
            // (the Gram role's copy of these lines, vjf_mega_gram.h, ON PURPOSE: behind one shared routine the moments role's code moves and
            //  vjf_mega_lite_act_kernel's v_writelane / v_readlane count goes from 3570 to 3584 -- profiles/mega_split_isa.txt, candidate 1)
            auto dim = [&](float x, const float4& cc) {                        // (one input dimension: the trial role's order of operations)
                float d;
                d = x - cc.x; d2[0] = fmaf(d, d, d2[0]); d = x - cc.y; d2[1] = fmaf(d, d, d2[1]);
                d = x - cc.z; d2[2] = fmaf(d, d, d2[2]); d = x - cc.w; d2[3] = fmaf(d, d, d2[3]);
            };
            int c = 0;
            for (; c + 3 < dxu; c += 4) {                                      // four dimensions' LDS loads in flight together (a loop of
                const float x0 = s_xu[c * LD + col], x1 = s_xu[(c + 1) * LD + col], x2 = s_xu[(c + 2) * LD + col], x3 = s_xu[(c + 3) * LD + col];   // single loads is a chain of LDS round trips)
                const float4 c0 = *reinterpret_cast<const float4*>(s_cen + c * npad + k);
                const float4 c1 = *reinterpret_cast<const float4*>(s_cen + (c + 1) * npad + k);
                const float4 c2 = *reinterpret_cast<const float4*>(s_cen + (c + 2) * npad + k);
                const float4 c3 = *reinterpret_cast<const float4*>(s_cen + (c + 3) * npad + k);
                dim(x0, c0); dim(x1, c1); dim(x2, c2); dim(x3, c3);
            }
            for (; c < dxu; ++c) dim(s_xu[c * LD + col], *reinterpret_cast<const float4*>(s_cen + c * npad + k));
        }
        const float4 iw = *reinterpret_cast<const float4*>(s_iw + k);
        const float iwv[4] = {iw.x, iw.y, iw.z, iw.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (k + q < n) s_phi[(k + q) * LD + col] = col < ncol ? expf(d2[q] * iwv[q]) : 0.f;
    }
    __syncthreads(); MG_PHASE();
    VJF_MG_STAMP(13);
    int mean_nsl = 1;
    {   // predictive variance and mean: vjf_mega_trial's stage 2, wavefront for wavefront
        const __amdgpu_buffer_rsrc_t r_xt = vjf_rsrc(A.xt);
        const float* Wm = S + P.off[VJF_SLOT_W_MEAN];
        const int ntile = (n + 15) >> 4;
        float v2[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) v2[g] = 0.f;
        const int nsl = min(NW, part_rows / 16);
        const int msl = nsl - 1 - wave;
        const int mper = (((n + 3) >> 2) + nsl - 1) / nsl * 4;
        const int mkb = msl * mper, mke = min(n, (msl + 1) * mper);
        const bool mpre = wave < nsl && ((mke - mkb + 3) >> 2) <= 16;
        float am[16];
        if (mpre && mke > mkb) mg_mma2_ld16(am, Wm, dz, dz, 0, mkb, mke, 0, lane);
        for (int r = 0; r * NW < ntile; r += 2) {
            int j0p[2], Kp[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int rr = r + h, idx = (rr & 1) ? rr * NW + NW - 1 - wave : rr * NW + wave;
                const int tt = ntile - 1 - idx;
                j0p[h] = (idx < ntile) ? tt * 16 : -1;
                Kp[h] = tri ? min(n, tt * 16 + 16) : n;
            }
            if (j0p[0] < 0) { j0p[0] = j0p[1]; Kp[0] = Kp[1]; j0p[1] = -1; }
            mg_varN<NG, LD>(v2, r_xt, n, j0p[0], Kp[0], j0p[1], Kp[1], (mg_lds_cf*)s_phi, lane, two);
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            v2[g] += __shfl_xor(v2[g], 16, 64); v2[g] += __shfl_xor(v2[g], 32, 64);
            if (lane < 16) s_red[wave * NC + 16 * g + lane] = v2[g];
        }
        if (wave < nsl) {
            vjf_f32x4 acc[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
            if (mpre) { if (mke > mkb) mg_mmaN_mm16<NG, LD>(acc, am, s_phi, dz, 0, mkb, mke, 0, lane, two); }
            else {
                // (more than 512 features: the slice in batches of 16 k-steps)
                for (int s0 = 0; 4 * s0 < mke - mkb; s0 += 16) {
                    float a2[16];
                    mg_mma2_ld16(a2, Wm, dz, dz, 0, mkb, mke, s0, lane);
                    mg_mmaN_mm16<NG, LD>(acc, a2, s_phi, dz, 0, mkb, mke, s0, lane, two);
                }
            }
            float* pr = s_part + (size_t)(msl * 16 + 4 * (lane >> 4)) * LD + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int g = 0; g < NG; ++g) pr[r * LD + 16 * g] = acc[g][r];
        }
        mean_nsl = nsl;
    }
    __syncthreads(); MG_PHASE();
    VJF_MG_STAMP(14);
    // out, per tile: [pt.mean (dz x 32) | Phi W (dz x 32) | pt.logvar (32)], write-through; then the tags
    const int mlen = (2 * dz + 1) * TR;
    for (int e = tid; e < NC * dz; e += NT) {
        const int j = e / NC, col = e - j * NC, b = col & 31;
        if (col >= ncol) continue;
        float* mb = A.mom + ((size_t)(col < TR ? tile0 : tile1) * 2 + (size_t)(t & 1)) * (size_t)mlen;
        float v = 0.f;
        for (int sl = 0; sl < mean_nsl; ++sl) v += s_part[(size_t)(sl * 16 + j) * LD + col];
        vjf_st_wt(mb + j * TR + b, s_xu[j * LD + col] + v);
        vjf_st_wt(mb + TR * dz + j * TR + b, v);
    }
    if (tid < ncol) {
        float* mb = A.mom + ((size_t)(tid < TR ? tile0 : tile1) * 2 + (size_t)(t & 1)) * (size_t)mlen;
        float v = 0.f;
        for (int w = 0; w < NW; ++w) v += s_red[w * NC + tid];
        vjf_st_wt(mb + 2 * TR * dz + (tid & 31), logf(v));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __hip_atomic_store(cnt + MG_C_TAG_MOM + tile0, (unsigned)(t + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (two) __hip_atomic_store(cnt + MG_C_TAG_MOM + tile1, (unsigned)(t + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    VJF_MG_STAMP(15);
    return true;
}

__device__ __forceinline__ void vjf_mega_moments(const VjfPlan& P, const VjfMegaArgs& A, float* smem, const int mw) {
    const int tid0 = threadIdx.x;
    const int n = P.n, dxu = P.dxu, npad = (n + 3) & ~3;
    const float* S = A.state;
    float* SCW = A.state + P.off[VJF_SLOT_SCALARS];
    float* s_cen = smem; float* s_iw = s_cen + (size_t)npad * dxu;
    mg_stage_centres(P, S, s_cen, s_iw, tid0);
    // (the row-major L^-1 of this launch: the trial workgroups' first act)
    if (!vjf_wg_wait_sc1<VJF_POLL_SLEEP_LITE>(A.cnt + MG_C_XT, (unsigned)A.n_trial, tid0, SCW + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u))
        vjf_status_or(SCW + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_K1);
    if (vjf_abort_wg()) return;
    // (w_chol upper triangular: the state's flag, or what the trial workgroups saw while they transposed it)
    const bool tri = vjf_ld_sc1(SCW + VJF_SC_TRI_CLEAN) != 0.f || __hip_atomic_load(A.cnt + MG_C_XT + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
    for (int t = 0; t < A.T; ++t) {
        // this workgroup's tiles mw, mw + n_mom, ..: two at a time side by side (every operand load of L^-1 serves both), a last one alone
        // (ONE instantiation of the pass, four column groups, for both cases -- tile1 < 0: the second half idles.  With a two-group
        //  instantiation beside it hipcc (ROCm 7.2.0) fails in its backend: "Illegal instruction detected ... $src_shared_base",
        //  DESIGN.md section 3 "Toolchain note"; either instantiation alone compiles)
        int tile = mw;
        if (A.n_mom >= A.ntiles) {                       // (uniform) a workgroup per tile: the one-tile layout, the trial role's own
            if (tile < A.ntiles && !mg_moments_pass<2>(P, A, smem, t, tile, -1, tri)) return;
            continue;
        }
        for (; tile < A.ntiles; tile += 2 * A.n_mom)
            if (!mg_moments_pass<4>(P, A, smem, t, tile, tile + A.n_mom < A.ntiles ? tile + A.n_mom : -1, tri)) return;
    }
}
