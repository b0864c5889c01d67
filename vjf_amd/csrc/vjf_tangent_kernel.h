// vjf_tangent_kernel.h -- tangent dynamics of the mean map of RBFDS.forward(sampling=False) (vjf/model.py:334-340 over
// vjf/module.py:64-77):  f(x, u) = x + Phi([x, u]) w_mean,  J = df/dx = I - w_mean^T G,  G[k][j] = phi_k (x_j - c_kj) / width_k^2.
//
//   vjf_tangent_rollout_kernel   one workgroup per tile of 16 trials loops over the steps of a chunk inside the kernel and keeps x and
//                                the tangent frame Q (dout x m per trial) in LDS:  features of [x_t, u_t] -> x_{t+1} = x_t + Phi w_mean
//                                -> V = J(x_t, u_t) Q -> every `qr` steps one pass of modified Gram-Schmidt on V, log R_ii summed.
//
// The x step is vjf_fc_rollout_kernel's (vjf_rollout_step.h: same tiling, same MFMA steps, W[t] = w_mean for every t).  J q = q - w_mean^T s with
// s_k = (phi_k / width_k^2)(x^T q - (C_x q)_k): two products with matrices every trial and every tangent vector share, so tangent
// vector v of the tile's 16 trials is one tile of 16 MFMA columns, [v][component][VJF_LDT] in LDS.  Per tile of 16 features a wavefront
// computes C_x Q_v (K = dout), scales the 16 x 16 accumulator in registers and feeds it back as the B operand of w_mean^T s: the
// accumulator's register r of the lanes kk = 0 .. 3 holds features 4 kk + r of the tile, so MFMA step r of the second product takes
// rows 4 kk + r of w_mean as its A operand -- a permutation of K, no trip through LDS.  K (the feature tiles) is split over the four
// wavefronts, tile ft to wavefront ft mod 4, and the four partial products are added in a fixed order.
// Workgroups are independent: no cooperative launch, no hand-off.  Included by vjf_host_tangent.h.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_forecast_kernel.h"     // vjf_rollout_step.h: the x step, FcTile, VJF_FC_THREADS / _WAVES / _KQ, vjf_f32x4, VJF_LDT

#define VJF_TG_MV 4                  // tangent vectors whose accumulators a wavefront holds while it walks its feature tiles
#define VJF_TG_MAXDOUT 64            // dout <= 64: C_x Q is at most 16 MFMA steps deep, w_mean^T s at most 4 output tiles

namespace {
struct VjfTgArgs {
    const float* x_in;       // (B, dout): the state the chunk starts from
    const float* u;          // (Tc, B, du) or null
    const float* q_in;       // (B, dout, m) or null: the first m columns of I
    const float* c; const float* logw;     // centroids (n, d), log widths (n)
    const float* w;          // w_mean (n, dout)
    const float* lsum_in;    // (B, m) or null: the sums start from 0
    float* x_out;            // (B, dout)
    float* q_out;            // (B, dout, m)
    float* lsum;             // (B, m) or null
    float* lhist;            // (intervals, B, m), the row of the interval the chunk starts in, or null
    int Tc, B, n, d, dout, m;
    int qr;                  // steps per interval (0: never orthonormalise)
    int tq;                  // steps of the chunk's first interval taken by earlier chunks
    int last;                // the chunk ends the horizon: orthonormalise behind its last step (with Tc = 0: the start)
    int vg;                  // tangent vectors per pass (the partial products of a pass are in LDS together)
};

// the x step's buffers plus 1 / width^2, the frame, x^T q and the sums, one pass's partial products and (cen_lds) w_mean
static inline size_t vjf_tangent_lds_floats(int n, int d, int dout, int m, int vg, bool cen_lds) {
    const size_t doutp = ((size_t)dout + 15) / 16 * 16, LD = VJF_LDT;
    return vjf_fc_lds_floats(n, d, dout, cen_lds) + (size_t)n + (size_t)m * dout * LD + 2 * (size_t)m * LD +
           (size_t)VJF_FC_WAVES * vg * doutp * LD + (cen_lds ? (size_t)n * dout : 0);
}

// NT, CL: vjf_fc_rollout_kernel's forms of the x step (NT > 0: this lane's elements of w_mean stay in registers for the whole chunk;
//         NT == 0: any shape, they are read when they are used) and of the shared operands (CL: centroids and w_mean in LDS, else read from
//         global memory when they are used).  All forms issue the same MFMA steps on the same operands in the same order.
// NO: output tiles of w_mean^T s, dout <= 16 NO.
template <int NT, bool CL, int NO>
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_tangent_rollout_kernel(VjfTgArgs A) {
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_FC_WAVES, NTH = VJF_FC_THREADS, MV = VJF_TG_MV;
    static_assert(NT == 0 || NT == NO, "the register form of the x step covers dout <= 16 NT: the same tiles as NO");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FcTile S = fc_tile(smem, A.n, A.d, A.dout, A.B);     // s_phi, s_x, s_part, s_w2: the x step's
    const int n = S.n, d = S.d, dout = S.dout, du = S.du, m = A.m, vg = A.vg, doutp = S.doutp;
    float *s_phi = S.s_phi, *s_x = S.s_x;
    float* s_iw2 = S.rest;                        // n            1 / width^2
    float* s_q = s_iw2 + n;                       // m x dout x LD     the frame: [v][j][trial]
    float* s_xq = s_q + m * dout * LD;            // m x LD       x_t^T q_v
    float* s_ls = s_xq + m * LD;                  // m x LD       running sums of log R_vv
    float* s_vp = s_ls + m * LD;                  // NW x vg x doutp x LD   the wavefronts' partial products of w_mean^T s, one pass
    const float* s_c = S.s_c = s_vp + NW * vg * doutp * LD;   // n x d   centroids (CL): behind this kernel's buffers
    float* s_wm = S.s_c + n * d;                  // n x dout     w_mean (CL)
    const int tid = S.tid, lane = S.lane, wave = S.wave, b0 = S.b0, nb = S.nb, mi = S.mi, kk = S.kk, r4 = S.r4, nft = (n + 15) / 16;
    const size_t row0 = (size_t)b0 * dout, su = (size_t)A.B * du, qrow0 = (size_t)b0 * dout * m, bm = (size_t)A.B * m;

    fc_stage<CL, true>(S, A.logw, A.c, s_iw2, A.x_in, nullptr, A.Tc > 0 ? A.u : nullptr);
    if (CL) for (int i = tid; i < n * dout; i += NTH) s_wm[i] = A.w[i];
    for (int i = tid; i < TB * dout * m; i += NTH) {
        const int b = i / (dout * m), r = i - b * dout * m, j = r / m, v = r - j * m;
        float q = 0.f;
        if (b < nb) q = A.q_in ? A.q_in[qrow0 + i] : (j == v ? 1.f : 0.f);
        s_q[(v * dout + j) * LD + b] = q;
    }
    for (int i = tid; i < TB * m; i += NTH) {
        const int b = i / m, v = i - b * m;
        s_ls[v * LD + b] = (b < nb && A.lsum_in) ? A.lsum_in[(size_t)b0 * m + i] : 0.f;
    }
    float aw[NT > 0 ? NT : 1][VJF_FC_KQ];                // (NT > 0) this lane's A operands of the x step: w_mean, the same at every step
    if constexpr (NT > 0) fc_fetch_w(S, A.w, aw);

    // One pass of modified Gram-Schmidt in column order on every trial's frame, in place: a wavefront takes four trials, sixteen lanes
    // each; lane g of a trial owns components g, g + 16, .. of every column and reads and writes nothing else, so the pass needs no
    // barrier.  The sums over components: each lane's own in component order, then a butterfly over the sixteen lanes (every lane ends
    // with the same bits).  R_vv = |column v| > 0; its log goes to the running sum and to `hist` (B, m) if given.
    auto orthonormalise = [&](float* hist) {
        const int b = wave * 4 + (lane >> 4), g = lane & 15;
        const bool bv = b < nb;
        auto sum16 = [](float s) {
            s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
            return s;
        };
        for (int v = 0; v < m; ++v) {
            float* qv_p = s_q + (size_t)v * dout * LD + b;
            float qv[4], ss = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = g + 16 * e;
                qv[e] = j < dout ? qv_p[j * LD] : 0.f;
                ss = fmaf(qv[e], qv[e], ss);
            }
            float r = sqrtf(sum16(ss));
            if (!bv) r = 1.f;                             // (rows beyond the batch hold zeros and stay zeros)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = g + 16 * e;
                qv[e] = qv[e] / r;
                if (j < dout) qv_p[j * LD] = qv[e];
            }
            if (g == 0 && bv) {
                const float lg = logf(r);
                s_ls[v * LD + b] += lg;
                if (hist) hist[(size_t)(b0 + b) * m + v] = lg;
            }
            for (int w = v + 1; w < m; ++w) {
                float* qw_p = s_q + (size_t)w * dout * LD + b;
                float qw[4], dt = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = g + 16 * e;
                    qw[e] = j < dout ? qw_p[j * LD] : 0.f;
                    dt = fmaf(qv[e], qw[e], dt);
                }
                dt = sum16(dt);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = g + 16 * e;
                    if (j < dout) qw_p[j * LD] = fmaf(-dt, qv[e], qw[e]);
                }
            }
        }
    };
    __syncthreads();
    if (A.Tc == 0 && A.qr > 0 && A.last) {
        orthonormalise(nullptr);
        __syncthreads();
    }

    for (int t = 0; t < A.Tc; ++t) {
        // the next step's control input: in flight while the features are computed
        const float* un = du > 0 && t + 1 < A.Tc ? A.u + (size_t)(t + 1) * su + (size_t)b0 * du : nullptr;
        const float u0 = fc_u_ahead(S, un);
        fc_features<CL>(S, A.c);
        // x_t^T q_v
        for (int i = tid; i < TB * m; i += NTH) {
            const int v = i / TB, b = i - v * TB;
            float a = 0.f;
            for (int j = 0; j < dout; ++j) a = fmaf(s_x[j * LD + b], s_q[(v * dout + j) * LD + b], a);
            s_xq[v * LD + b] = a;
        }
        __syncthreads();

        // Phi w_mean, K split over the four wavefronts as in the roll-out (streamed: every address inside w_mean)
        if constexpr (NT > 0) fc_product_reg(S, aw);
        else fc_product_masked(S, CL ? s_wm : A.w);

        // V = Q - w_mean^T s, `vg` tangent vectors per pass
        for (int v0 = 0; v0 < m; v0 += vg) {
            const int vn = min(vg, m - v0);
            for (int g0 = 0; g0 < vn; g0 += MV) {
                vjf_f32x4 acc[MV][NO];
#pragma unroll
                for (int vv = 0; vv < MV; ++vv)
#pragma unroll
                    for (int ot = 0; ot < NO; ++ot) acc[vv][ot] = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
                for (int ft = wave; ft < nft; ft += NW) {
                    // the tile's operands, shared by the tangent vectors: rows of C_x (A of the first product), rows 4 kk + r of w_mean
                    // (A of step r of the second), phi / width^2 of the features this lane's accumulator registers hold
                    const int f1 = ft * 16 + mi;
                    float ac[VJF_TG_MAXDOUT / 4], aw2[NO][4], gr[4];
#pragma unroll
                    for (int q = 0; q < VJF_TG_MAXDOUT / 4; ++q) {
                        ac[q] = 0.f;
                        if (4 * q < dout) {                              // (uniform)
                            const int j = 4 * q + kk;
                            const bool ok = f1 < n && j < dout;
                            const float cv = CL ? s_c[ok ? f1 * d + j : 0] : A.c[ok ? (size_t)f1 * d + j : 0];
                            ac[q] = ok ? cv : 0.f;
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f2 = ft * 16 + 4 * kk + r;
                        const bool fv = f2 < n;
                        gr[r] = fv ? s_phi[f2 * LD + mi] * s_iw2[f2] : 0.f;
#pragma unroll
                        for (int ot = 0; ot < NO; ++ot) {
                            aw2[ot][r] = 0.f;
                            if (ot * 16 < dout) {                        // (uniform)
                                const int i = ot * 16 + mi;
                                const bool ok = fv && i < dout;
                                const float wv = CL ? s_wm[ok ? f2 * dout + i : 0] : A.w[ok ? (size_t)f2 * dout + i : 0];
                                aw2[ot][r] = ok ? wv : 0.f;
                            }
                        }
                    }
#pragma unroll
                    for (int vv = 0; vv < MV; ++vv) {
                        if (g0 + vv < vn) {                              // (uniform)
                            const int v = v0 + g0 + vv;
                            const float* qp = s_q + (size_t)v * dout * LD + mi;
                            vjf_f32x4 p = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                            for (int q = 0; q < VJF_TG_MAXDOUT / 4; ++q)
                                if (4 * q < dout) {                      // (uniform)
                                    const int j = 4 * q + kk;
                                    const float bq = qp[(j < dout ? j : 0) * LD];
                                    p = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[q], j < dout ? bq : 0.f, p, 0, 0, 0);
                                }
                            const float xq = s_xq[v * LD + mi];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float sv = gr[r] * (xq - p[r]);
#pragma unroll
                                for (int ot = 0; ot < NO; ++ot)
                                    if (ot * 16 < dout) acc[vv][ot] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw2[ot][r], sv, acc[vv][ot], 0, 0, 0);
                            }
                        }
                    }
                }
#pragma unroll
                for (int vv = 0; vv < MV; ++vv)
                    if (g0 + vv < vn) {
#pragma unroll
                        for (int ot = 0; ot < NO; ++ot)
                            if (ot * 16 < dout) {
#pragma unroll
                                for (int r = 0; r < 4; ++r) s_vp[((wave * vg + g0 + vv) * doutp + ot * 16 + r4 + r) * LD + mi] = acc[vv][ot][r];
                            }
                    }
            }
            __syncthreads();
            // the four partials in a fixed order
            for (int i = tid; i < vn * dout * TB; i += NTH) {
                const int b = i & (TB - 1), r = i / TB, vl = r / dout, j = r - vl * dout;
                float s = s_vp[(vl * doutp + j) * LD + b];
#pragma unroll
                for (int w = 1; w < NW; ++w) s += s_vp[((w * vg + vl) * doutp + j) * LD + b];
                float* qe = s_q + ((size_t)(v0 + vl) * dout + j) * LD + b;
                *qe = *qe - s;
            }
            if (v0 + vg < m) __syncthreads();
        }

        // x_{t+1} = x_t + (p0 + p1 + p2 + p3)
        fc_advance(S, [](int, float v) { return v; });
        fc_u_advance(S, un, u0);
        __syncthreads();

        if (A.qr > 0 && ((A.tq + t + 1) % A.qr == 0 || (A.last && t + 1 == A.Tc))) {
            orthonormalise(A.lhist ? A.lhist + (size_t)((A.tq + t) / A.qr) * bm : nullptr);
            __syncthreads();
        }
    }

    for (int i = tid; i < nb * dout; i += NTH) {
        const int b = i / dout, j = i - b * dout;
        A.x_out[row0 + i] = s_x[j * LD + b];
    }
    for (int i = tid; i < nb * dout * m; i += NTH) {
        const int b = i / (dout * m), r = i - b * dout * m, j = r / m, v = r - j * m;
        A.q_out[qrow0 + i] = s_q[(v * dout + j) * LD + b];
    }
    if (A.lsum)
        for (int i = tid; i < nb * m; i += NTH) {
            const int b = i / m, v = i - b * m;
            A.lsum[(size_t)b0 * m + i] = s_ls[v * LD + b];
        }
}
}  // namespace
