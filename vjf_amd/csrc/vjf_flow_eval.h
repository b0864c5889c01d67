// vjf_flow_eval.h -- g = Phi([x, u]) w_mean and the columns of A = dg/dx = -w_mean^T G,  G[k][j] = phi_k (x_j - c_kj) / width_k^2,  of one
// tile of 16 trials at the point [x, u] in FcTile's s_x: what a kernel needs of the mean map f = x + g besides the step itself (J = I + A).
//
// Column j of A for the tile's 16 trials is one MFMA product: its A operand is w_mean^T (shared by every trial and every j), its B
// operand the n x 16 matrix  phi[k][b] (c[k][j] - x[b][j]) / width_k^2  formed in registers from the features in LDS, so the dout
// columns are dout accumulator tiles, `vg` of them per pass (the partial products of a pass are in LDS together).  K is split over the
// four wavefronts as in the x step (fc_k_range) and the four partial products are added in a fixed order: a trial is one MFMA column,
// its bits depend on its own row of s_x alone.
//
// This is vjf_fixed_point_kernel's `evaluate`, statement for statement.  That kernel keeps its own copy as a lambda: with the lambda
// replaced by a call of this function its assembly moves (profiles/smoother_isa.txt: <1,1> 92 -> 96 and <0,1> 91 -> 97 VGPRs, the
// other two forms shorter but different) and it runs 5 % longer (profiles/trial_algebra_ab.txt); the smoother, the sampler and the
// EKF call this one.  Whoever changes one changes both.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_forecast_kernel.h"     // vjf_rollout_step.h: the x step, FcTile, VJF_FC_THREADS / _WAVES, vjf_f32x4, VJF_LDT

#define VJF_FLOW_MV 4                // columns of A whose accumulators a wavefront holds while it walks its share of K

namespace {
struct FlowEval {
    const float* W;          // w_mean (n, dout): the model's array, or its copy in LDS
    const float* c;          // centroids (n, d) in global memory (read when !CL; CL: S.s_c)
    const float* s_iw2;      // n            1 / width^2
    float* s_g;              // dout x LD    g
    float* s_A;              // dout x dout x LD   A, [j][i][trial] = dg_i / dx_j
    float* s_ap;             // NW x vg x doutp x LD   the wavefronts' partial products of one pass
    int vg;                  // columns of A per pass
};

// g and A at [x, u] in S.s_x: into E.s_g and E.s_A.  Barriers inside; s_x is complete before it and s_g, s_A behind it.
// CL: centroids in LDS (S.s_c);  NO: output tiles of w_mean^T (dout <= 16 NO).
template <bool CL, int NO>
__device__ __forceinline__ void flow_evaluate(const FcTile& S, const FlowEval& E) {
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_FC_WAVES, NTH = VJF_FC_THREADS, MV = VJF_FLOW_MV;
    const int d = S.d, dout = S.dout, vg = E.vg, doutp = S.doutp, tid = S.tid, wave = S.wave, mi = S.mi, kk = S.kk, r4 = S.r4;
    const float* W = E.W;
    fc_features<CL>(S, E.c);
    __syncthreads();
    fc_product_masked(S, W);                      // Phi w_mean, K split over the four wavefronts as in the roll-out
    for (int v0 = 0; v0 < dout; v0 += vg) {
        const int vn = min(vg, dout - v0);
        for (int g0 = 0; g0 < vn; g0 += MV) {
            vjf_f32x4 acc[MV][NO];
            float xj[MV];
#pragma unroll
            for (int vv = 0; vv < MV; ++vv) {
                xj[vv] = S.s_x[(g0 + vv < vn ? v0 + g0 + vv : 0) * LD + mi];
#pragma unroll
                for (int ot = 0; ot < NO; ++ot) acc[vv][ot] = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
            }
            for (int k0 = S.kb; k0 < S.ke; k0 += 4) {
                const bool kv = k0 + kk < S.ke;
                const int k = kv ? k0 + kk : S.kb;
                const float gr = S.s_phi[k * LD + mi] * E.s_iw2[k];
                float aw[NO];
#pragma unroll
                for (int ot = 0; ot < NO; ++ot) {
                    aw[ot] = 0.f;
                    if (ot * 16 < dout) {                            // (uniform)
                        const bool ok = kv && ot * 16 + mi < dout;
                        const float wv = W[ok ? (size_t)k * dout + ot * 16 + mi : 0];
                        aw[ot] = ok ? wv : 0.f;
                    }
                }
#pragma unroll
                for (int vv = 0; vv < MV; ++vv)
                    if (g0 + vv < vn) {                              // (uniform)
                        const int j = v0 + g0 + vv;
                        const float cv = CL ? S.s_c[k * d + j] : E.c[(size_t)k * d + j];
                        const float bv = kv ? gr * (cv - xj[vv]) : 0.f;
#pragma unroll
                        for (int ot = 0; ot < NO; ++ot)
                            if (ot * 16 < dout) acc[vv][ot] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[ot], bv, acc[vv][ot], 0, 0, 0);
                    }
            }
#pragma unroll
            for (int vv = 0; vv < MV; ++vv)
                if (g0 + vv < vn) {
#pragma unroll
                    for (int ot = 0; ot < NO; ++ot)
                        if (ot * 16 < dout) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) E.s_ap[((wave * vg + g0 + vv) * doutp + ot * 16 + r4 + r) * LD + mi] = acc[vv][ot][r];
                        }
                }
        }
        __syncthreads();
        // the four partials in a fixed order
        if (v0 == 0)
            for (int i = tid; i < dout * TB; i += NTH) {
                const int b = i & (TB - 1), j = i / TB;
                float s = S.s_part[j * LD + b];
#pragma unroll
                for (int w = 1; w < NW; ++w) s += S.s_part[(w * doutp + j) * LD + b];
                E.s_g[j * LD + b] = s;
            }
        for (int i = tid; i < vn * dout * TB; i += NTH) {
            const int b = i & (TB - 1), r = i / TB, vl = r / dout, ii = r - vl * dout;
            float s = E.s_ap[(vl * doutp + ii) * LD + b];
#pragma unroll
            for (int w = 1; w < NW; ++w) s += E.s_ap[((w * vg + vl) * doutp + ii) * LD + b];
            E.s_A[((v0 + vl) * dout + ii) * LD + b] = s;
        }
        __syncthreads();
    }
}
}  // namespace
