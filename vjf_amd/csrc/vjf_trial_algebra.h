// vjf_trial_algebra.h -- what the kernels that walk a tile of 16 trials over the learned flow share of their per-trial linear algebra:
//   all four (vjf_fixed_point_kernel.h, vjf_smooth_kernel.h, vjf_smooth_sample_kernel.h, vjf_ekf_kernel.h)
//       the lane view -- four trials per wavefront, sixteen lanes per trial, lane l of a trial owning indices l and l + 16 --, the index
//       of a lower triangle [i (i + 1) / 2 + p][trial], the butterfly sum over a trial's sixteen lanes, the finite test, and the
//       common part of the LDS sums
//   the smoother and the EKF
//       ta_factor, the in-place Cholesky factor of such a triangle; ta_stage_triangle and ta_emit_moments, a carried covariance
//       triangle in from a full matrix or log-variances and mean / var / cov out of it
// The fixed-point kernel and the sampler keep their own factorisation (profiles/trial_algebra_ab.txt).  Everything is inlined.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_flow_eval.h"           // flow_evaluate; the x step's FcTile, VJF_FC_THREADS, VJF_LDT

namespace {
// floats of dynamic LDS every kernel of the family has: the x step's buffers plus 1 / width^2, `vectors` vectors (dout x LD), the
// dout x dout block that holds A, `triangles` lower triangles, one pass's partial products (vg columns of A) and (cen_lds) w_mean
static inline size_t vjf_trial_lds_floats(int n, int d, int dout, int vg, bool cen_lds, int vectors, int triangles) {
    const size_t doutp = ((size_t)dout + 15) / 16 * 16, LD = VJF_LDT, ntri = (size_t)dout * (dout + 1) / 2;
    return vjf_fc_lds_floats(n, d, dout, cen_lds) + (size_t)n + vectors * (size_t)dout * LD + (size_t)dout * dout * LD + triangles * ntri * LD +
           (size_t)VJF_FC_WAVES * vg * doutp * LD + (cen_lds ? (size_t)n * dout : 0);
}

// the trial of this lane within the tile and the lane's place among the trial's sixteen
__device__ __forceinline__ int ta_trial(const FcTile& S) { return S.wave * 4 + (S.lane >> 4); }
__device__ __forceinline__ int ta_l16(const FcTile& S) { return S.lane & 15; }

__device__ __forceinline__ int ta_tri(int i, int p) { return i * (i + 1) / 2 + p; }
__device__ __forceinline__ float ta_sum16(float s) {
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
    return s;
}
__device__ __forceinline__ bool ta_isfin(float v) { return fabsf(v) < INFINITY; }      // (a NaN compares false)

// The lower triangle at s_T becomes its Cholesky factor, a row per lane, column by column: what another lane needs of a row comes by a
// shuffle inside the sixteen.  True in every lane of the trial if every pivot is positive and finite.  The whole wavefront calls it, or
// none of it.
template <int NO>
__device__ __forceinline__ bool ta_factor(int b, int l16, int dout, float* s_T) {
    constexpr int LD = VJF_LDT;
    bool ok = true;
    for (int j = 0; j < dout; ++j) {
        const int own = j & 15, ej = j >> 4;
        const int rj = min(l16 + 16 * ej, dout - 1);              // the row of this lane that lane `own` has as row j
        float a[2] = {0.f, 0.f};
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            a[e] = (i >= j && i < dout) ? s_T[ta_tri(i, j) * LD + b] : 0.f;
        }
        for (int p = 0; p < j; ++p) {
            const float ljp = __shfl(s_T[ta_tri(rj, min(p, rj)) * LD + b], own, 16);
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int i = l16 + 16 * e;
                if (i >= j && i < dout) a[e] = fmaf(-s_T[ta_tri(i, p) * LD + b], ljp, a[e]);
            }
        }
        const float piv = __shfl(ej ? a[1] : a[0], own, 16);
        ok = ok && piv > 0.f && piv < INFINITY;
        const float dj = sqrtf(piv);
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i >= j && i < dout) s_T[ta_tri(i, j) * LD + b] = i == j ? dj : a[e] / dj;
        }
    }
    return ok;
}

// ---- carried moments: a mean (dout x LD) and the lower triangle of a covariance

// the triangle at s_P from this tile's rows of `cov` (B, dout, dout; its lower triangle is read) or, without one, the diagonal
// exp(lv) of `lv` (B, dout).  Rows beyond the batch carry the identity: finite, never stored.  All threads; no barrier.
__device__ __forceinline__ void ta_stage_triangle(const FcTile& S, float* s_P, const float* cov, const float* lv) {
    const int dout = S.dout;
    const size_t row0 = (size_t)S.b0 * dout;
    for (int i = S.tid; i < 16 * dout * dout; i += VJF_FC_THREADS) {
        const int b = i / (dout * dout), r = i - b * dout * dout, ii = r / dout, j = r - ii * dout;
        if (j <= ii) {
            float v = ii == j ? 1.f : 0.f;
            if (b < S.nb) v = cov ? cov[row0 * dout + i] : (ii == j ? expf(lv[row0 + b * dout + ii]) : 0.f);
            s_P[ta_tri(ii, j) * VJF_LDT + b] = v;
        }
    }
}

// this tile's rows of mean, var and (if asked for: cov != null) cov of row t from the mean at s_m and the triangle at s_P; `edge`: the
// full covariance to cov_edge (B, dout, dout) as well.  All threads; no barrier.
__device__ __forceinline__ void ta_emit_moments(const FcTile& S, const float* s_m, const float* s_P, int t, size_t rowT, float* mean, float* var,
                                             float* cov, bool edge, float* cov_edge) {
    constexpr int LD = VJF_LDT, NTH = VJF_FC_THREADS;
    const int dout = S.dout, nb = S.nb;
    const size_t row0 = (size_t)S.b0 * dout;
    for (int i = S.tid; i < nb * dout; i += NTH) {
        const int bb = i / dout, j = i - bb * dout;
        mean[(size_t)t * rowT + row0 + i] = s_m[j * LD + bb];
        var[(size_t)t * rowT + row0 + i] = s_P[ta_tri(j, j) * LD + bb];
    }
    float* full = cov ? cov + ((size_t)t * rowT + row0) * dout : nullptr;
    if (full || edge)
        for (int i = S.tid; i < nb * dout * dout; i += NTH) {
            const int bb = i / (dout * dout), r = i - bb * dout * dout, ii = r / dout, j = r - ii * dout;
            const float v = s_P[ta_tri(max(ii, j), min(ii, j)) * LD + bb];
            if (full) full[i] = v;
            if (edge) cov_edge[row0 * dout + i] = v;
        }
}
}  // namespace
