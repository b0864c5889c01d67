// vjf_ops_kernels.h -- stand-alone operator kernels behind the vjf.module / vjf.functional surface.
// These serve the reference's operator API one call at a time; the fused step does not use them.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_trial_kernel.h"        // VJF_K1_THREADS
#include "vjf_trial_mfma_kernel.h"   // mma_tile, vjf_f32x4, VJF_LDT

// functional.rbf (vjf/functional.py:11-22): workgroup = 256 centroids x 16 trials.  A thread runs ITS centroid (its own row, read
// 8 coordinates at a time) against the 16 trials staged in LDS (same address on every lane: broadcast reads, 16 bytes at a
// time when d is a multiple of 4); each distance is the same j-ordered fmaf chain as a plain loop.  grid = (ceil(n / 256), ceil(B / 16)).
__global__ __launch_bounds__(256) void vjf_rbf_kernel(const float* __restrict__ x, const float* __restrict__ c, const float* __restrict__ logw,
                                                      float* __restrict__ out, int B, int n, int d) {
    extern __shared__ __attribute__((aligned(16))) float s_x[];   // 16 x d
    const int tid = threadIdx.x, k = blockIdx.x * 256 + tid, b0 = blockIdx.y * 16, nb = min(16, B - b0);
    for (int e = tid; e < 16 * d; e += 256) s_x[e] = (e / d) < nb ? x[(size_t)b0 * d + e] : 0.f;
    __syncthreads();
    if (k >= n) return;
    const float* cen = c + (size_t)k * d;
    const bool v4 = (d & 3) == 0 && (((size_t)c) & 15) == 0;
    float d2[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) d2[b] = 0.f;
    for (int c0 = 0; c0 < d; c0 += 8) {
        float cv[8];
        if (v4) {
            const float4 ca = *reinterpret_cast<const float4*>(cen + c0);
            const float4 cb = c0 + 4 < d ? *reinterpret_cast<const float4*>(cen + c0 + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            cv[0] = ca.x; cv[1] = ca.y; cv[2] = ca.z; cv[3] = ca.w; cv[4] = cb.x; cv[5] = cb.y; cv[6] = cb.z; cv[7] = cb.w;
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const float4 x0 = *reinterpret_cast<const float4*>(&s_x[b * d + c0]);
                float t;
                t = x0.x - cv[0]; d2[b] = fmaf(t, t, d2[b]); t = x0.y - cv[1]; d2[b] = fmaf(t, t, d2[b]);
                t = x0.z - cv[2]; d2[b] = fmaf(t, t, d2[b]); t = x0.w - cv[3]; d2[b] = fmaf(t, t, d2[b]);
                if (c0 + 4 < d) {
                    const float4 x1 = *reinterpret_cast<const float4*>(&s_x[b * d + c0 + 4]);
                    t = x1.x - cv[4]; d2[b] = fmaf(t, t, d2[b]); t = x1.y - cv[5]; d2[b] = fmaf(t, t, d2[b]);
                    t = x1.z - cv[6]; d2[b] = fmaf(t, t, d2[b]); t = x1.w - cv[7]; d2[b] = fmaf(t, t, d2[b]);
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) cv[q] = c0 + q < d ? cen[c0 + q] : 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (c0 + q < d) {
#pragma unroll
                    for (int b = 0; b < 16; ++b) { const float t = s_x[b * d + c0 + q] - cv[q]; d2[b] = fmaf(t, t, d2[b]); }
                }
        }
    }
    const float w = expf(logw[k]);
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if (b < nb) out[(size_t)(b0 + b) * n + k] = expf(-0.5f * d2[b] / (w * w));
}

// Scalar losses: VJF_LOSS_BLOCKS workgroups, fp64 accumulation, fixed order (every workgroup sums a fixed share of the elements,
// the last one to finish adds the partial sums in workgroup order: the result does not depend on timing).
//   mode 0: gaussian_loss (functional.py:32-75)  mode 1: gaussian_entropy (:25-29)  mode 2: poisson (likelihood.py:51-62)
// The partial sums live in a small device-resident table of VJF_LOSS_SLOTS slots handed out in turn by the host: up to that
// many loss calls may be in flight at once (on any streams).
#define VJF_LOSS_BLOCKS 64
#define VJF_LOSS_SLOTS 32
__device__ double vjf_loss_part[VJF_LOSS_SLOTS][VJF_LOSS_BLOCKS];
__device__ unsigned vjf_loss_count[VJF_LOSS_SLOTS];
__global__ __launch_bounds__(256) void vjf_loss_kernel(int mode, const float* m1, const float* lv1, const float* m2, const float* lv2,
                                                       const float* logvar, float* out, int B, int d, int slot) {
    __shared__ double s_p[4];
    __shared__ int s_last;
    double acc = 0.0;
    const size_t N = (size_t)B * d;
    const float lvr = (mode == 0) ? logvar[0] : 0.f;
    const float p = expf(-0.5f * lvr);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)VJF_LOSS_BLOCKS * 256) {
        float t;
        if (mode == 0) {
            t = vjf_gauss_nll(m1[i], m2[i], p, lvr);
            if (lv1 || lv2) t += 0.5f * expf((lv1 ? lv1[i] : 0.f) + (lv2 ? lv2[i] : 0.f) - lvr);    // (the trace, where either side has a variance)
        } else if (mode == 1) {
            t = vjf_entropy_term(m1[i]);
        } else {
            const float eta = vjf_poisson_eta(m1[i]);
            t = vjf_poisson_nll(m2[i], eta, expf(eta));
        }
        acc += (double)t;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(&vjf_loss_part[slot][blockIdx.x], ((s_p[0] + s_p[1]) + s_p[2]) + s_p[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (release: the partial sum is visible at agent scope before the count)
        const unsigned done = __hip_atomic_fetch_add(&vjf_loss_count[slot], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = done == VJF_LOSS_BLOCKS - 1;
    }
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x < 64) {                                    // the last workgroup: 64 partial sums, fixed xor tree
        double t = __hip_atomic_load(&vjf_loss_part[slot][threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        if (threadIdx.x == 0) { out[0] = (float)(t / (double)B); __hip_atomic_store(&vjf_loss_count[slot], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    }
}

// p[0..n) *= f   (test hook of the sharded route: a one-rank communicator standing in for f identical ranks)
__global__ void vjf_scale_kernel(float* p, float f, int n) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) p[e] *= f;
}

namespace {   // (internal linkage from here on, as the forecast and recognition kernels have: their symbols carry it)
struct VjfPredArgs {
    const float* x; const float* c; const float* logw; const float* w_mean; const float* w_chol;
    float* mean; float* logvar; int B, n, d, dout;
};
// 16 trials per workgroup: features feature-major in LDS ([feature][17], as the fused kernels hold them), then Phi W (mean)
// and the row norm of Phi w_chol (logvar) as 16 x 16 output tiles on v_mfma_f32_16x16x4_f32 (mma_tile: the matrices are k-major
// for these products), one tile per wavefront and round.
__global__ __launch_bounds__(VJF_K1_THREADS) void vjf_blr_predict_kernel(VjfPredArgs A) {
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_K1_THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_phi = smem;                 // n x LD
    float* s_red = s_phi + A.n * LD;     // NW x TB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b0 = blockIdx.x * TB, nb = min(TB, A.B - b0);
    for (int i = tid; i < TB * A.n; i += VJF_K1_THREADS) {
        const int k = i / TB, b = i - k * TB;
        float ph = 0.f;
        if (b < nb) {
            float d2 = 0.f;
            for (int j = 0; j < A.d; ++j) { const float t = A.x[(size_t)(b0 + b) * A.d + j] - A.c[(size_t)k * A.d + j]; d2 = fmaf(t, t, d2); }
            const float w = expf(A.logw[k]);
            ph = expf(-0.5f * d2 / (w * w));
        }
        s_phi[k * LD + b] = ph;
    }
    __syncthreads();
    const int col = lane & 15, r4 = 4 * (lane >> 4);     // accumulator: row = r4 + r (output), column = trial
    if (A.mean)
        for (int t = wave; t * 16 < A.dout; t += NW) {
            vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            mma_tile(acc, A.w_mean, A.dout, A.dout, t * 16, s_phi, A.n, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = t * 16 + r4 + r;
                if (j < A.dout && col < nb) A.mean[(size_t)(b0 + col) * A.dout + j] = acc[r];
            }
        }
    if (!A.logvar) return;
    float v2 = 0.f;                                      // this lane's share of sum_j Z[trial col][j]^2
    for (int t = wave; t * 16 < A.n; t += NW) {
        vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        mma_tile(acc, A.w_chol, A.n, A.n, t * 16, s_phi, A.n, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) v2 = fmaf(acc[r], acc[r], v2);      // (rows beyond n are exact zeros)
    }
    v2 += __shfl_xor(v2, 16, 64);                        // the four row groups of a column, fixed order
    v2 += __shfl_xor(v2, 32, 64);
    if (lane < 16) s_red[wave * TB + lane] = v2;
    __syncthreads();
    for (int i = tid; i < nb * A.dout; i += VJF_K1_THREADS) {
        const int b = i / A.dout;
        float v = s_red[b];
        for (int w = 1; w < NW; ++w) v += s_red[w * TB + b];
        A.logvar[(size_t)(b0 + b) * A.dout + (i - b * A.dout)] = logf(v);
    }
}

// features + target rows of the stand-alone RLS:  E[b] = [Phi(x_b) | target_b | 0]
__global__ void vjf_rls_rows_kernel(const float* x, const float* c, const float* logw, const float* target, float* E,
                                    int B, int n, int d, int dout, int ldE) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * ldE) return;
    const int b = (int)(i / ldE), k = (int)(i - (size_t)b * ldE);
    float v = 0.f;
    if (k < n) {
        float d2 = 0.f;
        for (int j = 0; j < d; ++j) { const float t = x[(size_t)b * d + j] - c[(size_t)k * d + j]; d2 = fmaf(t, t, d2); }
        const float w = expf(logw[k]);
        v = expf(-0.5f * d2 / (w * w));
    } else if (k < n + dout) {
        v = target[(size_t)b * dout + (k - n)];
    }
    E[i] = v;
}

}  // namespace

// Recognition.forward for 16 trials per workgroup: activations feature-major in LDS (ping-pong), every layer as 16 x 16 output
// tiles on v_mfma_f32_16x16x4_f32 with the weights read as torch stores them (mma_tile<true>).
#define VJF_RECOGNITION_ACT 0
#include "vjf_recognition_kernel.h"     // vjf_recognition_kernel
#undef VJF_RECOGNITION_ACT
#define VJF_RECOGNITION_ACT 1
#include "vjf_recognition_kernel.h"     // vjf_recognition_act_kernel
#undef VJF_RECOGNITION_ACT
