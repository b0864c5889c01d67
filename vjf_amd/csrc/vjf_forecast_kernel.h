// vjf_forecast_kernel.h -- the sampled roll-out of RBFDS.forecast (vjf/model.py:342-361) as two kernels per chunk of steps:
//
//   vjf_fc_weights_kernel   W[t] = w_mean + w_chol @ w_noise[t]  (vjf/module.py:70-73) for every step of the chunk.  The weight
//                           samples do not depend on x, so all of them are ready before the sequential part begins.
//   vjf_fc_rollout_kernel   one workgroup per tile of 16 trials loops over the steps of the chunk inside the kernel:
//                           features of [x_t, u_t] -> Phi W[t] -> x_{t+1} = x_t + Phi W[t] (+ e_t sigma) -> store.
//
// Both follow vjf_blr_predict_kernel's tiling: activations feature-major in LDS ([feature][VJF_LDT]), products as 16 x 16 tiles on
// v_mfma_f32_16x16x4_f32 with the trial on the MFMA column.  Workgroups are independent: no cooperative launch, no hand-off.
// Included by vjf_host_forecast.h.  The kernels sit in an anonymous namespace: their symbols carry it.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_rollout_step.h"       // the x step and its forms, VJF_FC_*, vjf_fc_lds_floats; mma_tile, vjf_f32x4, VJF_LDT

namespace {
struct VjfFcWeightArgs {
    const float* w_mean; const float* w_chol; const float* noise;   // (n, dout), (n, n) dense, (Tc, n, dout)
    float* W;                                                       // (Tc, n, dout)
    int Tc, n, dout;
};

// The 16 rows m0 .. m0 + 15 of w_chol into LDS k-major ([k][VJF_LDT]): the B operand of every sample of the workgroup
__device__ __forceinline__ void fc_stage_chol(float* s_a, const float* w_chol, int m0, int n) {
    for (int e = threadIdx.x; e < 16 * n; e += VJF_FC_THREADS) {
        const int i = e / n, k = e - i * n;              // (consecutive lanes: consecutive k of one row)
        s_a[k * VJF_LDT + i] = (m0 + i) < n ? w_chol[(size_t)(m0 + i) * n + k] : 0.f;
    }
}
// Columns j0 .. j0 + 15 of one weight sample: rows m0 .. m0 + 15 of Wt = w_mean + w_chol @ nz.  The noise is the MFMA's A operand, read as it lies in memory:
//   acc(row j, col i) = sum_k nz[k][j0 + j] * w_chol[m0 + i][k] = (w_chol @ nz)[m0 + i][j0 + j]
// One wavefront, one accumulator over k = 0 .. n - 1 in mma_tile's order, whatever chunk, grid or workgroup the sample falls into: the
// bits of W[t] depend on t's inputs alone, for both weights kernels.  (The loop over j0 is the caller's: see fc_product_padded.)
__device__ __forceinline__ void fc_sample(const float* nz, float* Wt, const float* w_mean, const float* s_a, int m0, int n, int dout, int j0, int lane) {
    const int col = lane & 15, r4 = 4 * (lane >> 4);
    vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    mma_tile(acc, nz, dout, dout, j0, s_a, n, lane);
    if (m0 + col < n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + r4 + r;
            if (j < dout) Wt[(size_t)(m0 + col) * dout + j] = w_mean[(size_t)(m0 + col) * dout + j] + acc[r];
        }
    }
}

// Workgroup (m, s): rows 16 m .. 16 m + 15 of every W[t] with t = 4 s + wave (mod 4 gridDim.y).
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_fc_weights_kernel(VjfFcWeightArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m0 = blockIdx.x * 16, n = A.n, dout = A.dout;
    fc_stage_chol(smem, A.w_chol, m0, n);
    __syncthreads();
    for (int t = blockIdx.y * VJF_FC_WAVES + wave; t < A.Tc; t += gridDim.y * VJF_FC_WAVES)
        for (int j0 = 0; j0 < dout; j0 += 16)
            fc_sample(A.noise + (size_t)t * n * dout, A.W + (size_t)t * n * dout, A.w_mean, smem, m0, n, dout, j0, lane);
}

struct VjfFcArgs {
    const float* x_in;       // (B, dout): the state the chunk starts from (x0, or x[t0] of the previous chunk)
    const float* u;          // (Tc, B, du) or null
    const float* e;          // (Tc, B, dout) state noise or null
    const float* c; const float* logw;     // centroids (n, d), log widths (n)
    const float* W;          // (Tc, n, dout) weight samples of the chunk
    const float* tr_logvar;  // device scalar (read when e is given)
    float* x0_out;           // (B, dout) or null: where x_in is copied to (the first chunk writes x[0])
    float* x_out;            // (Tc, B, dout): x[t0 + 1 .. t0 + Tc]
    int Tc, B, n, d, dout;
};

// The roll-out of one tile of trials over a chunk's steps, for vjf_fc_rollout_kernel and vjf_fe_rollout_kernel (a member: the same bits).
// NT > 0: the look-ahead form for dout <= 16 NT and n <= VJF_FC_REG_N = 4 VJF_FC_WAVES VJF_FC_KQ (vjf_fc_reg_form) -- the A operands (this
//         lane's elements of W[t + 1]) are loaded right behind step t's MFMAs, in flight during its reduction and step t + 1's features.
// NT == 0: any shape; W[t] is read by mma_tile when it is used (fc_product_padded; from L2: vjf_fc_weights_kernel has just written it).
// Both issue the same MFMA steps on the same operands in the same order: the same bits.  CL: centroids in LDS (else global memory).
template <int NT, bool CL>
__device__ __forceinline__ void fc_rollout(VjfFcArgs A) {       // (by value: by reference vjf_fe_rollout_kernel<0, *> takes 11 VGPRs more)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const FcTile S = fc_tile(smem, A.n, A.d, A.dout, A.B);
    const size_t row0 = (size_t)S.b0 * S.dout, sx = (size_t)A.B * S.dout, su = (size_t)A.B * S.du, sw = (size_t)S.n * S.dout;
    fc_stage<CL, false>(S, A.logw, A.c, nullptr, A.x_in, A.x0_out, A.u);
    const float sigma = A.e ? expf(0.5f * A.tr_logvar[0]) : 0.f;
    float aw[NT > 0 ? NT : 1][VJF_FC_KQ];                // (NT > 0) this lane's A operands of the coming step
    if constexpr (NT > 0) fc_fetch_w(S, A.W, aw);
    __syncthreads();

    for (int t = 0; t < A.Tc; ++t) {
        // this step's noise and the next step's control input: in flight while the features are computed
        const float* un = S.du > 0 && t + 1 < A.Tc ? A.u + (size_t)(t + 1) * su + (size_t)S.b0 * S.du : nullptr;
        const float e0 = A.e && S.tid < S.nb * S.dout ? A.e[(size_t)t * sx + row0 + S.tid] : 0.f;
        const float u0 = fc_u_ahead(S, un);
        fc_features<CL>(S, A.c);
        __syncthreads();

        const float* Wt = A.W + (size_t)t * sw;
        if constexpr (NT > 0) {
            fc_product_reg(S, aw);
            if (t + 1 < A.Tc) fc_fetch_w(S, Wt + sw, aw);            // W[t + 1]: used behind the next step's features
        } else {
            for (int j0 = 0; j0 < S.dout; j0 += 16) fc_product_padded(S, Wt, j0);
        }
        __syncthreads();

        // (+ e_t sigma): the noise term rounded on its own as the step-by-step path rounds it
        float* xo = A.x_out + (size_t)t * sx + row0;
        fc_advance(S, [&](int i, float v) {
            if (A.e) v = __fadd_rn(v, __fmul_rn(i == S.tid ? e0 : A.e[(size_t)t * sx + row0 + i], sigma));
            xo[i] = v;
            return v;
        });
        fc_u_advance(S, un, u0);
        __syncthreads();
    }
}

template <int NT, bool CL>
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_fc_rollout_kernel(VjfFcArgs A) { fc_rollout<NT, CL>(A); }
}  // namespace
