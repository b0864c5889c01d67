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
#include "vjf_trial_mfma_kernel.h"   // mma_tile, vjf_f32x4, VJF_LDT

#define VJF_FC_THREADS 256
#define VJF_FC_WAVES (VJF_FC_THREADS / 64)
#define VJF_FC_KQ 16                 // MFMA steps of one wavefront's share of K that the look-ahead keeps in registers (n <= 256)

namespace {
struct VjfFcWeightArgs {
    const float* w_mean; const float* w_chol; const float* noise;   // (n, dout), (n, n) dense, (Tc, n, dout)
    float* W;                                                       // (Tc, n, dout)
    int Tc, n, dout;
};

// Workgroup (m, s): rows 16 m .. 16 m + 15 of every W[t] with t = 4 s + wave (mod 4 gridDim.y).  The 16 rows of w_chol sit in LDS
// k-major ([k][VJF_LDT]) and are the MFMA's B operand; the noise of step t is the A operand, read as it lies in memory:
//   acc(row j, col i) = sum_k noise[t][k][j0 + j] * w_chol[16 m + i][k] = (w_chol @ noise[t])[16 m + i][j0 + j]
// One wavefront computes one W[t] tile with one accumulator over k = 0 .. n - 1 in mma_tile's order, whatever chunk, grid or
// workgroup the step falls into: the bits of W[t] depend on t's inputs alone.
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_fc_weights_kernel(VjfFcWeightArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_a = smem;                                   // n x LD
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m0 = blockIdx.x * 16, n = A.n, dout = A.dout;
    for (int e = tid; e < 16 * n; e += VJF_FC_THREADS) {
        const int i = e / n, k = e - i * n;              // (consecutive lanes: consecutive k of one row)
        s_a[k * VJF_LDT + i] = (m0 + i) < n ? A.w_chol[(size_t)(m0 + i) * n + k] : 0.f;
    }
    __syncthreads();
    const int col = lane & 15, r4 = 4 * (lane >> 4);
    for (int t = blockIdx.y * VJF_FC_WAVES + wave; t < A.Tc; t += gridDim.y * VJF_FC_WAVES) {
        const float* nz = A.noise + (size_t)t * n * dout;
        float* Wt = A.W + (size_t)t * n * dout;
#include "vjf_fc_sample_body.h"         // rows m0 .. m0 + 15 of Wt = w_mean + w_chol @ nz (shared with vjf_fe_weights_kernel)
    }
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

static inline size_t vjf_fc_lds_floats(int n, int d, int dout, bool cen_lds) {
    const size_t doutp = ((size_t)dout + 15) / 16 * 16;
    return (size_t)n * VJF_LDT + (size_t)d * VJF_LDT + (size_t)VJF_FC_WAVES * doutp * VJF_LDT + (size_t)n + (cen_lds ? (size_t)n * d : 0);
}

// this wavefront's share of K: a multiple of 4 features per wavefront, the last one takes what is left
__device__ __forceinline__ void fc_k_range(int n, int wave, int& kb, int& ke) {
    const int per = ((n + VJF_FC_WAVES - 1) / VJF_FC_WAVES + 3) & ~3;
    kb = min(wave * per, n);
    ke = min(kb + per, n);
}

// NT > 0: the look-ahead form for dout <= 16 NT and n <= 64 VJF_FC_KQ -- the A operands (this lane's elements of W[t + 1]) are
//         loaded into registers right behind step t's MFMAs and are in flight during step t's reduction and step t + 1's features.
// NT == 0: any shape; W[t] is read by mma_tile when it is used (from L2: vjf_fc_weights_kernel has just written it).
// Both issue the same MFMA steps on the same operands in the same order, so they compute the same bits.
// CL: centroids in LDS (else read from global memory every step).
template <int NT, bool CL>
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_fc_rollout_kernel(VjfFcArgs A) {
#include "vjf_fc_rollout_body.h"        // the step loop on `A` (shared with vjf_fe_rollout_kernel)
}
}  // namespace
