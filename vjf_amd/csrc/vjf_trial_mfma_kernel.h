// vjf_trial_mfma_kernel.h -- K1 on the f32 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32).
//
// Same contract as vjf_trial_kernel (see vjf_trial_kernel.h for the reference citations); this
// version is used when 16 trials' working set fits LDS.  One workgroup = 4 wavefronts = 16 trials.
// Every dense product is evaluated transposed, out^T (features x 16 trials) = A (features x K) *
// X^T (K x 16 trials), so that
//   * the trial index sits on the MFMA column (lane & 15): per-trial reductions stay inside a lane,
//   * the B operand is the LDS-resident activation matrix, stored feature-major [feature][17]
//     (17 = 16 trials + 1 pad word: operand reads and transposed copies are bank-conflict free),
//   * the A operand comes straight from L2 in "k-major" matrices (row k contiguous over features),
//     64-byte segments per k: w_chol, w_mean and the backward weights already have that layout,
//     the forward weights are read from their transposed copies in the aux buffer.
// w_chol is upper triangular (module.py:102), so variance tile j0 only runs k <= j0 + 15.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_handoff.h"
#include "vjf_plan.h"
#include "vjf_trial_kernel.h"      // VjfTrialArgs, group_sum
#include "vjf_act.h"

#define VJF_LDT 17
#define VJF_K1M_WAVES 16           // wavefronts per workgroup (two per SIMD: one hides the other's L2 operand latency)
#define VJF_K1M_THREADS (64 * VJF_K1M_WAVES)
typedef float vjf_f32x4 __attribute__((ext_vector_type(4)));

// acc(row = 4*(lane>>4)+r, col = lane&15) += sum_{k<K} Ag[k*lda + m0 + row] * Xs[k*17 + col]
// rows m0+i >= M contribute 0.
// (NT: the matrix as torch stores a Linear weight, A[m][k] = Ag[m * lda + k], instead of k-major -- the stand-alone operators)
template <bool NT = false>
__device__ __forceinline__ void mma_tile(vjf_f32x4& acc, const float* __restrict__ Ag, int lda_, int M, int m0,
                                         const float* Xs, int K, int lane) {
    const int i = lane & 15, kk = lane >> 4;
    const bool rv = (m0 + i) < M;
    const size_t lda = NT ? 1 : (size_t)lda_;            // distance of two k
    // (rows beyond M: read from a valid address and masked where the value is USED -- a select right behind a load makes the
    //  compiler wait for the load there, and the next batch would not be in flight beside this batch's MFMAs)
    const float* ap = Ag + (size_t)(rv ? m0 + i : 0) * (NT ? (size_t)lda_ : 1) + (size_t)kk * lda;
    const float* xp = Xs + kk * VJF_LDT + i;
    const int K32 = K & ~31;
    int k0 = 0;
    if (K32 > 0) {                                     // batches of 8 steps, the next batch's 16 operand loads in flight
        float a0[8], x0[8], a1[8], x1[8];              // while the current batch's MFMAs issue
#pragma unroll
        for (int q = 0; q < 8; ++q) { a0[q] = ap[(size_t)(4 * q) * lda]; x0[q] = xp[(4 * q) * VJF_LDT]; }
        for (; k0 < K32; k0 += 64) {
            const bool more1 = k0 + 32 < K32;
            if (more1) {
#pragma unroll
                for (int q = 0; q < 8; ++q) { a1[q] = ap[(size_t)(k0 + 32 + 4 * q) * lda]; x1[q] = xp[(k0 + 32 + 4 * q) * VJF_LDT]; }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(rv ? a0[q] : 0.f, x0[q], acc, 0, 0, 0);
            if (!more1) { k0 += 32; break; }
            const bool more0 = k0 + 64 < K32;
            if (more0) {
#pragma unroll
                for (int q = 0; q < 8; ++q) { a0[q] = ap[(size_t)(k0 + 64 + 4 * q) * lda]; x0[q] = xp[(k0 + 64 + 4 * q) * VJF_LDT]; }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(rv ? a1[q] : 0.f, x1[q], acc, 0, 0, 0);
            if (!more0) { k0 += 64; break; }
        }
    }
    // remainder (< 32 rows): its up to 8 steps' operands in flight together (clamped addresses, masked at use), then the same
    // MFMA steps in the same order as a step-by-step loop would issue them
    if (k0 < K) {
        const float* apc = ap;                                          // (rows beyond M: a valid address, masked below)
        float ar[8], xr[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = k0 + 4 * q + kk;
            const bool kv = k < K;
            const float av = apc[(size_t)(kv ? k0 + 4 * q : 0) * lda], xv = xp[(kv ? k0 + 4 * q : 0) * VJF_LDT];
            ar[q] = (rv && kv) ? av : 0.f;
            xr[q] = kv ? xv : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (k0 + 4 * q < K) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[q], xr[q], acc, 0, 0, 0);   // (uniform)
    }
}

struct VjfTrialMfmaArgs {
    VjfTrialArgs t;
    const float* aux;      // transposed weights (VjfPlan::aux_*)
    unsigned long long* stamps;   // diagnostic only (null in normal runs)
    unsigned* done;        // += 1 per workgroup once it has read W, w_chol, sigma for the last time (null: not counted):
                           //   the post kernel, on another stream, waits for the count before it overwrites them
    unsigned* fwd_done;    // forward half: += 1 per workgroup once its E / ACT rows and posterior are written back to memory
                           //   (release at agent scope): the statistics Gram on another stream starts behind vjf_gate_kernel on it
    const unsigned* rls_done;  // backward half: workgroups of the previous step's post kernel that have their W, w_chol, sigma in
    unsigned rls_target;       //   memory; non-null -> the workgroup waits (bounded) for the count before stage 2, its reloads done
    int part;              // 0: whole step; 1: forward half (features, recognition, E / ACT rows, posterior);
                           // 2: backward half (predictive mean / variance, losses, backward, DEL rows) -- reloads the
                           //    forward half's rows, so that it can run after the RLS update of the previous step while
                           //    the forward half of this step ran beside it (vjf_filter_seq, two streams)
};

#define VJF_K1_STAMP(i)                                                                     \
    do {                                                                                    \
        if (AA.stamps && blockIdx.x == 0 && threadIdx.x == 0) {                             \
            unsigned long long t_;                                                          \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");      \
            AA.stamps[i] = t_;                                                              \
        }                                                                                   \
    } while (0)

static inline size_t vjf_trial_mfma_lds_floats(const VjfPlan& P) {
    // Wide observations (dy >= hmax): the first delta buffer lives in the (by then dead) decoder-mean rows and the
    // second one exists only for networks with more than one hidden layer -- two workgroups per CU at dy = 200.
    const bool compact = P.dy >= P.hmax;
    const size_t nd = compact ? (P.L > 1 ? 1 : 0) : 2;
    const size_t feat = (size_t)P.din + P.dxu + P.n + P.hsum + nd * (size_t)P.hmax + 8 * (size_t)P.dz + 2 * (size_t)P.dy;
    return feat * VJF_LDT + 16 * RS_N + VJF_K1M_WAVES * 16 + 16 + 64;
}

// a hidden layer's activation and its derivative from the layer's output: Tanh without the trailing argument
__device__ __forceinline__ float vjf_k1m_fwd(float x) { return tanhf(x); }
__device__ __forceinline__ float vjf_k1m_fwd(float x, const VjfAct& act) { return vjf_act_fwd(act, x); }
__device__ __forceinline__ float vjf_k1m_dh(float hv) { return 1.f - hv * hv; }
__device__ __forceinline__ float vjf_k1m_dh(float hv, const VjfAct& act) { return vjf_act_dh(act, hv); }
#include "vjf_trial_mfma_body.h"      // vjf_trial_mfma_kernel<>, vjf_trial_mfma_kernel<VjfAct>

// Refresh the transposed weight copies from the canonical tensors (run at the start of an API call:
// the caller may have written the state blob; within a sequence vjf_prep_kernel keeps them in step).
__global__ void vjf_aux_kernel(VjfPlan P, const float* state, float* aux) {
    for (int t = 0; t < P.n_train; ++t) {
        if (P.tr_aux[t] < 0) continue;
        const int rows = P.tr_rows[t], cols = P.tr_cols[t];
        for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < rows * cols; e += gridDim.x * blockDim.x) {
            const int r = e / cols, c = e - r * cols;
            aux[P.tr_aux[t] + (size_t)c * P.tr_auxld[t] + P.tr_auxcol[t] + r] = state[P.tr_off[t] + e];
        }
    }
}
