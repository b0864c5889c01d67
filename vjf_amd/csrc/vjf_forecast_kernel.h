// vjf_forecast_kernel.h -- the sampled roll-out of RBFDS.forecast (vjf/model.py:342-361) as two kernels per chunk of steps:
//
//   vjf_fc_weights_kernel   W[t] = w_mean + w_chol @ w_noise[t]  (vjf/module.py:70-73) for every step of the chunk.  The weight
//                           samples do not depend on x, so all of them are ready before the sequential part begins.
//   vjf_fc_rollout_kernel   one workgroup per tile of 16 trials loops over the steps of the chunk inside the kernel:
//                           features of [x_t, u_t] -> Phi W[t] -> x_{t+1} = x_t + Phi W[t] (+ e_t sigma) -> store.
//
// Both follow vjf_blr_predict_kernel's tiling: activations feature-major in LDS ([feature][VJF_LDT]), products as 16 x 16 tiles on
// v_mfma_f32_16x16x4_f32 with the trial on the MFMA column.  Workgroups are independent: no cooperative launch, no hand-off.
// Included from vjf_abi.hip behind vjf_blr_predict_kernel (mma_tile, VJF_LDT, VJF_K1_THREADS).
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_trial_mfma_kernel.h"   // mma_tile, vjf_f32x4, VJF_LDT

#define VJF_FC_THREADS 256
#define VJF_FC_WAVES (VJF_FC_THREADS / 64)
#define VJF_FC_KQ 16                 // MFMA steps of one wavefront's share of K that the look-ahead keeps in registers (n <= 256)

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
        for (int j0 = 0; j0 < dout; j0 += 16) {
            vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            mma_tile(acc, nz, dout, dout, j0, s_a, n, lane);
            if (m0 + col < n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = j0 + r4 + r;
                    if (j < dout) Wt[(size_t)(m0 + col) * dout + j] = A.w_mean[(size_t)(m0 + col) * dout + j] + acc[r];
                }
            }
        }
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
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_FC_WAVES, NTH = VJF_FC_THREADS, KQ = VJF_FC_KQ;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = A.n, d = A.d, dout = A.dout, du = d - dout, doutp = (dout + 15) / 16 * 16;
    float* s_phi = smem;                          // n x LD       features of step t
    float* s_x = s_phi + n * LD;                  // d x LD       [x_t, u_t]
    float* s_part = s_x + d * LD;                 // NW x doutp x LD   the wavefronts' partial products
    float* s_w2 = s_part + NW * doutp * LD;       // n            width^2
    float* s_c = s_w2 + n;                        // n x d        centroids (CL)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b0 = blockIdx.x * TB, nb = min(TB, A.B - b0);
    const size_t row0 = (size_t)b0 * dout;        // the tile's rows in a (B, dout) array are contiguous
    const size_t sx = (size_t)A.B * dout, su = (size_t)A.B * du, sw = (size_t)n * dout;

    for (int k = tid; k < n; k += NTH) { const float w = expf(A.logw[k]); s_w2[k] = w * w; }
    if (CL) for (int i = tid; i < n * d; i += NTH) s_c[i] = A.c[i];
    for (int i = tid; i < TB * dout; i += NTH) {
        const int b = i / dout, j = i - b * dout;
        float v = 0.f;
        if (b < nb) {
            v = A.x_in[row0 + i];
            if (A.x0_out) A.x0_out[row0 + i] = v;
        }
        s_x[j * LD + b] = v;
    }
    for (int i = tid; i < TB * du; i += NTH) {
        const int b = i / du, j = i - b * du;
        s_x[(dout + j) * LD + b] = b < nb ? A.u[(size_t)b0 * du + i] : 0.f;
    }
    const float sigma = A.e ? expf(0.5f * A.tr_logvar[0]) : 0.f;
    int kb, ke;
    fc_k_range(n, wave, kb, ke);
    const int mi = lane & 15, kk = lane >> 4, r4 = 4 * (lane >> 4);
    constexpr int NTR = NT > 0 ? NT : 1;
    float aw[NTR][KQ];                                    // (NT > 0) this lane's A operands of the coming step
    auto fetch_w = [&](const float* Wt) {
#pragma unroll
        for (int t = 0; t < NTR; ++t)
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                const int k = kb + 4 * q + kk, j = t * 16 + mi;
                const bool ok = k < ke && j < dout;       // (masked where the value is used: the loads stay in flight)
                aw[t][q] = Wt[ok ? (size_t)k * dout + j : 0];
            }
    };
    if (NT > 0) fetch_w(A.W);
    __syncthreads();

    for (int t = 0; t < A.Tc; ++t) {
        // this step's noise and the next step's control input: in flight while the features are computed
        float e0 = 0.f, u0 = 0.f;
        if (A.e && tid < nb * dout) e0 = A.e[(size_t)t * sx + row0 + tid];
        if (du > 0 && t + 1 < A.Tc && tid < nb * du) u0 = A.u[(size_t)(t + 1) * su + (size_t)b0 * du + tid];

        // features: exp(-1/2 |xu - c|^2 / width^2), the squared distance as a sum of squared differences
        for (int i = tid; i < TB * n; i += NTH) {
            const int k = i / TB, b = i - k * TB;
            float ph = 0.f;
            if (b < nb) {
                float d2 = 0.f;
                for (int j = 0; j < d; ++j) { const float df = s_x[j * LD + b] - (CL ? s_c[k * d + j] : A.c[(size_t)k * d + j]); d2 = fmaf(df, df, d2); }
                ph = expf(-0.5f * d2 / s_w2[k]);
            }
            s_phi[k * LD + b] = ph;
        }
        __syncthreads();

        // Phi W[t], K split over the four wavefronts: partial(row j, col trial) of features kb .. ke - 1
        const float* Wt = A.W + (size_t)t * sw;
        if (NT > 0) {
#pragma unroll
            for (int tl = 0; tl < NTR; ++tl) {
                vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                const bool rv = tl * 16 + mi < dout;
#pragma unroll
                for (int q = 0; q < KQ; ++q) {
                    const int k0 = kb + 4 * q;
                    if (k0 < ke) {                                       // (uniform over the wavefront)
                        const bool kv = k0 + kk < ke;
                        const float xv = s_phi[(kv ? k0 + kk : kb) * LD + mi];
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((rv && kv) ? aw[tl][q] : 0.f, kv ? xv : 0.f, acc, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) s_part[(wave * doutp + tl * 16 + r4 + r) * LD + mi] = acc[r];
            }
            if (t + 1 < A.Tc) fetch_w(Wt + sw);                          // W[t + 1]: used behind the next step's features
        } else {
            for (int j0 = 0; j0 < dout; j0 += 16) {
                vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                if (kb < ke) mma_tile(acc, Wt + (size_t)kb * dout, dout, dout, j0, s_phi + kb * LD, ke - kb, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) s_part[(wave * doutp + j0 + r4 + r) * LD + mi] = acc[r];
            }
        }
        __syncthreads();

        // x_{t+1} = x_t + (p0 + p1 + p2 + p3) (+ e_t sigma): the four partials in a fixed order, the noise term rounded on its
        // own as the step-by-step path rounds it
        float* xo = A.x_out + (size_t)t * sx + row0;
        for (int i = tid; i < nb * dout; i += NTH) {
            const int b = i / dout, j = i - b * dout;
            float v = s_part[j * LD + b];
#pragma unroll
            for (int w = 1; w < NW; ++w) v += s_part[(w * doutp + j) * LD + b];
            v = s_x[j * LD + b] + v;
            if (A.e) v = __fadd_rn(v, __fmul_rn(i == tid ? e0 : A.e[(size_t)t * sx + row0 + i], sigma));
            s_x[j * LD + b] = v;
            xo[i] = v;
        }
        if (du > 0 && t + 1 < A.Tc)
            for (int i = tid; i < nb * du; i += NTH) {
                const int b = i / du, j = i - b * du;
                s_x[(dout + j) * LD + b] = i == tid ? u0 : A.u[(size_t)(t + 1) * su + (size_t)b0 * du + i];
            }
        __syncthreads();
    }
}
