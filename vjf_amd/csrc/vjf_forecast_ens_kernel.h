// vjf_forecast_ens_kernel.h -- an ensemble of S sampled roll-outs of RBFDS.forecast (vjf/model.py:342-361, one draw of the
// predictive distribution each) and their per-step mean and variance, as three kernels per chunk of members x steps:
//
//   vjf_fe_weights_kernel   W[s][t] = w_mean + w_chol @ w_noise[s][t]  (vjf/module.py:70-73) for every member and step of the chunk:
//                           vjf_fc_weights_kernel's sample (fc_sample), the member on the flattened sample index.
//   vjf_fe_rollout_kernel   one workgroup per (tile of 16 trials, member): vjf_fc_rollout_kernel's body on the member's W, noise and start.
//   vjf_fe_moments_kernel   one workgroup per (tile of 16 trials, step, group of 8 output tiles): walks the chunk's members in member
//                           order, decodes y = x C^T + b on chip (vjf/model.py:321-324) and folds x and y into running (mean, M2).
//
// Tiling as in vjf_forecast_kernel.h: activations feature-major in LDS ([feature][VJF_LDT]), the trial on the MFMA column of
// v_mfma_f32_16x16x4_f32.  Workgroups are independent: no cooperative launch, no hand-off, no atomics.
// Included by vjf_host_forecast.h.  The kernels sit in an anonymous namespace: their symbols carry it.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_forecast_kernel.h"     // VjfFcArgs, fc_rollout, fc_sample, VJF_FC_*

namespace {
struct VjfFeWeightArgs {
    const float* w_mean; const float* w_chol;
    const float* noise;        // member sl, step t of the chunk at noise + sl * noise_ms + t * n * dout
    float* W;                  // (Sc, Tc, n, dout)
    size_t noise_ms;
    int Sc, Tc, n, dout;
};

// Workgroup (m, g): rows 16 m .. 16 m + 15 of the samples q = sl Tc + t with q = 4 g + wave (mod 4 gridDim.y).  One wavefront, one
// accumulator, k ascending per sample (fc_sample): the bits of W[s][t] depend on that sample's inputs alone.
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_fe_weights_kernel(VjfFeWeightArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m0 = blockIdx.x * 16, n = A.n, dout = A.dout, nq = A.Sc * A.Tc;
    fc_stage_chol(smem, A.w_chol, m0, n);
    __syncthreads();
    for (int q = blockIdx.y * VJF_FC_WAVES + wave; q < nq; q += gridDim.y * VJF_FC_WAVES) {
        const int sl = q / A.Tc, t = q - sl * A.Tc;
        for (int j0 = 0; j0 < dout; j0 += 16)
            fc_sample(A.noise + (size_t)sl * A.noise_ms + (size_t)t * n * dout, A.W + (size_t)q * n * dout, A.w_mean, smem, m0, n, dout, j0, lane);
    }
}

struct VjfFeArgs {
    VjfFcArgs a;                                         // member 0 of the chunk; u, c, logw, tr_logvar are shared
    size_t x_in_ms, e_ms, W_ms, x0_out_ms, x_out_ms;     // distance of two members in x_in, e, W, x0_out, x_out (floats)
};

// blockIdx.y: the member.  The step loop is vjf_fc_rollout_kernel's own (fc_rollout), so member s computes
// vjf_forecast_seq's bits on member s's inputs in every form of the kernel (look-ahead, W from L2, centroids in LDS or global memory).
template <int NT, bool CL>
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_fe_rollout_kernel(VjfFeArgs E) {
    VjfFcArgs A = E.a;
    const size_t s = blockIdx.y;
    A.x_in += s * E.x_in_ms;
    if (A.e) A.e += s * E.e_ms;
    A.W += s * E.W_ms;
    if (A.x0_out) A.x0_out += s * E.x0_out_ms;
    A.x_out += s * E.x_out_ms;
    fc_rollout<NT, CL>(A);
}

#define VJF_FE_THREADS 256
#define VJF_FE_WAVES (VJF_FE_THREADS / 64)
#define VJF_FE_TPW 2                                     // output tiles per wavefront: their running moments stay in registers
#define VJF_FE_GROUP (VJF_FE_WAVES * VJF_FE_TPW)         // output tiles per workgroup (blockIdx.z counts groups)
#define VJF_FE_LDC (16 * VJF_FE_GROUP + 16)              // row length of the decoder's LDS copy (k-major): 16 apart mod 32 banks
#define VJF_FE_BATCH 4                                   // members staged per barrier where LDS allows

struct VjfFeMomArgs {
    const float* xs;           // states: member sl of the chunk, row r of the launch at xs + sl * xs_ms + r * B * dout, (B, dout) each
    size_t xs_ms;
    const float* dec_W; const float* dec_b;              // (dy, dout), (dy); dy = 0: no decoder
    float* x_mean; float* x_var; float* y_mean; float* y_var;   // row 0 of the launch: (rows, B, dout) / (rows, B, dy)
    int Sc, ms0, S, last;      // members of the chunk; members folded before it; members in all; last chunk (M2 -> M2 / S)
    int B, dout, dy, mb;       // mb: members staged per barrier (1 or VJF_FE_BATCH)
};

static inline size_t vjf_fe_lds_floats(int dout, int mb, bool dec_lds) {
    return (size_t)2 * mb * dout * VJF_LDT + (dec_lds ? (size_t)dout * VJF_FE_LDC : 0);
}

// The output features of one (step, tile of trials) are [x | y] in tiles of 16: ceil(dout / 16) tiles of x, then ceil(dy / 16) of y.
// Workgroup z owns tiles 8 z .. 8 z + 7, wavefront w of it tiles 8 z + w and 8 z + 4 + w; lane (i = lane & 15, kk = lane >> 4) owns
// rows 4 kk .. 4 kk + 3 of trial i in each: the MFMA's accumulator layout, which an x tile simply reads out of LDS in.  Each owned
// element is folded over the members 0 .. S - 1 in member order by Welford's recurrence in fp32,
//   mean_k = mean_{k-1} + (v - mean_{k-1}) / k,   M2_k = M2_{k-1} + (v - mean_{k-1}) (v - mean_k),
// by that one lane, so its bits depend on that trial's inputs alone: not on the grid, the chunking, the batch or the stream.  Between
// member chunks (mean, M2) live in the output arrays; the last chunk stores M2 / S.
// DL: the decoder's rows of this workgroup's y tiles in LDS (k-major), else read from global memory (L2) as torch stores them; the
// same MFMA steps on the same operands in the same order either way (`decode` below).
// Dead lanes (trials beyond B, features beyond dout / dy) compute on zeros and store nothing.
template <bool DL>
__global__ __launch_bounds__(VJF_FE_THREADS) void vjf_fe_moments_kernel(VjfFeMomArgs A) {
    constexpr int TB = 16, LD = VJF_LDT, NTH = VJF_FE_THREADS, TPW = VJF_FE_TPW, LDC = VJF_FE_LDC;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int dout = A.dout, dy = A.dy, mb = A.mb;
    float* s_x = smem;                                   // 2 x mb x dout x LD   the members' states, double-buffered
    float* s_c = s_x + 2 * mb * dout * LD;               // dout x LDC           decoder rows of this workgroup's y tiles (DL)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b0 = blockIdx.x * TB, nb = min(TB, A.B - b0);
    const int mi = lane & 15, r4 = 4 * (lane >> 4);
    const int xt = (dout + 15) / 16, yt = (dy + 15) / 16, tile0 = blockIdx.z * VJF_FE_GROUP;
    const int ylo = max(tile0 - xt, 0), yhi = min(tile0 + VJF_FE_GROUP - xt, yt);       // this workgroup's y tiles [ylo, yhi)
    const size_t row = (size_t)blockIdx.y * A.B + b0;    // (row of the launch, first trial of the tile)
    const float* src = A.xs + row * dout;

    for (int i = tid; i < 2 * mb * dout * LD; i += NTH) s_x[i] = 0.f;
    if (DL)
        for (int e = tid; e < 16 * (yhi - ylo) * dout; e += NTH) {
            const int j = e / dout, k = e - j * dout;    // (consecutive lanes: consecutive k of one decoder row)
            s_c[k * LDC + j] = (16 * ylo + j) < dy ? A.dec_W[(size_t)(16 * ylo + j) * dout + k] : 0.f;
        }
    __syncthreads();
    auto stage = [&](int sl0, float* buf) {               // members sl0 .. sl0 + mb - 1 of the chunk (live trials only: the rest stay 0)
        for (int m = 0; m < mb && sl0 + m < A.Sc; ++m) {
            const float* xm = src + (size_t)(sl0 + m) * A.xs_ms;
            for (int i = tid; i < nb * dout; i += NTH) {
                const int b = i / dout, j = i - b * dout;
                buf[(m * dout + j) * LD + b] = xm[i];
            }
        }
    };

    // rows j0 .. j0 + 15 of y = x C^T for the 16 trials of xb: K = dout in MFMA steps of 4, k ascending, the last step padded with
    // zeros; `C` holds the tile's first row, two k `ks` apart (the row distance follows: LDS k-major, or global as torch stores it).
    // Addresses beyond dy / dout are clamped and the value masked: nothing is read outside the arrays.
    auto decode = [&](const float* C, int ks, int j0, const float* xb) {
        vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int kk = lane >> 4;
        const bool rv = j0 + mi < dy;
        const float* cp = C + (rv ? (size_t)mi * (ks == 1 ? dout : 1) : 0);
        for (int k0 = 0; k0 < dout; k0 += 4) {
            const bool kv = k0 + kk < dout;
            const int k = kv ? k0 + kk : 0;
            const float cv = cp[(size_t)k * ks], xv = xb[k * LD + mi];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32((rv && kv) ? cv : 0.f, kv ? xv : 0.f, acc, 0, 0, 0);
        }
        return acc;
    };

    // this lane's running moments and, for a y tile, its bias
    float mean[TPW][4], m2[TPW][4], bias[TPW][4];
    float* o_mean[TPW]; float* o_var[TPW];
    int kind[TPW], f0[TPW], fn[TPW];                     // 0 none, 1 x tile, 2 y tile; first feature of the tile; features of the tensor
#pragma unroll
    for (int p = 0; p < TPW; ++p) {
        const int tile = tile0 + p * VJF_FE_WAVES + wave;
        kind[p] = tile < xt ? 1 : (tile < xt + yt ? 2 : 0);
        f0[p] = 16 * (kind[p] == 2 ? tile - xt : tile);
        fn[p] = kind[p] == 2 ? dy : dout;
        o_mean[p] = kind[p] == 2 ? A.y_mean : A.x_mean;
        o_var[p] = kind[p] == 2 ? A.y_var : A.x_var;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = f0[p] + r4 + r;
            const bool live = kind[p] != 0 && mi < nb && j < fn[p];
            const size_t o = live ? (row + mi) * fn[p] + j : 0;
            mean[p][r] = (live && A.ms0 > 0) ? o_mean[p][o] : 0.f;
            m2[p][r] = (live && A.ms0 > 0) ? o_var[p][o] : 0.f;
            bias[p][r] = (kind[p] == 2 && j < dy) ? A.dec_b[j] : 0.f;
        }
    }

    stage(0, s_x);
    __syncthreads();
    for (int sl0 = 0, it = 0; sl0 < A.Sc; sl0 += mb, ++it) {
        const float* cur = s_x + (it & 1) * mb * dout * LD;
        if (sl0 + mb < A.Sc) stage(sl0 + mb, s_x + ((it + 1) & 1) * mb * dout * LD);    // (read last one barrier ago)
        for (int m = 0; m < mb && sl0 + m < A.Sc; ++m) {
            const float* xb = cur + m * dout * LD;
            const float kf = (float)(A.ms0 + sl0 + m + 1);
#pragma unroll
            for (int p = 0; p < TPW; ++p) {
                if (kind[p] == 0) continue;              // (uniform over the wavefront)
                float v[4];
                if (kind[p] == 1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const int j = f0[p] + r4 + r; v[r] = j < dout ? xb[j * LD + mi] : 0.f; }
                } else {
                    const vjf_f32x4 acc = DL ? decode(s_c + (f0[p] - 16 * ylo), LDC, f0[p], xb) : decode(A.dec_W + (size_t)f0[p] * dout, 1, f0[p], xb);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = acc[r] + bias[p][r];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float delta = v[r] - mean[p][r];
                    mean[p][r] += delta / kf;
                    m2[p][r] = fmaf(delta, v[r] - mean[p][r], m2[p][r]);
                }
            }
        }
        __syncthreads();
    }

    const float fS = (float)A.S;
#pragma unroll
    for (int p = 0; p < TPW; ++p) {
        if (kind[p] == 0 || mi >= nb) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = f0[p] + r4 + r;
            if (j < fn[p]) {
                const size_t o = (row + mi) * fn[p] + j;
                o_mean[p][o] = mean[p][r];
                o_var[p][o] = A.last ? m2[p][r] / fS : m2[p][r];
            }
        }
    }
}
}  // namespace
