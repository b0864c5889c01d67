// vjf_rollout_step.h -- the step x <- x + Phi([x, u]) W of one tile of 16 trials, once, for the three kernels that advance it:
// vjf_fc_rollout_kernel and vjf_fe_rollout_kernel (fc_rollout in vjf_forecast_kernel.h: W = W[t], state noise, every state stored) and
// vjf_tangent_rollout_kernel (W = w_mean at every step).  A kernel calls, per step: fc_u_ahead, fc_features, barrier, one of the
// products, barrier, fc_advance, fc_u_advance, barrier.  Every function is inlined into its caller;
// what they share is FcTile.  Activations are feature-major in LDS ([feature][VJF_LDT]), the trial on the column of v_mfma_f32_16x16x4_f32.
// Included by vjf_forecast_kernel.h.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_trial_mfma_kernel.h"   // mma_tile, vjf_f32x4, VJF_LDT

#define VJF_FC_THREADS 256
#define VJF_FC_WAVES (VJF_FC_THREADS / 64)
#define VJF_FC_KQ 16                 // MFMA steps of one wavefront's share of K that the register form keeps in registers
#define VJF_FC_REG_N (4 * VJF_FC_WAVES * VJF_FC_KQ)   // features the register form covers: 4 per MFMA step and wavefront (256)

// LDS of the x step: features, [x, u], the wavefronts' partial products, width^2 and, if asked for, the centroids
static inline size_t vjf_fc_lds_floats(int n, int d, int dout, bool cen_lds) {
    const size_t doutp = ((size_t)dout + 15) / 16 * 16;
    return (size_t)n * VJF_LDT + (size_t)d * VJF_LDT + (size_t)VJF_FC_WAVES * doutp * VJF_LDT + (size_t)n + (cen_lds ? (size_t)n * d : 0);
}
// (the register form, NT > 0: every planner asks this)
static inline bool vjf_fc_reg_form(int n, int dout) { return n <= VJF_FC_REG_N && dout <= 32; }

namespace {
// this wavefront's share of K: a multiple of 4 features per wavefront, the last one takes what is left
__device__ __forceinline__ void fc_k_range(int n, int wave, int& kb, int& ke) {
    const int per = ((n + VJF_FC_WAVES - 1) / VJF_FC_WAVES + 3) & ~3;
    kb = min(wave * per, n);
    ke = min(kb + per, n);
}

struct FcTile {
    float* s_phi;            // n x LD       features of step t
    float* s_x;              // d x LD       [x_t, u_t]
    float* s_part;           // NW x doutp x LD   the wavefronts' partial products
    float* s_w2;             // n            width^2
    float* rest;             // the first float behind them: the kernel's own buffers
    float* s_c;              // n x d        centroids (CL): at `rest`; a kernel with buffers of its own moves it before fc_stage
    int n, d, dout, du, doutp;
    int tid, lane, wave, mi, kk, r4;         // mi, kk: MFMA column and K slot of this lane; r4: its first accumulator row
    int b0, nb, kb, ke;                      // the tile's first trial and its live trials; this wavefront's share of K
};

__device__ __forceinline__ FcTile fc_tile(float* smem, int n, int d, int dout, int B) {
    FcTile S;
    S.n = n; S.d = d; S.dout = dout; S.du = d - dout; S.doutp = (dout + 15) / 16 * 16;
    S.s_phi = smem; S.s_x = S.s_phi + n * VJF_LDT; S.s_part = S.s_x + d * VJF_LDT;
    S.s_w2 = S.s_part + VJF_FC_WAVES * S.doutp * VJF_LDT; S.rest = S.s_w2 + n; S.s_c = S.rest;
    S.tid = threadIdx.x; S.lane = S.tid & 63; S.wave = S.tid >> 6;
    S.mi = S.lane & 15; S.kk = S.lane >> 4; S.r4 = 4 * (S.lane >> 4);
    S.b0 = blockIdx.x * 16; S.nb = min(16, B - S.b0);
    fc_k_range(n, S.wave, S.kb, S.ke);
    return S;
}

// width^2 (IW: and 1 / width^2 into s_iw2, the kernel's own), the centroids (CL: into S.s_c), the tile's rows of x_in (B, dout;
// copied to x0_out if given) and of u (B, du) if given; rows beyond the batch are zeros.  No barrier.
template <bool CL, bool IW>
__device__ __forceinline__ void fc_stage(const FcTile& S, const float* logw, const float* c, float* s_iw2,
                                         const float* x_in, float* x0_out, const float* u) {
    constexpr int TB = 16, LD = VJF_LDT, NTH = VJF_FC_THREADS;
    const int n = S.n, d = S.d, dout = S.dout, du = S.du;
    const size_t row0 = (size_t)S.b0 * dout;  // the tile's rows in a (B, dout) array are contiguous
    for (int k = S.tid; k < n; k += NTH) {
        const float w = expf(logw[k]);
        S.s_w2[k] = w * w;
        if (IW) s_iw2[k] = 1.f / (w * w);
    }
    if (CL) for (int i = S.tid; i < n * d; i += NTH) S.s_c[i] = c[i];
    for (int i = S.tid; i < TB * dout; i += NTH) {
        const int b = i / dout, j = i - b * dout;
        float v = 0.f;
        if (b < S.nb) {
            v = x_in[row0 + i];
            if (x0_out) x0_out[row0 + i] = v;
        }
        S.s_x[j * LD + b] = v;
    }
    if (u)
        for (int i = S.tid; i < TB * du; i += NTH) {
            const int b = i / du, j = i - b * du;
            S.s_x[(dout + j) * LD + b] = b < S.nb ? u[(size_t)S.b0 * du + i] : 0.f;
        }
}

// features: exp(-1/2 |xu - c|^2 / width^2), the squared distance as a sum of squared differences (c: the centroids in global memory)
template <bool CL>
__device__ __forceinline__ void fc_features(const FcTile& S, const float* c) {
    constexpr int TB = 16, LD = VJF_LDT;
    const int d = S.d;
    for (int i = S.tid; i < TB * S.n; i += VJF_FC_THREADS) {
        const int k = i / TB, b = i - k * TB;
        float ph = 0.f;
        if (b < S.nb) {
            float d2 = 0.f;
            for (int j = 0; j < d; ++j) { const float df = S.s_x[j * LD + b] - (CL ? S.s_c[k * d + j] : c[(size_t)k * d + j]); d2 = fmaf(df, df, d2); }
            ph = expf(-0.5f * d2 / S.s_w2[k]);
        }
        S.s_phi[k * LD + b] = ph;
    }
}

// ---- Phi W, K split over the four wavefronts: partial(row j, col trial) of features kb .. ke - 1 into s_part.  The three forms
//      issue the same MFMA steps on the same operands in the same order, so they compute the same bits.
// Register form (n <= VJF_FC_REG_N, dout <= 16 NT): this lane's A operands are fetched ahead of the step that uses them ...
template <int NT>
__device__ __forceinline__ void fc_fetch_w(const FcTile& S, const float* W, float (&aw)[NT][VJF_FC_KQ]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < VJF_FC_KQ; ++q) {
            const int k = S.kb + 4 * q + S.kk, j = t * 16 + S.mi;
            const bool ok = k < S.ke && j < S.dout;       // (masked where the value is used: the loads stay in flight)
            aw[t][q] = W[ok ? (size_t)k * S.dout + j : 0];
        }
}
// ... and the product reads nothing but them and s_phi
template <int NT>
__device__ __forceinline__ void fc_product_reg(const FcTile& S, const float (&aw)[NT][VJF_FC_KQ]) {
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
        vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const bool rv = tl * 16 + S.mi < S.dout;
#pragma unroll
        for (int q = 0; q < VJF_FC_KQ; ++q) {
            const int k0 = S.kb + 4 * q;
            if (k0 < S.ke) {                                         // (uniform over the wavefront)
                const bool kv = k0 + S.kk < S.ke;
                const float xv = S.s_phi[(kv ? k0 + S.kk : S.kb) * VJF_LDT + S.mi];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32((rv && kv) ? aw[tl][q] : 0.f, kv ? xv : 0.f, acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) S.s_part[(S.wave * S.doutp + tl * 16 + S.r4 + r) * VJF_LDT + S.mi] = acc[r];
    }
}
// Streamed forms, any shape.  Two, because their operands lie differently: the roll-out's W[t] is in L2 with four rows of padding behind
// the last sample, so mma_tile may keep batches of loads in flight and read up to row n + 2 where a share of K is shorter than 4; the
// tangent kernel's w_mean is the model's own array (or its copy in LDS) with nothing behind it, so every address is clamped into it and
// the value masked.  fc_product_padded is one output tile, rows j0 .. j0 + 15, the loop over the tiles its caller's: with that loop inside
// a routine around mma_tile the <0, *> roll-out kernels took 7 VGPRs more and lost a wavefront of occupancy (fc_sample: code grew).
__device__ __forceinline__ void fc_product_padded(const FcTile& S, const float* W, int j0) {
    vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (S.kb < S.ke) mma_tile(acc, W + (size_t)S.kb * S.dout, S.dout, S.dout, j0, S.s_phi + S.kb * VJF_LDT, S.ke - S.kb, S.lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) S.s_part[(S.wave * S.doutp + j0 + S.r4 + r) * VJF_LDT + S.mi] = acc[r];
}
__device__ __forceinline__ void fc_product_masked(const FcTile& S, const float* W) {
    for (int j0 = 0; j0 < S.dout; j0 += 16) {
        vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const bool rv = j0 + S.mi < S.dout;
        for (int k0 = S.kb; k0 < S.ke; k0 += 4) {
            const bool kv = k0 + S.kk < S.ke, ok = rv && kv;
            const float av = W[ok ? (size_t)(k0 + S.kk) * S.dout + j0 + S.mi : 0];
            const float xv = S.s_phi[(kv ? k0 + S.kk : S.kb) * VJF_LDT + S.mi];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? av : 0.f, kv ? xv : 0.f, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) S.s_part[(S.wave * S.doutp + j0 + S.r4 + r) * VJF_LDT + S.mi] = acc[r];
    }
}

// x_{t+1} = tail(i, x_t + (p0 + p1 + p2 + p3)), element i = b dout + j of the tile's live rows, the four partials in a fixed order;
// `tail` is the kernel's own end of the step (state noise, a store) and returns what the next step starts from
template <class Tail>
__device__ __forceinline__ void fc_advance(const FcTile& S, Tail&& tail) {
    constexpr int LD = VJF_LDT;
    for (int i = S.tid; i < S.nb * S.dout; i += VJF_FC_THREADS) {
        const int b = i / S.dout, j = i - b * S.dout;
        float v = S.s_part[j * LD + b];
#pragma unroll
        for (int w = 1; w < VJF_FC_WAVES; ++w) v += S.s_part[(w * S.doutp + j) * LD + b];
        S.s_x[j * LD + b] = tail(i, S.s_x[j * LD + b] + v);
    }
}

// The next step's control input, un = this tile's rows of u[t + 1] (null: there is none): each thread's first element is loaded at
// the top of the step and is in flight while the features are computed; it goes into s_x behind fc_advance.
__device__ __forceinline__ float fc_u_ahead(const FcTile& S, const float* un) { return un && S.tid < S.nb * S.du ? un[S.tid] : 0.f; }
__device__ __forceinline__ void fc_u_advance(const FcTile& S, const float* un, float u0) {
    if (un)
        for (int i = S.tid; i < S.nb * S.du; i += VJF_FC_THREADS) {
            const int b = i / S.du, j = i - b * S.du;
            S.s_x[(S.dout + j) * VJF_LDT + b] = i == S.tid ? u0 : un[i];
        }
}
}  // namespace
