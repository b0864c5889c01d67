// vjf_kstep_kernel.h -- k-step-ahead prediction error of the mean map x <- x + Phi([x, u]) w_mean over a filtered record, the
// figure reported for learned dynamics: from every row t the map is rolled h = 1 .. K steps and compared with what the filter found
// at row t + h (mu) and with what was observed there (y, through the decoder), summed over the record per horizon and column.
//
//   vjf_kstep_tile_kernel   one workgroup per tile of 16 consecutive starts of the flattened record (start r = t B + b; horizon h
//                           of it is compared with row r + h B, step j reads row r + j B of u): the x step of vjf_rollout_step.h with
//                           W = w_mean at every step, y-hat = xh C^T + b decoded on chip per horizon, and per horizon and column the
//                           live starts' terms added in start order in fp32 -> one partial per (tile, horizon, column) in scratch.
//   vjf_kstep_fold_kernel   one lane per (horizon, column): the tiles' partials added in tile order into an fp64 accumulator that
//                           lives in the scratch across chunks of tiles; the last chunk writes the outputs as float64.
//
// No atomics: the bits are defined by the order of the starts alone (not by the chunking, the stream or the forms of the x step).
// Tiling as in vjf_forecast_kernel.h: activations feature-major in LDS ([feature][VJF_LDT]), the start on the MFMA column of
// v_mfma_f32_16x16x4_f32, so a start's prediction depends on that start's inputs alone.  A start whose horizon has run out of record
// keeps stepping (on the control input it read last) and is masked out of the sums and of `pred`.
// The decode is vjf_fe_moments_kernel's (a lambda of that kernel, so it is restated here: the same MFMA steps, k ascending, the last
// step padded with zeros), with the whole decoder in LDS where it fits.
// Included by vjf_host_kstep.h.  The kernels sit in an anonymous namespace: their symbols carry it.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_forecast_kernel.h"     // vjf_rollout_step.h: the x step, FcTile, VJF_FC_THREADS / _WAVES / _KQ, vjf_f32x4, VJF_LDT

#define VJF_KS_ETA_MAX 10.f          // the Poisson likelihood's clamp of the linear predictor (vjf/likelihood.py:60)

namespace {
struct VjfKsArgs {
    const float* mu;         // (R, dout): the filtered means, R = T B rows
    const float* y;          // (R, dy) or null
    const float* u;          // (R, du) or null
    const float* c; const float* logw;     // centroids (n, d), log widths (n)
    const float* w;          // w_mean (n, dout)
    const float* dec_W; const float* dec_b;   // (dy, dout), (dy); read when dy > 0
    float* part;             // (tiles of the chunk, K + 1, 2 dout + 2 dy): [sse_x | base_x | sse_y or nll_y | base_y] per horizon
    float* pred;             // (K, R, dout) or null
    long long R, tile0;      // rows of the record; the chunk's first tile
    int B, K, n, d, dout, dy, poisson;
};

// A product, a sum and a difference rounded on their own.  This toolchain's __fmul_rn / __fadd_rn / __fsub_rn are the plain operators,
// which hipcc's default -ffp-contract=fast fuses with a neighbour into one fma (one rounding); the pragma keeps the roundings apart,
// so the sums have the bits the stated order defines (tests/test_gpu_kstep.py recomputes them in numpy).
__device__ __forceinline__ float ks_mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float ks_add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float ks_sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// row length of the decoder's LDS copy (k-major): two k are 16 apart mod 32 banks
__host__ __device__ static inline size_t vjf_ks_ldc(int dy) { return ((size_t)dy + 31) / 32 * 32 + 16; }
// the x step's buffers plus xh_0, y-hat of this horizon and of horizon 0 and (dec_lds) the decoder
static inline size_t vjf_ks_lds_floats(int n, int d, int dout, int dy, bool cen_lds, bool dec_lds) {
    const size_t dyp = ((size_t)dy + 15) / 16 * 16;
    return vjf_fc_lds_floats(n, d, dout, cen_lds) + (size_t)dout * VJF_LDT + 2 * dyp * VJF_LDT + (dec_lds ? (size_t)dout * vjf_ks_ldc(dy) : 0);
}

// NT, CL: vjf_fc_rollout_kernel's forms of the x step (NT > 0: this lane's elements of w_mean are fetched once and stay in registers;
//         NT == 0: any shape, they are read when they are used) and of the centroids (CL: in LDS).  DL: the decoder in LDS, else read
//         from global memory (L2) as torch stores it.  All forms issue the same MFMA steps on the same operands in the same order.
template <int NT, bool CL, bool DL>
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_kstep_tile_kernel(VjfKsArgs A) {
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_FC_WAVES, NTH = VJF_FC_THREADS;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FcTile S = fc_tile(smem, A.n, A.d, A.dout, 0);
    const int dout = S.dout, du = S.du, dy = A.dy, K = A.K, dyp = (dy + 15) / 16 * 16, ldc = (int)vjf_ks_ldc(dy), ncol = 2 * dout + 2 * dy;
    const long long R = A.R, r0 = (A.tile0 + blockIdx.x) * TB;       // the tile's first start
    S.b0 = 0;                                                        // (the tile's rows are addressed through r0)
    S.nb = (int)(R - r0 < TB ? R - r0 : TB);
    float* s_x = S.s_x;
    float* s_x0 = S.rest;                         // dout x LD    xh_0 = mu of the tile's starts (the baselines)
    float* s_y = s_x0 + dout * LD;                // dyp x LD     y-hat of xh_h
    float* s_y0 = s_y + dyp * LD;                 // dyp x LD     y-hat of xh_0
    float* s_dec = s_y0 + dyp * LD;               // dout x ldc   the decoder, k-major (DL)
    S.s_c = s_dec + (DL ? dout * ldc : 0);        // n x d        centroids (CL): behind this kernel's buffers
    const int tid = S.tid, lane = S.lane, wave = S.wave, nb = S.nb, mi = S.mi, r4 = S.r4;
    // the tile's starts whose horizon h is inside the record: the first live(h) of them, since the starts are consecutive rows
    auto live = [&](int h) {
        const long long l = R - (r0 + (long long)h * A.B);
        return (int)(l < 0 ? 0 : (l > nb ? nb : l));
    };

    fc_stage<CL, false>(S, A.logw, A.c, nullptr, A.mu + r0 * dout, nullptr, nullptr);
    for (int i = tid; i < TB * dout; i += NTH) {                     // (each thread copies what it has just staged)
        const int b = i / dout, j = i - b * dout;
        s_x0[j * LD + b] = s_x[j * LD + b];
    }
    if (du > 0) {                                                    // step 1 reads row r + B of u: zeros, then the live rows (same thread, same element)
        for (int i = tid; i < TB * du; i += NTH) {
            const int b = i / du, j = i - b * du;
            s_x[(dout + j) * LD + b] = 0.f;
        }
        FcTile Su = S;
        Su.nb = K >= 1 ? live(1) : 0;
        const float* un = Su.nb > 0 ? A.u + (r0 + A.B) * du : nullptr;
        fc_u_advance(Su, un, fc_u_ahead(Su, un));
    }
    if (DL)
        for (int e = tid; e < dyp * dout; e += NTH) {
            const int j = e / dout, k = e - j * dout;                // (consecutive lanes: consecutive k of one decoder row)
            s_dec[k * ldc + j] = j < dy ? A.dec_W[(size_t)j * dout + k] : 0.f;
        }
    float aw[NT > 0 ? NT : 1][VJF_FC_KQ];                // (NT > 0) this lane's A operands of the x step: w_mean, the same at every step
    if constexpr (NT > 0) fc_fetch_w(S, A.w, aw);
    __syncthreads();

    // rows j0 .. j0 + 15 of y = x C^T for the tile's 16 starts: K = dout in MFMA steps of 4, k ascending, the last step padded with
    // zeros; `C` holds the tile's first row, two k `ks` apart (LDS k-major, or global as torch stores it).  Addresses beyond dy / dout
    // are clamped and the value masked: nothing is read outside the arrays.  (vjf_fe_moments_kernel's decode.)
    auto decode = [&](const float* C, int ks, int j0) {
        vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int kk = lane >> 4;
        const bool rv = j0 + mi < dy;
        const float* cp = C + (rv ? (size_t)mi * (ks == 1 ? dout : 1) : 0);
        for (int k0 = 0; k0 < dout; k0 += 4) {
            const bool kv = k0 + kk < dout;
            const int k = kv ? k0 + kk : 0;
            const float cv = cp[(size_t)k * ks], xv = s_x[k * LD + mi];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32((rv && kv) ? cv : 0.f, kv ? xv : 0.f, acc, 0, 0, 0);
        }
        return acc;
    };
    const float nan = __builtin_nanf("");

    for (int h = 0; h <= K; ++h) {
        const int lv = live(h);                                      // (uniform; never grows with h)
        float* ph = A.part + ((size_t)blockIdx.x * (K + 1) + h) * ncol;
        if (lv == 0) {                                               // the whole tile has run out of record
            for (int col = tid; col < ncol; col += NTH) ph[col] = 0.f;
            if (A.pred)
                for (int i = tid; i < nb * dout; i += NTH) A.pred[((size_t)(h - 1) * R + r0) * dout + i] = nan;
            continue;
        }
        if (dy > 0) {
            for (int yt = wave; yt < dyp / 16; yt += NW) {
                const vjf_f32x4 acc = DL ? decode(s_dec + 16 * yt, ldc, 16 * yt) : decode(A.dec_W + (size_t)16 * yt * dout, 1, 16 * yt);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * yt + r4 + r;
                    const float v = acc[r] + (j < dy ? A.dec_b[j] : 0.f);
                    s_y[j * LD + mi] = v;
                    if (h == 0) s_y0[j * LD + mi] = v;
                }
            }
            __syncthreads();
        }
        // per column the live starts' terms in start order: each term rounded on its own, then added.  (The targets are read from
        // global memory by the summing lane: staging the tile's target rows into LDS with every lane first was measured and was slower,
        // 15.3 -> 17.6 ms per call at 4096 trials x 200 rows -- a barrier more per horizon, DESIGN.md section 3 "Scoring predictions".)
        const long long rt = r0 + (long long)h * A.B;                // the targets' first row
        for (int col = tid; col < dout + dy; col += NTH) {
            float s = 0.f, sb = 0.f;
            if (col < dout) {
                const float* tg = A.mu + rt * dout + col;
                for (int b = 0; b < lv; ++b) {
                    const float t = tg[(size_t)b * dout];
                    const float e = ks_sub_rn(s_x[col * LD + b], t), e0 = ks_sub_rn(s_x0[col * LD + b], t);
                    s = ks_add_rn(s, ks_mul_rn(e, e));
                    sb = ks_add_rn(sb, ks_mul_rn(e0, e0));
                }
                ph[col] = s;
                ph[dout + col] = sb;
            } else {
                const int cy = col - dout;
                const float* tg = A.y + rt * dy + cy;
                for (int b = 0; b < lv; ++b) {
                    const float t = tg[(size_t)b * dy], eta = s_y[cy * LD + b], eta0 = s_y0[cy * LD + b];
                    if (A.poisson) {                                 // exp(min(eta, 10)) - y min(eta, 10); a NaN stays one
                        const float c1 = eta > VJF_KS_ETA_MAX ? VJF_KS_ETA_MAX : eta, c0 = eta0 > VJF_KS_ETA_MAX ? VJF_KS_ETA_MAX : eta0;
                        s = ks_add_rn(s, ks_sub_rn(expf(c1), ks_mul_rn(t, c1)));
                        sb = ks_add_rn(sb, ks_sub_rn(expf(c0), ks_mul_rn(t, c0)));
                    } else {
                        const float e = ks_sub_rn(eta, t), e0 = ks_sub_rn(eta0, t);
                        s = ks_add_rn(s, ks_mul_rn(e, e));
                        sb = ks_add_rn(sb, ks_mul_rn(e0, e0));
                    }
                }
                ph[2 * dout + cy] = s;
                ph[2 * dout + dy + cy] = sb;
            }
        }
        if (h == K) break;
        if (live(h + 1) == 0) continue;                              // (no start left to predict for: the branch above ends the tile)

        // xh_{h+1} from xh_h; the control input of the step after it (row r + (h + 2) B, the starts still inside the record) is in
        // flight while the features are computed
        FcTile Su = S;
        Su.nb = h + 2 <= K ? live(h + 2) : 0;
        const float* un = du > 0 && Su.nb > 0 ? A.u + (r0 + (long long)(h + 2) * A.B) * du : nullptr;
        const float u0 = fc_u_ahead(Su, un);
        fc_features<CL>(S, A.c);
        __syncthreads();
        if constexpr (NT > 0) fc_product_reg(S, aw);
        else fc_product_masked(S, A.w);
        __syncthreads();
        float* po = A.pred ? A.pred + ((size_t)h * R + r0) * dout : nullptr;     // (row h of pred is horizon h + 1)
        const int l1 = live(h + 1) * dout;
        fc_advance(S, [&](int i, float v) {
            if (po) po[i] = i < l1 ? v : nan;
            return v;
        });
        fc_u_advance(Su, un, u0);
        __syncthreads();
    }
}

struct VjfKsFoldArgs {
    const float* part;       // (tiles, E)
    double* acc;             // (E): the running sums, in the scratch across chunks
    double* sse_x; double* base_x; double* sse_y; double* base_y;    // (K + 1, dout) / (K + 1, dy)
    long long tiles;
    int E, ncol, dout, dy, first, last;      // E = (K + 1) ncol; first / last chunk of the call
};

// Lane e owns element e = h ncol + column of every tile's partials: tile order, fp64.
__global__ __launch_bounds__(256) void vjf_kstep_fold_kernel(VjfKsFoldArgs A) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= A.E) return;
    double a = A.first ? 0.0 : A.acc[e];
    // (sixteen tiles' loads in flight, then their additions in tile order: the chain is the additions', not the loads')
    long long t = 0;
    for (; t + 16 <= A.tiles; t += 16) {
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = A.part[(size_t)(t + q) * A.E + e];
#pragma unroll
        for (int q = 0; q < 16; ++q) a += (double)v[q];
    }
    for (; t < A.tiles; ++t) a += (double)A.part[(size_t)t * A.E + e];
    A.acc[e] = a;
    if (A.last) {
        const int h = e / A.ncol, cc = e - h * A.ncol, dout = A.dout, dy = A.dy;
        if (cc < dout) A.sse_x[(size_t)h * dout + cc] = a;
        else if (cc < 2 * dout) A.base_x[(size_t)h * dout + cc - dout] = a;
        else if (cc < 2 * dout + dy) A.sse_y[(size_t)h * dy + cc - 2 * dout] = a;
        else A.base_y[(size_t)h * dy + cc - 2 * dout - dy] = a;
    }
}
}  // namespace
