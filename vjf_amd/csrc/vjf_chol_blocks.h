// vjf_chol_blocks.h -- the 32x32 LDS block primitives of the blocked Cholesky / RLS kernels (vjf_chol_kernel.h,
// vjf_rlsb_kernels.h) and the chain that factors a diagonal block together with the inverse of its factor.  All block
// products run on the f32 matrix cores (v_mfma_f32_32x32x2_f32).
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_gram_kernel.h"   // vjf_f32x16

// ---------------------------------------------------------------------------------------------
// LDS block helpers.  A 32x32 block is 32 rows of VJF_BLK_LD = 33 floats in LDS; element (r,c) sits at r*33 + c.  Every
// block access is a dword access (bank = dword address mod 32, conflicts only inside a half-wavefront), and the patterns in
// use -- c*33 + m, m*33 + c, row*33 + c over the lanes c, the chain's lc*33 + j / j*33 + lc (lc a permutation of the lane) and
// the intake's r*33 + c4 + i (four rows x eight quads) -- put 32 lanes on 32 banks.  Unlike an XOR swizzle, which folds the
// lane into every element offset, each access of a product is ONE per-lane base plus a compile-time offset (the instruction's
// immediate): the routines below form that base once.  Rows are not 16-byte aligned: no wider access to a block.  The last
// float of a block (VJF_BLK_FLOATS - 1) belongs to no element.  Blocks in GLOBAL memory stay 1024 floats, row-major.
#define VJF_BLK_LD 33
#define VJF_BLK_FLOATS (32 * VJF_BLK_LD)
__device__ __forceinline__ int vsw(int r, int c) { return r * VJF_BLK_LD + c; }
__device__ __forceinline__ int vtri(int bi, int bj) { return bi * (bi + 1) / 2 + bj; }
// accumulator layout of v_mfma_f32_32x32x2_f32: column = lane & 31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
__device__ __forceinline__ int vrow(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

__device__ __forceinline__ float vrl(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ float vrsqrt(float d) {               // rsqrt with one Newton step: ~0.5 ulp
    float s = __builtin_amdgcn_rsqf(d);
    return s * fmaf(-0.5f * d * s, s, 1.5f);
}

__device__ __forceinline__ void blk_load(vjf_f32x16& acc, const float* blk, int lane) {
    const float* p = blk + vsw(4 * (lane >> 5), lane & 31);       // row vrow(r, h) = vrow(r, 0) + 4 h
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = p[vrow(r, 0) * VJF_BLK_LD];
}
__device__ __forceinline__ void blk_store(const vjf_f32x16& acc, float* blk, int lane) {
    float* p = blk + vsw(4 * (lane >> 5), lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) p[vrow(r, 0) * VJF_BLK_LD] = acc[r];
}
// acc += Ab * Bb  (Neg: acc -= Ab * Bb; Bt: use Bb^T).  MFMA step t takes k = 2 t + h: A[c][k] and B[k][c] (Bt: B[c][k])
template <bool Bt, bool Neg = false>
__device__ __forceinline__ void blk_mma(vjf_f32x16& acc, const float* Ab, const float* Bb, int lane) {
    const int c = lane & 31, h = lane >> 5;
    const float* pa = Ab + vsw(c, h);
    const float* pb = Bb + (Bt ? vsw(c, h) : vsw(h, c));
    float a[16], b[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {                   // all 32 operand reads first ...
        a[t] = pa[2 * t];
        b[t] = pb[Bt ? 2 * t : 2 * t * VJF_BLK_LD];
    }
    __builtin_amdgcn_sched_barrier(0);               // ... so the 16 MFMAs issue back to back
#pragma unroll
    for (int t = 0; t < 16; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Neg ? -a[t] : a[t], b[t], acc, 0, 0, 0);
}

// acc += A * B with A a block in LDS (At: its transpose) and B given by a functor: fb(m, j) = B[m][j]  (j = lane & 31)
template <bool At, class FB>
__device__ __forceinline__ void blk_mma_f(vjf_f32x16& acc, int lane, const float* Ab, FB fb) {
    const int c = lane & 31, h = lane >> 5;
    const float* pa = Ab + (At ? vsw(h, c) : vsw(c, h));
    float a[16], b[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        a[t] = pa[At ? 2 * t * VJF_BLK_LD : 2 * t];
        b[t] = fb(2 * t + h, c);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 16; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc, 0, 0, 0);
}

// Rank-2 form of the merged chain: two pivots per matrix-core round, so that BOTH k slots of v_mfma_f32_32x32x2 carry a
// column (the rank-1 chain of tools/chol_chain_variants.h zeroes one of them) -- 16 rounds of 2 MFMAs instead of 32 steps of 2.
// The tile sits in the accumulator under a symmetric permutation: register r holds logical row 2r on lanes 0..31 and
// logical row 2r + 1 on lanes 32..63 (physical row (r&3) + 8 (r>>2) + 4 half  <->  logical row 2r + half; same map for the
// columns), so the two pivot rows of a round are the two halves of ONE register and land in the A / B operand layout
// (k = lane >> 5) with no data movement; only column 2m scaled by its pivot has to cross to the other half once
// (v_permlane32_swap) to update row 2m + 1 before its own pivot is taken.  A relabelling only: the factor is the lower
// triangular L of the tile in the natural order.  Reads the tile from `dk`, writes L (lower) back and L^-1 (lower) to `inv`.
__device__ __forceinline__ float vlo2both(float v) {            // lanes 0..31 of v on both halves
    const unsigned u = __float_as_uint(v);
    return __uint_as_float(__builtin_amdgcn_permlane32_swap(u, u, false, false)[0]);
}
// `nvalid`: rows / columns of the tile inside the matrix (the rest is the identity padding of the last block): a round whose two
// pivots are padding would scale by 1 and update by 0 -- it is skipped (a uniform branch around the round: the loop stays fully
// unrolled, every register index static), the result is the same bits.
__device__ __forceinline__ bool potrf_inv_chain2(float* dk, float* inv, int lane, int nvalid = 32) {
    const int c = lane & 31, h = lane >> 5;
    const int lc = 2 * ((c & 3) + 4 * (c >> 3)) + ((c >> 2) & 1);   // logical column held by this lane
    vjf_f32x16 acc, racc;
    const float* pin = dk + vsw(h, lc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int lr = 2 * r + h;                                   // logical row of (register r, half h)
        acc[r] = pin[2 * r * VJF_BLK_LD];
        racc[r] = (lr == lc) ? 1.f : 0.f;
    }
    float vcol[16], xcol[16];
    float dmin = 3.0e38f, slast = 1.f;
    const int rounds = (nvalid + 1) >> 1;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        vcol[m] = xcol[m] = (lc == 2 * m + h) ? 1.f : 0.f;          // (what a skipped round leaves: the identity)
        if (m < rounds) {                                           // (uniform)
        const int p1 = (m & 3) + 8 * (m >> 2), p2 = p1 + 4;         // physical columns of logical 2m and 2m + 1
        const float d1 = vrl(acc[m], p1);                           // T[2m][2m]
        const float q2 = vrl(acc[m], 32 + p2);                      // T[2m+1][2m+1], before column 2m is eliminated
        const float s1 = __builtin_amdgcn_rsqf(d1);
        const float l1 = acc[m] * s1;                               // lanes 0..31: L[.][2m]
        const float e = vrl(l1, p2);                                // L[2m+1][2m]
        const float t = fmaf(-e, vlo2both(l1), acc[m]);             // lanes 32..63: row 2m+1 with column 2m eliminated
        const float d2 = fmaf(-e, e, q2);
        const float s2 = __builtin_amdgcn_rsqf(d2);
        const float v = h ? t * s2 : l1;                            // L[.][2m] | L[.][2m+1] by half = the k slot
        const float x1 = racc[m] * s1;                              // lanes 0..31: Linv[2m][.]
        const float x2 = fmaf(-e, vlo2both(x1), racc[m]) * s2;      // lanes 32..63: Linv[2m+1][.]
        const float b = h ? x2 : x1;
        const float nv = -v;
        dmin = fminf(dmin, fminf(d1, d2));
        slast = s2;
        vcol[m] = v;
        xcol[m] = b;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(nv, v, acc, 0, 0, 0);
        racc = __builtin_amdgcn_mfma_f32_32x32x2f32(nv, b, racc, 0, 0, 0);
        }
    }
    float* pl = dk + vsw(lc, h);
    float* px = inv + vsw(h, lc);
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const int j = 2 * m + h;
        if (lc >= j) pl[2 * m] = vcol[m];                           // dk[vsw(lc, j)]
        px[2 * m * VJF_BLK_LD] = (lc <= j) ? xcol[m] : 0.f;         // inv[vsw(j, lc)]
    }
    return (dmin > 0.f) && (slast == slast) && (fabsf(slast) < 3.0e38f);
}
