// Diagnostic micro-benchmark: one trailing-update block product (load C, 16 MFMAs, store C) of the Cholesky kernel, as
// trail_tile runs it: the three tile indices are RUN-TIME values (read from memory per product, as vtri(bi, bj) of the loop
// counters is in the kernel), so the per-lane addresses of a product are formed per product and not hoisted out of the loop.
// Prints cycles per product for one wavefront, one per SIMD (4) and two per SIMD (8: the workgroup of the kernel).
//   hipcc --offload-arch=gfx950 -O3 -o tools/blk_mma_bench tools/blk_mma_bench.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include "../vjf_amd/csrc/vjf_chol_blocks.h"
#define NREP 64
#define NBLK 24
__global__ __launch_bounds__(512) void k(float* out, unsigned long long* t, const int* tiles, int nw) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < NBLK * VJF_BLK_FLOATS; e += 512) lds[e] = 0.001f * (e % 977);
    __syncthreads();
    unsigned long long t1 = 0, t2 = 0;
    if (wave < nw) {
        const int* my = tiles + wave * 3 * NREP;                   // (uniform: scalar loads)
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");
        for (int rep = 0; rep < NREP; ++rep) {
            const int ic = my[3 * rep], ia = my[3 * rep + 1], ib = my[3 * rep + 2];
            float* cb = lds + (size_t)ic * VJF_BLK_FLOATS;
            vjf_f32x16 acc;
            blk_load(acc, cb, lane);
            blk_mma<true, true>(acc, lds + (size_t)ia * VJF_BLK_FLOATS, lds + (size_t)ib * VJF_BLK_FLOATS, lane);
            blk_store(acc, cb, lane);
        }
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t2)::"memory");
    }
    __syncthreads();
    out[tid] = lds[tid];
    if (lane == 0) t[wave] = t2 - t1;
}
__global__ void spin(float* out, int n) { float v = threadIdx.x; for (int i = 0; i < n; ++i) v = fmaf(v, 1.0000001f, 0.5f); if (v == 123.f) out[0] = v; }
int main() {
    float* out; unsigned long long* t; int* tiles;
    hipMalloc(&out, 4096); hipMalloc(&t, 64); hipMalloc(&tiles, 8 * 3 * NREP * sizeof(int));
    static int h_tiles[8 * 3 * NREP];
    for (int w = 0; w < 8; ++w)                                    // every wavefront its own three blocks, in a changing order
        for (int r = 0; r < NREP; ++r)
            for (int q = 0; q < 3; ++q) h_tiles[(w * NREP + r) * 3 + q] = 3 * w + (q + r) % 3;
    hipMemcpy(tiles, h_tiles, sizeof(h_tiles), hipMemcpyHostToDevice);
    const size_t bytes = (size_t)NBLK * VJF_BLK_FLOATS * 4;
    hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    spin<<<2048, 256>>>(out, 20000000); hipDeviceSynchronize();
    unsigned long long h[8];
    for (int nw : {1, 4, 8}) {
        for (int rep = 0; rep < 2; ++rep) { k<<<1, 512, bytes>>>(out, t, tiles, nw); hipDeviceSynchronize(); }
        hipMemcpy(h, t, 64, hipMemcpyDeviceToHost);
        printf("%d wavefronts (%s): cycles per block product:", nw, nw == 1 ? "one" : nw == 4 ? "1 per SIMD" : "2 per SIMD");
        for (int w = 0; w < nw; ++w) printf(" %llu", h[w] / NREP);
        printf("\n");
    }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
