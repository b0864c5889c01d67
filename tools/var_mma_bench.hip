// Diagnostic micro-benchmark (not part of the product): the predictive-variance share of ONE trial workgroup (vjf_mega_trial.h, stage 2:
// mg_var2 of vjf_mega_common.h) at config B's shape -- sum_j (L^-1 Phi)_j^2 for one tile of 32 trials, n = 200 features, 8 wavefronts
// with the snake deal of the row tiles, Xt = L^-1 row-major in memory read with 16-byte sc1 loads, Phi in LDS at LD = 33 -- in the
// variants below, 128 workgroups of 512 threads (one per compute unit), R repetitions.
//   V0  the routine as it was before the interior / partial split (clamped k, masked A at every k-step), kept here VERBATIM as the reference
//   V1  full 16-k steps without clamp and mask, B operands at immediate offsets from one base per batch, rows >= n from a bounded
//       descriptor (zeros); the next step's eight reads issued in front of this step's MFMAs   (look-ahead of one 16-k step: the product's form)
//   V2  the same without look-ahead: a step's eight reads directly in front of its MFMAs
//   V3  V1 with the B operands in HALF steps: four reads (two k-steps), the next half step's four in front of this one's MFMAs --
//       8 registers of B operands instead of 16
//   V4  V2 in half steps: 4 registers
// Every variant is checked against a plain fp64 product and BIT FOR BIT against V0 (every lane's two partial sums), for the triangle and
// the dense walk and for n = 200 and n = 224 (and n = 196, 212: a last row tile with rows >= n, a partial step in the dense walk).
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -o tools/var_mma_bench tools/var_mma_bench.hip && tools/var_mma_bench
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../vjf_amd/csrc/vjf_handoff.h"   // vjf_rsrc, vjf_ld4_sc1, vjf_f32x4
constexpr int LD = 33, NT = 512, NW = 8, TR = 32, NMAX = 224;

// ---- V0: mg_var2 of the parent, verbatim
__device__ __forceinline__ void var_v0(float& v2a, float& v2b, __amdgpu_buffer_rsrc_t rx, int n, int j0A, int KA, int j0B, int KB,
                                       const float* Xs, int lane) {
    if (j0A < 0) return;
    const int i = lane & 15, kk = lane >> 4;
    const bool rvA = (j0A + i) < n, rvB = j0B >= 0 && (j0B + i) < n;
    const int offA = (rvA ? j0A + i : 0) * n + 4 * kk, offB = (rvB ? j0B + i : 0) * n + 4 * kk;
    const float* xp = Xs + i;
    const int ntA = (KA + 15) >> 4, ntB = j0B >= 0 ? (KB + 15) >> 4 : 0;
    const int SA = (ntA + 3) >> 2, SB = (ntB + 3) >> 2, S = SA + SB;
    vjf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    auto fold = [&]() {
        v2a = fmaf(acc0[0], acc0[0], fmaf(acc0[1], acc0[1], fmaf(acc0[2], acc0[2], fmaf(acc0[3], acc0[3], v2a))));
        v2b = fmaf(acc1[0], acc1[0], fmaf(acc1[1], acc1[1], fmaf(acc1[2], acc1[2], fmaf(acc1[3], acc1[3], v2b))));
    };
    auto ldb = [&](float4 (&a)[4], int sb) {
        const bool inB = sb >= SA;                                            // (uniform)
        const int t0 = 4 * (inB ? sb - SA : sb), off = inB ? offB : offA;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int kq = 16 * (t0 + q) + 4 * kk; a[q] = vjf_ld4_sc1(rx, off + (kq + 3 < n ? 16 * (t0 + q) : 0)); }
    };
    auto mmb = [&](const float4 (&a)[4], int sb) {
        const bool inB = sb >= SA;
        const int t0 = 4 * (inB ? sb - SA : sb), nt = inB ? ntB : ntA, ke = inB ? KB : KA;
        const bool rv = inB ? rvB : rvA;
        if (sb == SA && SA > 0) {                                             // the first batch of the second tile
            fold();
            acc0 = vjf_f32x4{0.f, 0.f, 0.f, 0.f}; acc1 = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (t0 + q < nt) {                                                // (uniform)
                const int k0 = 16 * (t0 + q) + 4 * kk;
                const float av[4] = {a[q].x, a[q].y, a[q].z, a[q].w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k = k0 + c, kc = min(k, ke - 1);
                    const float v = (rv && k < ke) ? av[c] : 0.f;             // (masked at use: see mg_mma2)
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(v, xp[kc * LD], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(v, xp[kc * LD + 16], acc1, 0, 0, 0);
                }
            }
        }
    };
    float4 a0[4], a1[4], a2[4];
    ldb(a0, 0);
    if (S > 1) ldb(a1, 1);
    if (S > 2) ldb(a2, 2);
    for (int sb = 0; sb < S; sb += 3) {
        mmb(a0, sb);
        if (sb + 3 < S) ldb(a0, sb + 3);
        if (sb + 1 < S) { mmb(a1, sb + 1); if (sb + 4 < S) ldb(a1, sb + 4); }
        if (sb + 2 < S) { mmb(a2, sb + 2); if (sb + 5 < S) ldb(a2, sb + 5); }
    }
    fold();
}

// ---- V1 .. V4 (LOOK: look-ahead or none, CH: k-steps per chunk of B operands): the interior / partial split; rx is bounded to n x n floats
template <int LOOK, int CH>
__device__ __forceinline__ void var_new(float& v2a, float& v2b, __amdgpu_buffer_rsrc_t rx, int n, int j0A, int KA, int j0B, int KB,
                                        const float* Xs, int lane) {
    if (j0A < 0) return;
    const int i = lane & 15, kk = lane >> 4;
    const bool rvA = (j0A + i) < n, rvB = j0B >= 0 && (j0B + i) < n;
    const int offA = (j0A + i) * n + 4 * kk, offB = (j0B >= 0 ? j0B + i : 0) * n + 4 * kk;
    const float* xp = Xs + i;
    const float* xq = xp + 4 * kk * LD;
    const int ntA = (KA + 15) >> 4, ntB = j0B >= 0 ? (KB + 15) >> 4 : 0;
    const int SA = (ntA + 3) >> 2, SB = (ntB + 3) >> 2, S = SA + SB;
    vjf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    auto fold = [&]() {
        v2a = fmaf(acc0[0], acc0[0], fmaf(acc0[1], acc0[1], fmaf(acc0[2], acc0[2], fmaf(acc0[3], acc0[3], v2a))));
        v2b = fmaf(acc1[0], acc1[0], fmaf(acc1[1], acc1[1], fmaf(acc1[2], acc1[2], fmaf(acc1[3], acc1[3], v2b))));
    };
    auto ldb = [&](float4 (&a)[4], int sb) {
        const bool inB = sb >= SA;
        const int t0 = 4 * (inB ? sb - SA : sb), off = inB ? offB : offA;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int kq = 16 * (t0 + q) + 4 * kk; a[q] = vjf_ld4_sc1(rx, off + (kq + 3 < n ? 16 * (t0 + q) : 0)); }
    };
    auto mmb = [&](const float4 (&a)[4], int sb) {
        const bool inB = sb >= SA;
        const int t0 = 4 * (inB ? sb - SA : sb), nt = inB ? ntB : ntA, ke = inB ? KB : KA;
        const bool rv = inB ? rvB : rvA;
        if (sb == SA && SA > 0) {
            fold();
            acc0 = vjf_f32x4{0.f, 0.f, 0.f, 0.f}; acc1 = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const int nf = (ke >> 4) - t0;
        const float* xb = xq + 16 * t0 * LD;
        constexpr int NCH = 4 / CH;                                           // a step's B operands are read in NCH chunks of CH k-steps
        float b[2][2 * CH];
        auto rdb = [&](float (&bq)[2 * CH], int j) {
            const int q = j / NCH, c0 = (j % NCH) * CH;
#pragma unroll
            for (int c = 0; c < CH; ++c) { bq[2 * c] = xb[(16 * q + c0 + c) * LD]; bq[2 * c + 1] = xb[(16 * q + c0 + c) * LD + 16]; }
        };
        if (LOOK && nf > 0) rdb(b[0], 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < nf) {
                const float av[4] = {a[q].x, a[q].y, a[q].z, a[q].w};
#pragma unroll
                for (int h = 0; h < NCH; ++h) {
                    const int j = q * NCH + h;
                    if (LOOK) {
                        if (h + 1 < NCH) rdb(b[(j + 1) & 1], j + 1);
                        else if (q + 1 < 4 && q + 1 < nf) rdb(b[(j + 1) & 1], j + 1);
                    } else rdb(b[j & 1], j);
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[h * CH + c], b[j & 1][2 * c], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[h * CH + c], b[j & 1][2 * c + 1], acc1, 0, 0, 0);
                    }
                }
            } else if (t0 + q < nt) {
                const int k0 = 16 * (t0 + q) + 4 * kk;
                const float av[4] = {a[q].x, a[q].y, a[q].z, a[q].w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k = k0 + c, kc = min(k, ke - 1);
                    const float v = (rv && k < ke) ? av[c] : 0.f;
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(v, xp[kc * LD], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(v, xp[kc * LD + 16], acc1, 0, 0, 0);
                }
            }
        }
    };
    float4 a0[4], a1[4], a2[4];
    ldb(a0, 0);
    if (S > 1) ldb(a1, 1);
    if (S > 2) ldb(a2, 2);
    for (int sb = 0; sb < S; sb += 3) {
        mmb(a0, sb);
        if (sb + 3 < S) ldb(a0, sb + 3);
        if (sb + 1 < S) { mmb(a1, sb + 1); if (sb + 4 < S) ldb(a1, sb + 4); }
        if (sb + 2 < S) { mmb(a2, sb + 2); if (sb + 5 < S) ldb(a2, sb + 5); }
    }
    fold();
}

__host__ __device__ inline float phi_of(int k, int col) { return 0.05f + 0.9f * (float)((k * 37 + col * 11) % 101) / 101.f; }

template <int V>
__global__ __launch_bounds__(NT) void bench(const float* xt, float* out, unsigned long long* tks, int R, int n, int tri) {
    extern __shared__ float lds[];
    float* s_phi = lds; float* s_red = lds + NMAX * LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int e = tid; e < n * LD; e += NT) { const int k = e / LD, col = e - k * LD; s_phi[e] = col < TR ? phi_of(k, col) : 0.f; }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t r_xt = V == 0 ? vjf_rsrc(xt) : vjf_rsrc(xt, (size_t)n * n);
    const int ntile = (n + 15) >> 4;
    unsigned long long t0, t1;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");
    for (int it = 0; it < R; ++it) {
        float v2a = 0.f, v2b = 0.f;
        for (int r = 0; r * NW < ntile; r += 2) {              // the trial role's deal: tiles in descending cost, in a snake over the wavefronts
            int j0p[2], Kp[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int rr = r + h, idx = (rr & 1) ? rr * NW + NW - 1 - wave : rr * NW + wave;
                const int tt = ntile - 1 - idx;
                j0p[h] = (idx < ntile) ? tt * 16 : -1;
                Kp[h] = tri ? min(n, tt * 16 + 16) : n;
            }
            if (j0p[0] < 0) { j0p[0] = j0p[1]; Kp[0] = Kp[1]; j0p[1] = -1; }
            if (V == 0) var_v0(v2a, v2b, r_xt, n, j0p[0], Kp[0], j0p[1], Kp[1], s_phi, lane);
            if (V == 1) var_new<1, 4>(v2a, v2b, r_xt, n, j0p[0], Kp[0], j0p[1], Kp[1], s_phi, lane);
            if (V == 2) var_new<0, 4>(v2a, v2b, r_xt, n, j0p[0], Kp[0], j0p[1], Kp[1], s_phi, lane);
            if (V == 3) var_new<1, 2>(v2a, v2b, r_xt, n, j0p[0], Kp[0], j0p[1], Kp[1], s_phi, lane);
            if (V == 4) var_new<0, 2>(v2a, v2b, r_xt, n, j0p[0], Kp[0], j0p[1], Kp[1], s_phi, lane);
        }
        if (it == 0) { out[((size_t)blockIdx.x * NT + tid) * 2] = v2a; out[((size_t)blockIdx.x * NT + tid) * 2 + 1] = v2b; }
        v2a += __shfl_xor(v2a, 16, 64); v2a += __shfl_xor(v2a, 32, 64);
        v2b += __shfl_xor(v2b, 16, 64); v2b += __shfl_xor(v2b, 32, 64);
        if (lane < 16) { s_red[wave * TR + lane] = v2a; s_red[wave * TR + 16 + lane] = v2b; }
        __syncthreads();
        if (tid < TR) s_phi[((it * 7 + tid) % n) * LD + tid] += 1e-9f * s_red[tid];     // (a dependence between repetitions)
        __syncthreads();
    }
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");
    if (tid == 0) tks[blockIdx.x] = t1 - t0;
}

int main() {
    const int R = 2000, G = 128;
    float *out, *xt;
    unsigned long long* tk;
    hipMalloc(&out, (size_t)G * NT * 2 * 4); hipMalloc(&tk, G * 8); hipMalloc(&xt, (size_t)NMAX * NMAX * 4);
    const size_t lds = 100 * 1024;                             // (more than half a compute unit's: one workgroup per unit, as in the product)
    int bad = 0;
    std::vector<float> ref0((size_t)NT * 2), got((size_t)NT * 2), hx((size_t)NMAX * NMAX);
    const int shapes[4] = {200, 224, 196, 212};
    for (int si = 0; si < 4; ++si)
        for (int tri = 1; tri >= 0; --tri) {
            const int n = shapes[si];
            for (int j = 0; j < n; ++j)
                for (int k = 0; k < n; ++k) {
                    const float v = (float)(((j * 53 + k * 29) % 211) - 105) / 211.f / (1.f + 0.05f * (float)abs(j - k));
                    hx[(size_t)j * n + k] = (tri && k > j) ? 0.f : (j == k ? 1.f + fabsf(v) : v);
                }
            hipMemcpy(xt, hx.data(), (size_t)n * n * 4, hipMemcpyHostToDevice);
            std::vector<double> want(TR, 0.0);                 // the plain fp64 product
            const int ntile = (n + 15) / 16;
            for (int j = 0; j < n; ++j) {
                const int K = tri ? (16 * (j / 16) + 16 < n ? 16 * (j / 16) + 16 : n) : n;
                for (int col = 0; col < TR; ++col) {
                    double s = 0.0;
                    for (int k = 0; k < K; ++k) s += (double)hx[(size_t)j * n + k] * (double)phi_of(k, col);
                    want[col] += s * s;
                }
            }
            (void)ntile;
            auto run = [&](auto kern, int v, const char* name) {
                hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                hipMemset(out, 0xff, (size_t)G * NT * 2 * 4);
                hipLaunchKernelGGL(kern, dim3(G), dim3(NT), lds, 0, xt, out, tk, 1, n, tri);
                if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); exit(2); }
                hipMemcpy(got.data(), out, (size_t)NT * 2 * 4, hipMemcpyDeviceToHost);
                double worst = 0.0;
                for (int col = 0; col < TR; ++col) {
                    double s = 0.0;
                    for (int t = 0; t < NT; ++t) if ((t & 15) == (col & 15)) s += (double)got[(size_t)t * 2 + (col >> 4)];
                    worst = fmax(worst, fabs(s - want[col]) / fabs(want[col]));
                }
                int bits = 0;
                if (v == 0) ref0 = got;
                else bits = memcmp(ref0.data(), got.data(), (size_t)NT * 2 * 4) != 0;
                hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
                hipEventRecord(e0);
                hipLaunchKernelGGL(kern, dim3(G), dim3(NT), lds, 0, xt, out, tk, R, n, tri);
                hipEventRecord(e1); hipEventSynchronize(e1);
                float ms; hipEventElapsedTime(&ms, e0, e1);
                unsigned long long ticks[G]; hipMemcpy(ticks, tk, G * 8, hipMemcpyDeviceToHost);
                unsigned long long lo = ~0ull, hi = 0; for (int g = 0; g < G; ++g) { lo = ticks[g] < lo ? ticks[g] : lo; hi = ticks[g] > hi ? ticks[g] : hi; }
                const bool ok = worst < 2.0 * NMAX * 6e-8 && !bits;      // (fp32 sums of <= 224 terms, then squared: 2 K eps)
                bad += ok ? 0 : 1;
                printf("n %3d %-8s %-44s %7.3f us per phase   s_memtime ticks per phase, min / max over workgroups %7.1f / %7.1f   fp64 max rel err %.2e   %s\n",
                       n, tri ? "triangle" : "dense", name, ms * 1e3 / R, (double)lo / R, (double)hi / R, worst, v == 0 ? "(reference bits)" : (bits ? "BITS DIFFER from V0" : "bits equal to V0"));
            };
            run(bench<0>, 0, "V0 clamped and masked k-steps (the parent)");
            run(bench<1>, 1, "V1 full steps plain, look-ahead one step");
            run(bench<2>, 2, "V2 full steps plain, no look-ahead");
            run(bench<3>, 3, "V3 as V1 in half steps (4 + 4 registers)");
            run(bench<4>, 4, "V4 as V2 in half steps (4 registers)");
        }
    printf("(matrix-core floor at n = 200, triangle: 728 v_mfma_f32_16x16x4_f32 per tile, <= 104 per wavefront, two wavefronts per SIMD)\n");
    printf("%s\n", bad ? "FAILED" : "all variants ok");
    return bad ? 1 : 0;
}
