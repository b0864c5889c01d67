// Diagnostic micro-benchmark (not part of the product): the weight-gradient tiles of ONE trial workgroup (vjf_mega_trial.h, stage 6,
// stamp 19 -> 8 -> 9) at config B's shape -- 4096 trials' plan: d_y = 50, d_z = 10, RBF(200), hidden [128] -- with the trial role's own
// LDS layout (vjf_mega_trial_lds, [feature][33]), eight wavefronts, write-through stores into a late slab in memory, then the drain
// and the barrier in front of the count.  Both forms come from the library's headers:
//   V0  one loop per tensor (mg_slab_block, magic division, rotating start) around mg_grad_tile: the parent, 62 tiles
//   V1  mg_grad_walk<true>: the plan's tile table (vjf_mega_grad_tiles, scalar loads), the next tile's sixteen LDS reads in front of this
//       tile's chains and store; 61 tiles (the mean head's column tile that holds only the ones row stores nothing and is not listed)
//   V2  mg_grad_walk<false>: the table without the look-ahead
// and, to say where a tile's time goes (diagnostic only: their slabs are not V0's and are not compared), V2 changed in one respect:
//   D1  no store: the accumulators end in an empty asm
//   D2  operand reads without bank conflicts: lane l reads word l + 4 s of the tile's rows instead of row (l & 15), column (l >> 4) + 4 s
//   D3  both
// The slabs of V1 and V2 are compared BYTE FOR BYTE with V0's, for a first tile of a workgroup (plain store) and a later one
// (read-add-store), untouched padding included; V0 is checked against a plain fp64 product.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -o tools/grad_tile_bench tools/grad_tile_bench.hip && tools/grad_tile_bench
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../vjf_amd/csrc/vjf_mega_common.h"

constexpr int NT = VJF_MG_THREADS, NW = VJF_MG_WAVES, LD = VJF_MG_LD;

__host__ __device__ inline float lds_of(int e) { return (float)(((e * 37 + (e >> 5) * 11) % 201) - 100) / 128.f; }   // (exact in fp32)

// mg_grad_walk<false> with the store taken out (NOSTORE) and / or the reads made linear in the lane (LINEAR)
template <bool NOSTORE, bool LINEAR>
__device__ __forceinline__ void walk_diag(const int* table, int& q, const int qend, const float* smem, const int one, const int zero, float* late, const int lane) {
    mg_cst_i* tab = (mg_cst_i*)table + VJF_GT_HDR;
    mg_lds_cf* lds = (mg_lds_cf*)smem;
    const int i = lane & 15, kk = lane >> 4, row = LINEAR ? lane : i * LD + kk;
    for (; q < qend; q += NW) {
        const mg_i8 e = *(const mg_cst_i8*)(tab + VJF_GT_ENT * q);
        const int ao = i < e[1] ? e[0] + row : zero + (LINEAR ? 0 : kk);
        const int bo = i < e[3] ? e[2] + row : ((i == e[3] ? one : zero) + (LINEAR ? 0 : kk));
        float a[8], b[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) { a[s] = lds[ao + 4 * s]; b[s] = lds[bo + 4 * s]; }
        vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; s += 2) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s + 1], b[s + 1], acc1, 0, 0, 0);
        }
        acc += acc1;
        if (i < e[6] && 4 * kk < e[7]) {
            float* p = late + e[4] + i * e[5] + 4 * kk;
            if (NOSTORE) asm volatile("" ::"v"(p), "v"(acc) : "memory");
            else vjf_st4_wt(p, acc[0], acc[1], acc[2], acc[3]);
        }
    }
}

template <int V>
__global__ __launch_bounds__(NT) void bench(const VjfPlan P, const int* table, float* slab, unsigned long long* tks, int R, int first_i) {
    extern __shared__ float smem[];
    const VjfMegaTrialLds Lo = vjf_mega_trial_lds<false>(P);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool first = first_i != 0;
    for (int e = tid; e < Lo.total; e += NT) smem[e] = lds_of(e);
    __syncthreads();
    if (tid < LD) { smem[Lo.one + tid] = tid < VJF_MG_TR ? 1.f : 0.f; smem[Lo.zero + tid] = 0.f; }
    __syncthreads();
    float* s_one = smem + Lo.one; float* s_zero = smem + Lo.zero;
    const int dz = P.dz, dy = P.dy, hL = P.h[P.L - 1];
    const bool compact = dy >= P.hmax;
    float* s_d0 = compact ? smem + Lo.py : smem + Lo.dd;
    float* s_d1 = compact ? smem + Lo.dd : smem + Lo.dd + P.hmax * LD;
    const float* hact = smem + Lo.act + (P.hsum - hL) * LD;
    float* late = slab + (size_t)blockIdx.x * vjf_mega_slab_layout(P).len;
    unsigned long long dt_tiles = 0, dt_out = 0;
    for (int it = 0; it < R; ++it) {
        unsigned long long t0, t1, t2;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");
        if (V == 0) {
            int gbase = 0;
            auto grad_tensor = [&](const float* D, int M, const float* Bact, int Kin, int blkid) {
                int b_off, b_ldm, b_rows;
                mg_slab_block(P, blkid, b_off, b_ldm, b_rows);
                const int ntm = (M + 15) >> 4, ntj = (Kin + 1 + 15) >> 4;
                const unsigned mj = mg_magic(ntj);
                for (int q = (wave - gbase) & (NW - 1); q < ntm * ntj; q += NW) {
                    const int tm = mg_div(q, mj), tj = q - tm * ntj;
                    mg_grad_tile(D, M, tm * 16, Bact, Kin, tj * 16, s_one, s_zero, late + b_off, b_ldm, b_rows, first, lane);
                }
                gbase += ntm * ntj;
            };
            auto layer_grads = [&](int l, const float* da) {
                int aoff = 0;
                for (int q = 0; q < l - 1; ++q) aoff += P.h[q];
                grad_tensor(da, P.h[l], l > 0 ? smem + Lo.act + aoff * LD : smem + Lo.in, l > 0 ? P.h[l - 1] : P.din, 3 + (P.L - 1 - l));
            };
            grad_tensor(smem + Lo.dpy, dy, smem + Lo.xt, dz, 0);
            grad_tensor(smem + Lo.dmu, dz, hact, hL, 1);
            grad_tensor(smem + Lo.dlv, dz, hact, hL, 2);
            layer_grads(P.L - 1, s_d0);
            if (P.L >= 2) layer_grads(P.L - 2, s_d1);
        } else if (V >= 3) {
            int gq = wave;
            walk_diag<V == 3 || V == 5, V == 4 || V == 5>(table, gq, ((mg_cst_i*)table)[2], smem, Lo.one, Lo.zero, late, lane);
        } else {
            int gq = wave;
            mg_grad_walk<V == 1>(table, gq, ((mg_cst_i*)table)[2], smem, Lo.one, Lo.zero, late, first, lane);
        }
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // "slab out": every storing wavefront drains, the workgroup barrier
        __syncthreads();
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t2)::"memory");
        dt_tiles += t1 - t0; dt_out += t2 - t1;
        if (tid < VJF_MG_TR && R > 1) smem[Lo.dpy + ((it * 7 + tid) % dy) * LD + tid] += 1e-9f * (float)(it & 1);   // (a dependence between repetitions)
        __syncthreads();
    }
    if (lane == 0) { tks[(blockIdx.x * NW + wave) * 2] = dt_tiles; tks[(blockIdx.x * NW + wave) * 2 + 1] = dt_out; }
}

int main() {
    vjf_config cfg{};
    cfg.ydim = 50; cfg.xdim = 10; cfg.udim = 0; cfg.n_rbf = 200; cfg.n_hidden = 1; cfg.hidden[0] = 128;
    cfg.likelihood = VJF_LIK_GAUSSIAN; cfg.max_batch = 4096;
    VjfPlan P;
    if (vjf_make_plan(&cfg, &P)) { printf("bad plan\n"); return 2; }
    const VjfMegaTrialLds Lo = vjf_mega_trial_lds(P);
    const VjfMegaSlab SL = vjf_mega_slab_layout(P);
    std::vector<int> tab((size_t)vjf_mega_grad_tiles(P, nullptr));
    vjf_mega_grad_tiles(P, tab.data());
    const int R = 2000, G = 1, ntile_new = tab[0];
    int ntile_old = 0;
    {
        const int hL = P.h[P.L - 1];
        auto cnt = [&](int M, int Kin) { ntile_old += ((M + 15) >> 4) * ((Kin + 1 + 15) >> 4); };
        cnt(P.dy, P.dz); cnt(P.dz, hL); cnt(P.dz, hL);
        for (int l = P.L - 1; l >= 0; --l) cnt(P.h[l], l > 0 ? P.h[l - 1] : P.din);
    }
    int* d_tab; float* d_slab; unsigned long long* d_tk;
    hipMalloc(&d_tab, tab.size() * 4); hipMalloc(&d_slab, (size_t)G * SL.len * 4); hipMalloc(&d_tk, (size_t)G * NW * 2 * 8);
    hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    const size_t lds = (size_t)Lo.total * 4;
    printf("config B: %d tiles in the per-tensor loops, %d in the table; late slab %d floats; LDS %zu bytes\n", ntile_old, ntile_new, SL.len, lds);
    // the plain fp64 product of the first tile of a workgroup, from the same LDS image
    std::vector<double> want((size_t)SL.len, 0.0);
    std::vector<char> stored((size_t)SL.len, 0);
    {
        auto L = [&](int e) { return (double)lds_of(e); };
        auto blk = [&](int b, int D, int M, int Bact, int Kin) {
            for (int j = 0; j < SL.rows[b]; ++j)
                for (int m = 0; m < SL.ldm[b]; ++m) {
                    double s = 0.0;
                    if (m < M) for (int t = 0; t < VJF_MG_TR; ++t) s += L(D + m * LD + t) * (j < Kin ? L(Bact + j * LD + t) : 1.0);
                    want[(size_t)SL.off[b] + (size_t)j * SL.ldm[b] + m] = s; stored[(size_t)SL.off[b] + (size_t)j * SL.ldm[b] + m] = 1;
                }
        };
        const int hL = P.h[P.L - 1], hact = Lo.act + (P.hsum - hL) * LD;
        const bool compact = P.dy >= P.hmax;
        blk(0, Lo.dpy, P.dy, Lo.xt, P.dz); blk(1, Lo.dmu, P.dz, hact, hL); blk(2, Lo.dlv, P.dz, hact, hL);
        blk(3, compact ? Lo.py : Lo.dd, P.h[0], Lo.in, P.din);               // (one hidden layer)
    }
    int bad = 0;
    std::vector<float> ref[2], got((size_t)SL.len), seed((size_t)SL.len);
    for (int e = 0; e < SL.len; ++e) seed[e] = (float)((e * 13) % 97) / 64.f;
    auto run = [&](auto kern, int v, const char* name, int ntile) {
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        bool bits = true; double worst = 0.0;
        for (int first = 1; first >= 0; --first) {
            if (first) hipMemset(d_slab, 0xff, (size_t)SL.len * 4); else hipMemcpy(d_slab, seed.data(), (size_t)SL.len * 4, hipMemcpyHostToDevice);
            hipLaunchKernelGGL(kern, dim3(G), dim3(NT), lds, 0, P, d_tab, d_slab, d_tk, 1, first);
            if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); exit(2); }
            hipMemcpy(got.data(), d_slab, (size_t)SL.len * 4, hipMemcpyDeviceToHost);
            if (v == 0) {
                ref[first] = got;
                if (first) for (int e = 0; e < SL.len; ++e) if (stored[e]) worst = fmax(worst, fabs((double)got[e] - want[e]));
            } else if (v < 3) bits = bits && memcmp(ref[first].data(), got.data(), (size_t)SL.len * 4) == 0;
        }
        hipMemset(d_slab, 0, (size_t)SL.len * 4);
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        hipEventRecord(e0);
        hipLaunchKernelGGL(kern, dim3(G), dim3(NT), lds, 0, P, d_tab, d_slab, d_tk, R, 1);
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        unsigned long long tk[NW * 2]; hipMemcpy(tk, d_tk, sizeof(tk), hipMemcpyDeviceToHost);
        double tmax = 0, tmin = 1e30, omax = 0;
        for (int w = 0; w < NW; ++w) { tmax = fmax(tmax, (double)tk[2 * w] / R); tmin = fmin(tmin, (double)tk[2 * w] / R); omax = fmax(omax, (double)tk[2 * w + 1] / R); }
        // (fp32 sums of 32 products of magnitudes < 1: 32 x 2^-24 and the rounding of the sum)
        const bool ok = bits && (v != 0 || worst < 32 * 6e-8 * 2);
        bad += ok ? 0 : 1;
        printf("%-52s %7.3f us per repetition   s_memtime ticks: tiles min / max over wavefronts %7.1f / %7.1f (%6.1f per tile of the slowest), slab out %7.1f   %s\n",
               name, ms * 1e3 / R, tmin, tmax, tmax / ((ntile + NW - 1) / NW), omax,
               v == 0 ? (worst < 32 * 6e-8 * 2 ? "(reference bits; fp64 ok)" : "fp64 MISMATCH") : v >= 3 ? "(diagnostic: not compared)" : (bits ? "bytes equal to V0 (first and later tile)" : "BYTES DIFFER from V0"));
    };
    for (int rep = 0; rep < 2; ++rep) {
        run(bench<0>, 0, "V0 one loop per tensor, mg_grad_tile (the parent)", ntile_old);
        run(bench<1>, 1, "V1 tile table, next tile's reads ahead", ntile_new);
        run(bench<2>, 2, "V2 tile table, no look-ahead", ntile_new);
        run(bench<3>, 3, "D1 V2 without the store", ntile_new);
        run(bench<4>, 4, "D2 V2 with conflict-free operand reads", ntile_new);
        run(bench<5>, 5, "D3 V2 with neither store nor bank conflicts", ntile_new);
    }
    printf("(matrix cores: 8 v_mfma_f32_16x16x4_f32 per tile, 32 cycles each, two wavefronts per SIMD)\n");
    printf("%s\n", bad ? "FAILED" : "all variants ok");
    return bad ? 1 : 0;
}
