// vjf_host_kstep.h -- host side of vjf_kstep_score: the planner (pure arithmetic on the shapes and the overrides
// vjf_host_forecast.h reads, plus VJF_KS_CHUNK), the forms of the tile kernel, one dispatch on them, and the one chunk loop.
// Included by vjf_abi.hip only, behind vjf_host_ctx.h (fail, allow_lds, kMaxLds) and vjf_host_forecast.h (fc_env_on, fc_env_int,
// with_fc_form, kFeStateBytes).
#pragma once
#include "vjf_kstep_kernel.h"           // vjf_kstep_tile_kernel, vjf_kstep_fold_kernel

namespace {

// ---- planner.  cl: centroids in LDS, dl: the decoder in LDS (`cen_lds`: VJF_FC_CENTROID_LDS switches both off), the centroids first
//      (every feature of every step reads them, the decoder is read once per horizon); la: w_mean's x-step operands in registers
//      (`lookahead`: VJF_FC_LOOKAHEAD), where fc_forms takes that form.  fits == false: the entry point refuses.
//      Tiles run in chunks whose partials ((K + 1)(2 dout + 2 dy) floats per tile) stay within kKsPartBytes, at least one tile;
//      `chunk` (VJF_KS_CHUNK) asks for fewer tiles per chunk.  The fold is sequential in tile order: the bits do not depend on it.
constexpr size_t kKsPartBytes = kFeStateBytes;          // 32 MiB, the ensemble's state cap
struct KsPlan { bool fits, cl, la, dl; size_t lds; long long tiles, per_chunk; size_t elems, acc_bytes; };
KsPlan ks_plan(int T, int B, int K, int n, int d, int dout, int dy, bool cen_lds, bool lookahead, int chunk) {
    const size_t budget = kMaxLds - 1024;
    KsPlan p{};
    p.fits = vjf_ks_lds_floats(n, d, dout, dy, false, false) * 4 <= budget;
    p.cl = cen_lds && vjf_ks_lds_floats(n, d, dout, dy, true, false) * 4 <= budget;
    p.dl = cen_lds && dy > 0 && vjf_ks_lds_floats(n, d, dout, dy, p.cl, true) * 4 <= budget;
    p.la = p.cl && lookahead && vjf_fc_reg_form(n, dout);
    p.lds = vjf_ks_lds_floats(n, d, dout, dy, p.cl, p.dl) * 4;
    p.tiles = ((long long)T * B + 15) / 16;
    p.elems = (size_t)(K + 1) * (2 * (size_t)dout + 2 * (size_t)dy);
    long long per = (long long)(kKsPartBytes / (p.elems * 4));
    if (per < 1) per = 1;
    if (per > p.tiles) per = p.tiles;
    if (chunk >= 1 && chunk < per) per = chunk;
    p.per_chunk = per;
    p.acc_bytes = (p.elems * 8 + 255) / 256 * 256;
    return p;
}
// [fp64 accumulators] [partials of a chunk], whatever VJF_KS_CHUNK asks for
size_t ks_scratch_bytes(int T, int B, int K, int dout, int dy) {
    const KsPlan p = ks_plan(T, B, K, 1, dout, dout, dy, false, false, 0);
    return p.acc_bytes + ((size_t)p.per_chunk * p.elems * 4 + 255) / 256 * 256;
}

// f(NT, CL, DL): the x step's dispatch (with_fc_form) and the decoder's place
template <class F> void with_ks_form(const KsPlan& p, int dout, F&& f) {
    with_fc_form(p.la, p.cl, dout, [&](auto nt, auto cl) {
        if (p.dl) f(nt, cl, std::true_type{});
        else f(nt, cl, std::false_type{});
    });
}

// ---- the call behind its argument checks.  `a`: what the chunks share (filled by the entry point); `f`: the outputs.
int kstep_run(VjfKsArgs a, VjfKsFoldArgs f, void* scratch, const KsPlan& p, hipStream_t s) {
    f.acc = (double*)scratch;
    a.part = (float*)((char*)scratch + p.acc_bytes);
    f.part = a.part;
    f.E = (int)p.elems; f.ncol = 2 * a.dout + 2 * a.dy; f.dout = a.dout; f.dy = a.dy;
    for (long long t0 = 0; t0 < p.tiles; t0 += p.per_chunk) {
        const long long tc = p.tiles - t0 < p.per_chunk ? p.tiles - t0 : p.per_chunk;
        a.tile0 = t0;
        with_ks_form(p, a.dout, [&](auto nt, auto cl, auto dl) {
            auto kernel = vjf_kstep_tile_kernel<decltype(nt)::value, decltype(cl)::value, decltype(dl)::value>;
            allow_lds(kernel, p.lds);
            hipLaunchKernelGGL(kernel, dim3((unsigned)tc), dim3(VJF_FC_THREADS), p.lds, s, a);
        });
        VJF_HIP(hipGetLastError());
        f.tiles = tc; f.first = t0 == 0; f.last = t0 + tc == p.tiles;
        hipLaunchKernelGGL(vjf_kstep_fold_kernel, dim3((unsigned)((p.elems + 255) / 256)), dim3(256), 0, s, f);
        VJF_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace
