// vjf_host_tangent.h -- host side of vjf_tangent_rollout: the planner (pure arithmetic on the shapes and the overrides
// vjf_host_forecast.h reads), the forms of the kernel, one dispatch on them, and the one chunk loop.
// Included by vjf_abi.hip only, behind vjf_host_ctx.h (fail, allow_lds, kMaxLds) and vjf_host_forecast.h (fc_env_on, kFcMaxChunk).
#pragma once
#include "vjf_tangent_kernel.h"         // vjf_tangent_rollout_kernel

namespace {

// ---- planner.  The frame, the sums and one pass's partial products are in LDS beside the roll-out's buffers: `vg` tangent vectors per
//      pass, as many as fit (all m wherever the model dimensions are moderate; the bits do not depend on it).  cl: centroids and w_mean
//      in LDS (`cen_lds`: VJF_FC_CENTROID_LDS); la: w_mean's x-step operands in registers (`lookahead`: VJF_FC_LOOKAHEAD).
//      fits == false: the entry point refuses (dout beyond VJF_TG_MAXDOUT, or not one pass fits).
struct TgPlan { bool fits, cl, la; int vg; size_t lds; };
TgPlan tg_plan(int n, int d, int dout, int m, bool cen_lds, bool lookahead) {
    const size_t budget = kMaxLds - 1024;
    TgPlan p{};
    if (dout > VJF_TG_MAXDOUT) return p;
    p.cl = cen_lds && vjf_tangent_lds_floats(n, d, dout, m, m, true) * 4 <= budget;
    int vg = m;
    while (vg >= 1 && vjf_tangent_lds_floats(n, d, dout, m, vg, p.cl) * 4 > budget) --vg;
    if (vg < 1) return p;
    p.fits = true;
    p.vg = vg;
    p.la = p.cl && lookahead && vjf_fc_reg_form(n, dout);
    p.lds = vjf_tangent_lds_floats(n, d, dout, m, vg, p.cl) * 4;
    return p;
}
// Steps per launch: at most kFcMaxChunk, `chunk` (VJF_FC_CHUNK) asks for fewer; cut at interval boundaries wherever an interval is
// not longer than that (else inside it: the kernel is told how far the interval has come, the frame is not touched at a cut).
int tg_chunk(int qr, int chunk) {
    int c = chunk >= 1 && chunk < kFcMaxChunk ? chunk : kFcMaxChunk;
    if (qr > 0 && qr <= c) c = c / qr * qr;
    return c;
}

// f(NT, CL, NO) with the kernel's template arguments as std::integral_constant / std::bool_constant values: the x step's dispatch
// (with_fc_form) and NO, the tiles of 16 that cover dout (1, 2 or 4) -- in the register form that is NT itself, so NT is passed on
template <class F> void with_tg_form(const TgPlan& p, int dout, F&& f) {
    with_fc_form(p.la, p.cl, dout, [&](auto nt, auto cl) {
        if constexpr (decltype(nt)::value > 0) f(nt, cl, nt);
        else if (dout <= 16) f(nt, cl, std::integral_constant<int, 1>{});
        else if (dout <= 32) f(nt, cl, std::integral_constant<int, 2>{});
        else f(nt, cl, std::integral_constant<int, 4>{});
    });
}

// ---- the call behind its argument checks.  `a`: what the chunks share (u, c, logw, w, the outputs and the sizes, filled by the entry
//      point).  The state is carried from chunk to chunk through the output buffers: a chunk after the first starts from x_out, q_out
//      and lsum, which a workgroup reads (its own rows) before it writes them.
int tangent_run(VjfTgArgs a, const float* x0, const float* q0, int T, bool accumulate, const TgPlan& p, int chunk_override, hipStream_t s) {
    const int B = a.B, du = a.d - a.dout, tiles = (B + 15) / 16, step = tg_chunk(a.qr, chunk_override);
    const float* u = a.u;
    float* lhist = a.lhist;
    a.vg = p.vg;
    int t0 = 0;
    do {
        const int Tc = T - t0 < step ? T - t0 : step;
        a.x_in = t0 == 0 ? x0 : a.x_out;
        a.q_in = t0 == 0 ? q0 : a.q_out;
        a.lsum_in = t0 == 0 && !accumulate ? nullptr : a.lsum;
        a.u = u ? u + (size_t)t0 * B * du : nullptr;
        a.Tc = Tc; a.last = t0 + Tc == T;
        a.tq = a.qr > 0 ? t0 % a.qr : 0;
        a.lhist = lhist && a.qr > 0 ? lhist + (size_t)(t0 / a.qr) * B * a.m : nullptr;
        with_tg_form(p, a.dout, [&](auto nt, auto cl, auto no) {
            auto kernel = vjf_tangent_rollout_kernel<decltype(nt)::value, decltype(cl)::value, decltype(no)::value>;
            allow_lds(kernel, p.lds);
            hipLaunchKernelGGL(kernel, dim3(tiles), dim3(VJF_FC_THREADS), p.lds, s, a);
        });
        VJF_HIP(hipGetLastError());
        t0 += Tc;
    } while (t0 < T);
    return 0;
}

}  // namespace
