// vjf_host_fixed_point.h -- host side of vjf_fixed_points: the planner (pure arithmetic on the shapes and the override
// vjf_host_forecast.h reads), the forms of the kernel and the one launch.
// Included by vjf_abi.hip only, behind vjf_host_ctx.h (fail, allow_lds, kMaxLds) and vjf_host_forecast.h (fc_env_on).
#pragma once
#include "vjf_fixed_point_kernel.h"     // vjf_fixed_point_kernel

namespace {

// ---- planner.  A (its place is the factor's between two evaluations), the triangle of M and one pass's partial products are in LDS
//      beside the x step's buffers: `vg` columns of A per pass, as many as fit (the bits do not depend on it).  cl: centroids and w_mean
//      in LDS (`cen_lds`: VJF_FC_CENTROID_LDS) wherever they fit beside a pass of one group of VJF_FP_MV columns -- a wavefront walks its
//      share of K once per group whatever vg is, so a smaller vg costs barriers only.  fits == false: the entry point refuses (dout beyond VJF_FP_MAXDOUT, or not one pass fits).
struct FpPlan { bool fits, cl; int vg; size_t lds; };
FpPlan fp_plan(int n, int d, int dout, bool cen_lds) {
    const size_t budget = kMaxLds - 1024;
    FpPlan p{};
    if (dout > VJF_FP_MAXDOUT) return p;
    p.cl = cen_lds && vjf_fixed_point_lds_floats(n, d, dout, dout < VJF_FP_MV ? dout : VJF_FP_MV, true) * 4 <= budget;
    int vg = dout;
    while (vg >= 1 && vjf_fixed_point_lds_floats(n, d, dout, vg, p.cl) * 4 > budget) --vg;
    if (vg < 1) return p;
    p.fits = true;
    p.vg = vg;
    p.lds = vjf_fixed_point_lds_floats(n, d, dout, vg, p.cl) * 4;
    return p;
}

// ---- the call behind its argument checks: one launch, a workgroup per tile of 16 trials
int fixed_point_run(VjfFpArgs a, const FpPlan& p, hipStream_t s) {
    const int tiles = (a.B + 15) / 16;
    a.vg = p.vg;
    auto launch = [&](auto cl, auto no) {
        auto kernel = vjf_fixed_point_kernel<decltype(cl)::value, decltype(no)::value>;
        allow_lds(kernel, p.lds);
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(VJF_FC_THREADS), p.lds, s, a);
    };
    auto with_no = [&](auto cl) {
        if (a.dout <= 16) launch(cl, std::integral_constant<int, 1>{});
        else launch(cl, std::integral_constant<int, 2>{});
    };
    if (p.cl) with_no(std::true_type{});
    else with_no(std::false_type{});
    VJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace
