// vjf_host_fixed_point.h -- host side of vjf_fixed_points: the planner (pure arithmetic on the shapes and the override
// vjf_host_forecast.h reads), the forms of the kernel and the one launch.
// Included by vjf_abi.hip only, behind vjf_host_ctx.h (fail, allow_lds, kMaxLds) and vjf_host_forecast.h (fc_env_on).
#pragma once
#include "vjf_fixed_point_kernel.h"     // vjf_fixed_point_kernel
#include "vjf_host_tile_forms.h"        // tile_plan_cl_vg, with_tile_form, launch_tile_form

namespace {

// ---- planner.  A (its place is the factor's between two evaluations), the triangle of M and one pass's partial products are in LDS
//      beside the x step's buffers: `vg` columns of A per pass, as many as fit (the bits do not depend on it).  cl: centroids and w_mean
//      in LDS (`cen_lds`: VJF_FC_CENTROID_LDS) wherever they fit beside a pass of one group of VJF_FLOW_MV columns -- a wavefront walks its
//      share of K once per group whatever vg is, so a smaller vg costs barriers only.  fits == false: the entry point refuses (dout beyond VJF_FP_MAXDOUT, or not one pass fits).
struct FpPlan { bool fits, cl; int vg; size_t lds; };
FpPlan fp_plan(int n, int d, int dout, bool cen_lds) {
    FpPlan p{};
    if (dout > VJF_FP_MAXDOUT) return p;
    auto bytes = [&](int vg, bool cl) { return vjf_fixed_point_lds_floats(n, d, dout, vg, cl) * 4; };
    p.fits = tile_plan_cl_vg(dout, cen_lds, bytes, p.cl, p.vg);
    if (!p.fits) return p;
    p.lds = bytes(p.vg, p.cl);
    return p;
}

// ---- the call behind its argument checks: one launch, a workgroup per tile of 16 trials
int fixed_point_run(VjfFpArgs a, const FpPlan& p, hipStream_t s) {
    const int tiles = (a.B + 15) / 16;
    a.vg = p.vg;
    with_tile_form(p.cl, a.dout, [&](auto cl, auto no) {
        launch_tile_form(vjf_fixed_point_kernel<decltype(cl)::value, decltype(no)::value>, dim3(tiles), p.lds, s, a);
    });
    VJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace
