// vjf_host_laplace.h -- host side of vjf_laplace_filter: the planner (pure arithmetic on the shapes and two overrides:
// VJF_FC_CENTROID_LDS, which vjf_host_forecast.h reads, and VJF_LAPLACE_DECODER_LDS), the forms of the kernel and the one launch.
// Included by vjf_abi.hip only, behind vjf_host_ctx.h (fail, allow_lds, kMaxLds) and vjf_host_forecast.h (fc_env_on).
#pragma once
#include "vjf_laplace_kernel.h"     // vjf_laplace_kernel
#include "vjf_host_tile_forms.h"    // tile_plan_cl_vg, with_tile_form, with_flag, launch_tile_form

namespace {

// ---- planner.  The EKF's buffers (the dout x dout block, the three triangles, one pass's partial products) with seven vectors in the
//      place of three and a second set of sixteen partial sums.  cl, vg and dl as in ekf_plan (`dec_lds`: VJF_LAPLACE_DECODER_LDS):
//      centroids and w_mean in LDS where they fit beside a pass of one group of columns of A, then as many columns per pass as fit,
//      then the decoder in LDS, twice, where it fits beside all that; else it is read from global memory, so dy bounds nothing.  The
//      bits depend on none of the three.
//      Every dout <= 16 with n <= 256 and d - dout <= 8 fits whatever dy is (the corner needs 82.8 KiB with cl = dl = false and
//      vg = 1); dout = 24 fits up to n = 256 with eight control inputs as well (149.5 KiB at vg = 1).  dout > VJF_LAP_MAXDOUT = 24 is
//      refused: a wavefront holds at most five tiles of pair rows.
//      fits == false: the entry point refuses (dout beyond VJF_LAP_MAXDOUT, or not one pass fits).
struct LapPlan { bool fits, cl, dl; int vg; size_t lds; };
LapPlan lap_plan(int n, int d, int dout, int dy, bool cen_lds, bool dec_lds) {
    LapPlan p{};
    if (dout > VJF_LAP_MAXDOUT) return p;
    auto bytes = [&](int vg, bool cl, bool dl) { return vjf_lap_lds_floats(n, d, dout, dy, vg, cl, dl) * 4; };
    p.fits = tile_plan_cl_vg(dout, cen_lds, [&](int vg, bool cl) { return bytes(vg, cl, false); }, p.cl, p.vg);
    if (!p.fits) return p;
    p.dl = dec_lds && bytes(p.vg, p.cl, true) <= kTileLdsBudget;
    p.lds = bytes(p.vg, p.cl, p.dl);
    return p;
}

// ---- the call behind its argument checks: one launch, a workgroup per tile of 16 trials
int lap_run(VjfLapArgs a, const LapPlan& p, hipStream_t s) {
    const int tiles = (a.B + 15) / 16;
    a.vg = p.vg;
    with_tile_form(p.cl, a.dout, [&](auto cl, auto no) {
        with_flag(p.dl, [&](auto dl) {
            launch_tile_form(vjf_laplace_kernel<decltype(cl)::value, decltype(no)::value, decltype(dl)::value>, dim3(tiles), p.lds, s, a);
        });
    });
    VJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace
