// vjf_host_ekf.h -- host side of vjf_ekf: the planner (pure arithmetic on the shapes and two overrides: VJF_FC_CENTROID_LDS, which
// vjf_host_forecast.h reads, and VJF_EKF_DECODER_LDS), the forms of the kernel and the one launch.
// Included by vjf_abi.hip only, behind vjf_host_ctx.h (fail, allow_lds, kMaxLds) and vjf_host_forecast.h (fc_env_on).
#pragma once
#include "vjf_ekf_kernel.h"        // vjf_ekf_kernel
#include "vjf_host_tile_forms.h"    // tile_plan_cl_vg, with_tile_form, with_flag, launch_tile_form

namespace {

// ---- planner.  The dout x dout block, the three triangles and one pass's partial products are in LDS beside the x step's buffers.
//      cl: centroids and w_mean in LDS (`cen_lds`: VJF_FC_CENTROID_LDS) wherever they fit beside a pass of one group of VJF_FLOW_MV
//      columns of A; else they are read from global memory.  vg: columns of A per pass, as many as fit, down to 1.  dl: the decoder
//      in LDS, twice (k-major for the decodes, j-major for C^T v), where it fits beside all that (`dec_lds`: VJF_EKF_DECODER_LDS);
//      else it is read from global memory, so dy bounds nothing.  The bits depend on none of the three.
//      So every dout <= 24 with n <= 256 and d - dout <= 8 fits whatever dy is (the corner needs 144.3 KiB with cl = dl = false,
//      vg = 1, and takes vg = 2: 152.8 KiB); dout = 28 does not fit even beside n = 40, and the block and the triangles of
//      dout = 32 alone are 173 KiB.
//      fits == false: the entry point refuses (dout beyond VJF_EKF_MAXDOUT, or not one pass fits).
struct EkfPlan { bool fits, cl, dl; int vg; size_t lds; };
EkfPlan ekf_plan(int n, int d, int dout, int dy, bool cen_lds, bool dec_lds) {
    EkfPlan p{};
    if (dout > VJF_EKF_MAXDOUT) return p;
    auto bytes = [&](int vg, bool cl, bool dl) { return vjf_ekf_lds_floats(n, d, dout, dy, vg, cl, dl) * 4; };
    p.fits = tile_plan_cl_vg(dout, cen_lds, [&](int vg, bool cl) { return bytes(vg, cl, false); }, p.cl, p.vg);
    if (!p.fits) return p;
    p.dl = dec_lds && bytes(p.vg, p.cl, true) <= kTileLdsBudget;
    p.lds = bytes(p.vg, p.cl, p.dl);
    return p;
}

// ---- the call behind its argument checks: one launch, a workgroup per tile of 16 trials
int ekf_run(VjfEkfArgs a, const EkfPlan& p, hipStream_t s) {
    const int tiles = (a.B + 15) / 16;
    a.vg = p.vg;
    with_tile_form(p.cl, a.dout, [&](auto cl, auto no) {
        with_flag(p.dl, [&](auto dl) {
            launch_tile_form(vjf_ekf_kernel<decltype(cl)::value, decltype(no)::value, decltype(dl)::value>, dim3(tiles), p.lds, s, a);
        });
    });
    VJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace
