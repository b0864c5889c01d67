// vjf_host_ekf.h -- host side of vjf_ekf: the planner (pure arithmetic on the shapes and two overrides: VJF_FC_CENTROID_LDS, which
// vjf_host_forecast.h reads, and VJF_EKF_DECODER_LDS), the forms of the kernel and the one launch.
// Included by vjf_abi.hip only, behind vjf_host_ctx.h (fail, allow_lds, kMaxLds) and vjf_host_forecast.h (fc_env_on).
#pragma once
#include "vjf_ekf_kernel.h"        // vjf_ekf_kernel

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
    const size_t budget = kMaxLds - 1024;
    EkfPlan p{};
    if (dout > VJF_EKF_MAXDOUT) return p;
    p.cl = cen_lds && vjf_ekf_lds_floats(n, d, dout, dy, dout < VJF_FLOW_MV ? dout : VJF_FLOW_MV, true, false) * 4 <= budget;
    int vg = dout;
    while (vg >= 1 && vjf_ekf_lds_floats(n, d, dout, dy, vg, p.cl, false) * 4 > budget) --vg;
    if (vg < 1) return p;
    p.fits = true;
    p.vg = vg;
    p.dl = dec_lds && vjf_ekf_lds_floats(n, d, dout, dy, vg, p.cl, true) * 4 <= budget;
    p.lds = vjf_ekf_lds_floats(n, d, dout, dy, vg, p.cl, p.dl) * 4;
    return p;
}

// ---- the call behind its argument checks: one launch, a workgroup per tile of 16 trials
int ekf_run(VjfEkfArgs a, const EkfPlan& p, hipStream_t s) {
    const int tiles = (a.B + 15) / 16;
    a.vg = p.vg;
    auto launch = [&](auto cl, auto no, auto dl) {
        auto kernel = vjf_ekf_kernel<decltype(cl)::value, decltype(no)::value, decltype(dl)::value>;
        allow_lds(kernel, p.lds);
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(VJF_FC_THREADS), p.lds, s, a);
    };
    auto with_dl = [&](auto cl, auto no) {
        if (p.dl) launch(cl, no, std::true_type{});
        else launch(cl, no, std::false_type{});
    };
    auto with_no = [&](auto cl) {
        if (a.dout <= 16) with_dl(cl, std::integral_constant<int, 1>{});
        else with_dl(cl, std::integral_constant<int, 2>{});
    };
    if (p.cl) with_no(std::true_type{});
    else with_no(std::false_type{});
    VJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace
