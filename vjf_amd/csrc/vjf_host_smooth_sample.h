// vjf_host_smooth_sample.h -- host side of vjf_smooth_sample: the planner (pure arithmetic on the shapes and the two overrides), the
// forms of the kernel and the one launch.
// Included by vjf_abi.hip only, behind vjf_host_ctx.h (fail, allow_lds, kMaxLds), vjf_host_forecast.h (fc_env_on, fc_env_int) and
// vjf_host_smooth.h (sm_plan).
#pragma once
#include "vjf_smooth_sample_kernel.h"     // vjf_smooth_sample_kernel
#include "vjf_host_tile_forms.h"           // kTileLdsBudget, with_tile_form, launch_tile_form

namespace {

// ---- planner.  Beside the x step's buffers: the dout x dout block, one triangle, one pass's partial products and the two member
//      buffers of SC members (vjf_sms_member_floats each).  In this order:
//      SC   the largest number of members <= S that fits beside one group of min(dout, VJF_FLOW_MV) columns of A with the shared
//           operands in global memory (`members` > 0, VJF_SMS_MEMBERS, forces a smaller one); where not even one member fits beside
//           a group the group shrinks down to one column;
//      cl   centroids and w_mean in LDS (`cen_lds`: VJF_FC_CENTROID_LDS) if they fit beside that;
//      vg   columns of A per pass, as many as still fit.
//      A member's bits depend on none of the three.  The shapes accepted are exactly those sm_plan accepts, each with SC >= 1: the
//      kernel has one triangle and two vectors fewer than the smoother's, and one member costs less than that at every dout
//      (17 dout (dout + 1) / 2 + 34 dout floats against 4 ((9 dout) | 1)).  dout = 32 beside a small n would fit this kernel alone; it
//      is refused with the smoother so that wherever draws exist their row moments can be had from vjf_smooth.  fits == false: the
//      entry point refuses.
struct SmsPlan { bool fits, cl; int vg, sc; size_t lds; };
SmsPlan sms_plan(int n, int d, int dout, int S, bool cen_lds, int members = 0) {
    const size_t budget = kTileLdsBudget;
    SmsPlan p{};
    if (dout > VJF_SMS_MAXDOUT || S < 1 || !sm_plan(n, d, dout, cen_lds).fits) return p;
    auto bytes = [&](int vg, int sc, bool cl) { return vjf_sms_lds_floats(n, d, dout, vg, sc, cl) * 4; };
    int vg = dout < VJF_FLOW_MV ? dout : VJF_FLOW_MV;
    while (vg >= 1 && bytes(vg, 1, false) > budget) --vg;
    if (vg < 1) return p;
    const size_t per = 2 * vjf_sms_member_floats(dout) * 4;
    size_t room = (budget - bytes(vg, 1, false)) / per + 1;
    int sc = room < (size_t)S ? (int)room : S;
    if (members > 0 && members < sc) sc = members;
    p.cl = cen_lds && bytes(vg, sc, true) <= budget;
    while (vg < dout && bytes(vg + 1, sc, p.cl) <= budget) ++vg;
    p.fits = true;
    p.vg = vg;
    p.sc = sc;
    p.lds = bytes(vg, sc, p.cl);
    return p;
}

// ---- the call behind its argument checks: one launch, a workgroup per tile of 16 trials and chunk of SC members
int smooth_sample_run(VjfSmsArgs a, const SmsPlan& p, hipStream_t s) {
    const int tiles = (a.B + 15) / 16, chunks = (a.S + p.sc - 1) / p.sc;
    a.vg = p.vg;
    a.sc = p.sc;
    with_tile_form(p.cl, a.dout, [&](auto cl, auto no) {
        launch_tile_form(vjf_smooth_sample_kernel<decltype(cl)::value, decltype(no)::value>, dim3(tiles, chunks), p.lds, s, a);
    });
    VJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace
