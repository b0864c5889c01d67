// vjf_host_smooth.h -- host side of vjf_smooth: the planner (pure arithmetic on the shapes and the override vjf_host_forecast.h
// reads), the forms of the kernel and the one launch.
// Included by vjf_abi.hip only, behind vjf_host_ctx.h (fail, allow_lds, kMaxLds) and vjf_host_forecast.h (fc_env_on).
#pragma once
#include "vjf_smooth_kernel.h"     // vjf_smooth_kernel
#include "vjf_host_tile_forms.h"    // tile_plan_cl_vg, with_tile_form, launch_tile_form

namespace {

// ---- placement.  960 bytes of read-only data in front of .text.  The four kernels of this header add descriptors, symbols and notes to
//      the gfx950 code object, which moved the start of .text from 0x14c00 to 0x15800 -- every kernel of the library 3072 bytes further
//      on, at another offset inside its 4-KiB pages -- and the 200-step vjf_mega_kernel launch of bench.py, byte-identical code, ran 1.0
//      to 1.5 % longer for it.  With this array .text starts at 0x15c00, the parent's offset inside a page.  In one pass of alternating
//      runs the launch then took the parent's time, in the next it stayed 0.4 % above the parent's worst run in two runs of three
//      (profiles/smoother_ab.txt has every pass; llvm-readelf -S of the code object shows the address): the offset is part of the
//      cause, not all of it.  The array is never read.  A change that grows what lies in front of .text has to look at that address.
//      The four kernels of vjf_host_smooth_sample.h did so again (.text at 0x16900); 768 bytes more put it at 0x16c00, the same
//      offset inside a page (profiles/sampler_ab.txt).  The nine kernels of vjf_host_kstep.h: .text at 0x18800, 1024 bytes more put it
//      at 0x18c00 (profiles/kstep_ab.txt).  The eight kernels of vjf_host_ekf.h: .text at 0x1a500, 1792 bytes more put it at 0x1ac00
//      (profiles/ekf_ab.txt).  The eight kernels of vjf_host_laplace.h: .text at 0x1c500, 1792 bytes more put it at 0x1cc00
//      (profiles/laplace_ab.txt).
__device__ __attribute__((used)) const unsigned char vjf_text_pad[6336] = {1};

// ---- planner.  The dout x dout block, the two triangles and one pass's partial products are in LDS beside the x step's buffers.
//      cl: centroids and w_mean in LDS (`cen_lds`: VJF_FC_CENTROID_LDS) wherever they fit beside a pass of one group of VJF_FLOW_MV
//      columns of A; else they are read from global memory.  vg: columns of A per pass, as many as fit, down to 1 (the bits depend on
//      neither).  So every dout <= 24 with n <= 256 and d - dout <= 8 fits (the corner needs 125.5 KB with cl = false, vg = 1, and
//      takes vg = 5); without a control input dout = 24 fits beside n <= 753, dout = 28 beside n <= 360, dout = 30 beside n <= 141, and
//      the block and the triangles of dout = 32 (141 KB) leave no room for the x step whatever n is.  fits == false: the entry point
//      refuses (dout beyond VJF_SM_MAXDOUT, or not one pass fits).
struct SmPlan { bool fits, cl; int vg; size_t lds; };
SmPlan sm_plan(int n, int d, int dout, bool cen_lds) {
    SmPlan p{};
    if (dout > VJF_SM_MAXDOUT) return p;
    auto bytes = [&](int vg, bool cl) { return vjf_smooth_lds_floats(n, d, dout, vg, cl) * 4; };
    p.fits = tile_plan_cl_vg(dout, cen_lds, bytes, p.cl, p.vg);
    if (!p.fits) return p;
    p.lds = bytes(p.vg, p.cl);
    return p;
}

// ---- the call behind its argument checks: one launch, a workgroup per tile of 16 trials
int smooth_run(VjfSmArgs a, const SmPlan& p, hipStream_t s) {
    const int tiles = (a.B + 15) / 16;
    a.vg = p.vg;
    with_tile_form(p.cl, a.dout, [&](auto cl, auto no) {
        launch_tile_form(vjf_smooth_kernel<decltype(cl)::value, decltype(no)::value>, dim3(tiles), p.lds, s, a);
    });
    VJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace
