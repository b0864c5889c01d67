// vjf_host_tile_forms.h -- what the host sides of the kernels that walk a tile of 16 trials over the learned flow share
// (vjf_host_fixed_point.h, vjf_host_smooth.h, vjf_host_smooth_sample.h, vjf_host_ekf.h): the planner's loop and the dispatch on a
// kernel's forms.  Included behind vjf_host_ctx.h (kMaxLds) and a kernel header (vjf_flow_eval.h: VJF_FLOW_MV).
#pragma once
#include <type_traits>

namespace {
constexpr size_t kTileLdsBudget = kMaxLds - 1024;

// `bytes(vg, cl)`: the kernel's dynamic LDS with vg columns of A per pass and (cl) centroids and w_mean in LDS.  cl where `cen_lds`
// allows it and they fit beside a pass of one group of VJF_FLOW_MV columns -- a wavefront walks its share of K once per group whatever
// vg is, so a smaller vg costs barriers only -- then vg, as many columns as fit, down to 1.  False if not one column fits.
template <class Bytes>
bool tile_plan_cl_vg(int dout, bool cen_lds, Bytes bytes, bool& cl, int& vg) {
    cl = cen_lds && bytes(dout < VJF_FLOW_MV ? dout : VJF_FLOW_MV, true) <= kTileLdsBudget;
    vg = dout;
    while (vg >= 1 && bytes(vg, cl) > kTileLdsBudget) --vg;
    return vg >= 1;
}

// f(flag) with `b` as std::true_type / std::false_type
template <class F>
void with_flag(bool b, F f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
// f(CL, NO) with a kernel's template arguments as integral constants: centroids in LDS or not, one output tile of w_mean^T or two
template <class F>
void with_tile_form(bool cl, int dout, F f) {
    with_flag(cl, [&](auto c) {
        if (dout <= 16) f(c, std::integral_constant<int, 1>{});
        else f(c, std::integral_constant<int, 2>{});
    });
}
// one launch of a form: the cap on dynamic LDS raised to what the plan asks for
template <class K, class A>
void launch_tile_form(K kernel, dim3 grid, size_t lds, hipStream_t s, const A& a) {
    allow_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, grid, dim3(VJF_FC_THREADS), lds, s, a);
}
}  // namespace
