// vjf_act.h -- the activations of the recognition layers (vjf/recognition.py:17-24: `activation` is any module class; the
// reference default is Tanh).  One definition, shared by every route: the one-launch trial role (vjf_mega_kernel.h), the
// per-step matrix-core trial kernel (vjf_trial_mfma_kernel.h), the wide route's element-wise pass (vjf_trial_wide.h) and the
// stand-alone operator (vjf_recognition_kernel.h).
//
// The supported set is the activations whose derivative follows from the layer's OUTPUT h: every route keeps h (LDS, the ACT
// columns of the workspace) and never the pre-activation a.  Each derivative is the one torch's autograd uses for that module
// (threshold_backward on the result, leaky_relu_backward, elu_backward, softplus_backward, sigmoid_backward on the output,
// hardtanh_backward).  The Tanh kernels keep their own code (mg_tanh / tanhf, 1 - h^2): the functions below run only in the act
// kernels, which read `kind` from a kernel argument (uniform: every branch on it is a scalar branch).
//
// Exponentials and logarithms go through the hardware v_exp_f32 / v_log_f32 / v_rcp_f32 (each within 1 ulp; 8-cycle issues, and
// on this part a SIMD never overlaps VALU with MFMA work, so every instruction here is paid in the trial role's time).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vjf_hip.h"

// tanh for the recognition layers (recognition.py:31-42), branch-free: the library's tanhf is ~70 VALU instructions with both of its
// branches taken in every wavefront, eight calls per lane and layer -- 1.2 us of a 32-trial tile's 4.5-us layer on a part whose SIMDs
// run VALU and MFMA instructions one after the other.  |x| < 0.55: x + x^3 P(x^2), the odd series through
// x^15; else 1 - 2 / (e^{2|x|} + 1) on the hardware exp2 and reciprocal (within 1 ulp each): <= ~2-3 ulp of the result, <= 1.1e-7
// absolute (emulated against fp64 over [-12, 12]: 1.8 ulp with exact exp2 / division); saturates to +-1 beyond |x| ~ 9, NaN stays NaN.
__device__ __forceinline__ float mg_tanh(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_exp2f(ax * 2.885390081777927f);          // e^{2|x|}
    const float big = 1.f - 2.f * __builtin_amdgcn_rcpf(t + 1.f);
    const float z = x * x;
    float p = -1.4558343870513183e-3f;                                         // -929569/638512875
    p = fmaf(p, z, 3.5921280365724810e-3f);                                    // 21844/6081075
    p = fmaf(p, z, -8.8632355299021966e-3f);                                   // -1382/155925
    p = fmaf(p, z, 2.1869488536155203e-2f);                                    // 62/2835
    p = fmaf(p, z, -5.3968253968253971e-2f);                                   // -17/315
    p = fmaf(p, z, 1.3333333333333333e-1f);                                    // 2/15
    p = fmaf(p, z, -3.3333333333333331e-1f);                                   // -1/3
    const float small = fmaf(p * z, x, x);
    return ax < 0.55f ? small : copysignf(big, x);
}

// The activation of an act kernel, a by-value kernel argument (vjf_set_activation / vjf_recognition_forward_act validate it).
struct VjfAct {
    int kind;          // VJF_ACT_*
    float p0, p1;      // LeakyReLU: slope; ELU: alpha; Softplus: beta, threshold; Hardtanh: min_val, max_val
};

// e^x - 1 for x <= 0 (ELU's negative branch): x > -0.35 the series through x^8 (truncation < 6e-9 relative), else the hardware
// exp2 minus 1 (no cancellation there: |e^x - 1| > 0.29) -- <= ~2 ulp of the result.
__device__ __forceinline__ float vjf_expm1_neg(float x) {
    float p = 2.4801587301587302e-5f;                                          // 1/40320
    p = fmaf(p, x, 1.9841269841269841e-4f);                                    // 1/5040
    p = fmaf(p, x, 1.3888888888888889e-3f);                                    // 1/720
    p = fmaf(p, x, 8.3333333333333332e-3f);                                    // 1/120
    p = fmaf(p, x, 4.1666666666666664e-2f);                                    // 1/24
    p = fmaf(p, x, 1.6666666666666666e-1f);                                    // 1/6
    p = fmaf(p, x, 0.5f);
    const float small = fmaf(p * x, x, x);
    const float big = __builtin_amdgcn_exp2f(x * 1.4426950408889634f) - 1.f;
    return x > -0.35f ? small : big;
}

// forward: h = act(a)
//   Tanh       mg_tanh (above)
//   ReLU       a < 0 ? 0 : a                                  exact (NaN stays NaN, as torch.relu)
//   LeakyReLU  a > 0 ? a : s a                                exact up to the one rounding of s a
//   ELU        a > 0 ? a : alpha (e^a - 1)                    vjf_expm1_neg: <= ~2 ulp
//   Softplus   beta a > thr ? a : log1p(e^{beta a}) / beta    max(x, 0) + log1p(e^{-|x|}), x = beta a; log1p(t) = log(1+t) t / ((1+t) - 1)
//                                                             on the hardware log2 / rcp (exact 1+t cancels the rounding of 1+t): <= ~4 ulp
//   Sigmoid    1 / (1 + e^{-a})                               hardware exp2 + rcp: <= ~2 ulp for |a| < 8; the tail's relative error grows
//                                                             as |a| 2^-24 (the rounding of a log2(e)), 5e-6 at a = -80 where h ~ 2e-35
//   Hardtanh   a < lo ? lo : (a > hi ? hi : a)                exact (ReLU6: lo = 0, hi = 6)
__device__ __forceinline__ float vjf_act_fwd(int kind, float a, float p0, float p1) {
    switch (kind) {
        case VJF_ACT_RELU: return a < 0.f ? 0.f : a;
        case VJF_ACT_LEAKY_RELU: return a > 0.f ? a : p0 * a;
        case VJF_ACT_ELU: return a > 0.f ? a : p0 * vjf_expm1_neg(a);
        case VJF_ACT_SOFTPLUS: {
            const float x = a * p0;
            const float t = __builtin_amdgcn_exp2f(-fabsf(x) * 1.4426950408889634f);   // e^{-|x|} in (0, 1]
            const float u = 1.f + t, d = u - 1.f;
            const float l1p = d == 0.f ? t : __builtin_amdgcn_logf(u) * 0.6931471805599453f * t * __builtin_amdgcn_rcpf(d);
            const float sp = ((x > 0.f ? x : 0.f) + l1p) * __builtin_amdgcn_rcpf(p0);
            return x > p1 ? a : sp;
        }
        case VJF_ACT_SIGMOID: return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-a * 1.4426950408889634f));
        case VJF_ACT_HARDTANH: return a < p0 ? p0 : (a > p1 ? p1 : a);
        default: return mg_tanh(a);
    }
}

// derivative dh/da, from the output h
//   Tanh       1 - h^2
//   ReLU       h > 0                                          (threshold_backward on the result)
//   LeakyReLU  h > 0 ? 1 : s                                  (h > 0 <=> a > 0 for s >= 0)
//   ELU        h > 0 ? 1 : h + alpha                          (alpha e^a = h + alpha)
//   Softplus   1 - e^{-beta h}   (= sigmoid(beta a))          y = beta h < 0.35: the series y - y^2/2 + ... through y^8 (no cancellation),
//                                                             else 1 - hardware exp2: <= ~2 ulp; exactly 1 in fp32 once beta h > 17
//   Sigmoid    h (1 - h)
//   Hardtanh   lo < h < hi                                    (hardtanh_backward: 0 at the bounds)
__device__ __forceinline__ float vjf_act_dh(int kind, float h, float p0, float p1) {
    switch (kind) {
        case VJF_ACT_RELU: return h > 0.f ? 1.f : 0.f;
        case VJF_ACT_LEAKY_RELU: return h > 0.f ? 1.f : p0;
        case VJF_ACT_ELU: return h > 0.f ? 1.f : h + p0;
        case VJF_ACT_SOFTPLUS: return -vjf_expm1_neg(-p0 * h);
        case VJF_ACT_SIGMOID: return h * (1.f - h);
        case VJF_ACT_HARDTANH: return (h > p0 && h < p1) ? 1.f : 0.f;
        default: return 1.f - h * h;
    }
}
__device__ __forceinline__ float vjf_act_fwd(const VjfAct& f, float a) { return vjf_act_fwd(f.kind, a, f.p0, f.p1); }
__device__ __forceinline__ float vjf_act_dh(const VjfAct& f, float h) { return vjf_act_dh(f.kind, h, f.p0, f.p1); }
