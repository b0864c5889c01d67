// vjf_step_math.h -- the scalar formulas of one VJF.filter step, each written once for every filter route.
//
// Values in, values out: no pointer into the state, no load and no store (vjf_put_loss4 apart, which writes the four numbers a
// caller hands it a place for).  The call sites keep their own accessors (plain, vjf_ld_sc1, vjf_st_wt, atomics), their reduction
// shapes and their masks; the reference citations live here.  The kernels are compiled with contraction on: an expression keeps
// its shape inside a function, and a caller adds nothing between a product and the sum that takes it.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_plan.h"

// ------------------------------------------------------------------------------------------------ loss, finite guards
// The step's loss from the three sums over the trials (model.py:124-154).  A component that is not finite is replaced by 0 and
// drops out of the reference's graph (model.py:138-145); loss = l_recon - entropy (+ l_dynamics outside warm-up, model.py:146-149).
struct VjfLossVerdict {
    float l_recon, l_dyn, ent, loss;      // the three means, 0 where they were not finite, and the loss
    bool ok_r, ok_d, ok_h, warm;          // finite?
    // every component IN the loss is finite: the gradient sums are the reference's
    __device__ __forceinline__ bool grad_ok() const { return ok_r && ok_h && (warm || ok_d); }
    // some, not all, of the components in the loss are non-finite: the reference steps along the gradient of the others
    // (all of them: its gradient is zero and optimizer.step() moves nothing, model.py:206-214)
    __device__ __forceinline__ bool partial(bool do_sgd) const { return do_sgd && !grad_ok() && (ok_r || ok_h || (!warm && ok_d)); }
    // the components a replay of the backward half leaves out: bit 0 recon, 1 dynamics, 2 entropy
    __device__ __forceinline__ unsigned dropped() const { return (ok_r ? 0u : 1u) | (ok_d ? 0u : 2u) | (ok_h ? 0u : 4u); }
    __device__ __forceinline__ unsigned status() const {
        return (ok_r ? 0u : VJF_STATUS_NONFINITE_RECON) | (ok_d ? 0u : VJF_STATUS_NONFINITE_DYN) | (ok_h ? 0u : VJF_STATUS_NONFINITE_ENT);
    }
};
__device__ __forceinline__ VjfLossVerdict vjf_loss_verdict(float sum_recon, float sum_dyn, float sum_ent, float invB, bool warm) {
    VjfLossVerdict v;
    v.l_recon = sum_recon * invB; v.l_dyn = sum_dyn * invB; v.ent = sum_ent * invB;
    v.ok_r = isfinite(v.l_recon); v.ok_d = isfinite(v.l_dyn); v.ok_h = isfinite(v.ent);
    v.warm = warm;
    if (!v.ok_r) v.l_recon = 0.f;
    if (!v.ok_d) v.l_dyn = 0.f;
    if (!v.ok_h) v.ent = 0.f;
    v.loss = warm ? v.l_recon - v.ent : v.l_recon - v.ent + v.l_dyn;
    return v;
}
// (loss, log-likelihood, dynamics term, entropy) as VJF.filter returns them
__device__ __forceinline__ void vjf_put_loss4(float* l4, const VjfLossVerdict& v) {
    l4[0] = v.loss; l4[1] = -v.l_recon; l4[2] = -v.l_dyn; l4[3] = v.ent;
}

// When the likelihood log-variance rho takes its gradient step (its gradient comes from the reconstruction term alone).  Three
// conditions, one per family of routes, kept as they have been -- changing one is a change of behaviour:
//   vjf_serial_kernel (serial, Kalman and sharded routes):            do_sgd && v.grad_ok()
//       any non-finite component in the loss skips the whole SGD step, rho with it; these routes have no replay.
//   vjf_prep_kernel (multi-launch RLS, wide, one- and three-stream):  do_sgd && (v.grad_ok() || (replay && v.ok_r))
//       replay = a replay buffer is there && v.partial(do_sgd): rho steps with the replayed parameters; without a replay buffer as
//       the serial kernel.
//   SGD role of the one-launch route (vjf_mega_sgd.h):                do_sgd && ok_r
//       also when every component in the loss but the reconstruction term is non-finite (the parameters then wait for the replay).

// ------------------------------------------------------------------------------------------------ clip + SGD
__device__ __forceinline__ float vjf_clip1(float g) { return fminf(fmaxf(g, -1.f), 1.f); }          // clip_grad_value_(.., 1.0), model.py:210
// optimizer.step() on the batch-mean gradient gsum / B (model.py:210-211)
__device__ __forceinline__ float vjf_sgd_step(float w, float gsum, float invB, float lr) {
    const float g = vjf_clip1(gsum * invB);
    return w - lr * g;
}
// the clipped gradient of the Gaussian likelihood's log-variance: d/d rho of mean_b sum_i 0.5 ((y - py)^2 exp(-rho) + rho)
__device__ __forceinline__ float vjf_rho_grad(int dy, float rho, float sse_y, float invB) {
    return vjf_clip1(0.5f * ((float)dy - expf(-rho) * sse_y * invB));
}

// ------------------------------------------------------------------------------------------------ running variances
#define VJF_LIK_VAR_CAP 1000.f            // running_var's default size_cap (likelihood.py:28-40)
#define VJF_TR_VAR_CAP 500.f              // running_var(.., size_cap=500), the state noise (model.py:370-377)
// running_var in the log domain: the old variance weighs min(n_acc, cap) samples, the step's mean square Bf; tot = the new count
__device__ __forceinline__ float vjf_running_logvar(float logvar, float n_acc, float cap, float Bf, float mse, float& tot) {
    const float acc = fminf(n_acc, cap);
    tot = acc + Bf;
    return logf((acc / tot) * expf(logvar) + (Bf / tot) * mse);
}
// the same in two halves, for a caller that has the old variance long before the mean square (vjf_post_kernel.h)
__device__ __forceinline__ float vjf_running_old_share(float logvar, float n_acc, float cap, float Bf, float& tot) {
    const float acc = fminf(n_acc, cap);
    tot = acc + Bf;
    return (acc / tot) * expf(logvar);
}
__device__ __forceinline__ float vjf_running_logvar_split(float old_share, float tot, float Bf, float mse) { return logf(old_share + (Bf / tot) * mse); }
// mean square of the residual dx - Phi W from its fp64 sum t over B trials (model.py:373-374); a quadratic form may round below 0
__device__ __forceinline__ float vjf_resid_mse(double t, float Bf, int dz) {
    if (t < 0.0) t = 0.0;
    return (float)(t / ((double)Bf * (double)dz));
}

// ------------------------------------------------------------------------------------------------ per-element loss terms, seeds
// The forward halves alone, for the stand-alone loss operator (vjf_loss_kernel).  The element functions of the filter step below
// hold the same expressions in their own bodies: calling these from there costs vjf_mega_lite_act_kernel lane spills
// (profiles/step_math_isa.txt).
// gaussian_loss of one element with a shared log-variance lv, p = exp(-lv / 2), without the trace (functional.py:54-73)
__device__ __forceinline__ float vjf_gauss_nll(float a, float b, float p, float lv) {
    const float dsc = a * p - b * p;
    return 0.5f * (dsc * dsc + lv);
}
__device__ __forceinline__ float vjf_entropy_term(float lv) { return 0.5f * lv; }                   // gaussian_entropy, functional.py:25-29
#define VJF_POISSON_ETA_MAX 10.f          // the Poisson likelihood's clamp of the log-rate (likelihood.py:51-62)
__device__ __forceinline__ float vjf_poisson_eta(float pv) { return fminf(pv, VJF_POISSON_ETA_MAX); }
__device__ __forceinline__ float vjf_poisson_nll(float yv, float eta, float ex) { return ex - yv * eta; }   // ex = exp(eta)

// One element of the reconstruction term, Gaussian likelihood (likelihood.py:19-26): p = exp(-rho / 2), e = exp(-rho).  Adds the
// element's loss to lrec and its squared residual to ssey; returns the seed d l / d py (no 1/B).
__device__ __forceinline__ float vjf_gauss_recon(float yv, float pv, float rho, float p, float e, float& lrec, float& ssey) {
    const float r = pv - yv, dsc = yv * p - pv * p;
    lrec += 0.5f * (dsc * dsc + rho);
    ssey = fmaf(r, r, ssey);
    return e * r;
}
// The same for the Poisson likelihood (likelihood.py:51-62); no gradient where the clamp holds.
__device__ __forceinline__ float vjf_poisson_recon(float yv, float pv, float& lrec, float& ssey) {
    const float eta = fminf(pv, VJF_POISSON_ETA_MAX), ex = expf(eta);
    lrec += ex - yv * eta;
    const float r = pv - yv;
    ssey = fmaf(r, r, ssey);
    return pv <= VJF_POISSON_ETA_MAX ? ex - yv : 0.f;
}
// One element of the dynamics term and of the entropy (model.py:390-391, functional.py:62-75, 25-29): mp, plv the predictive
// mean and log-variance, (mu, lv) the posterior, p = exp(-sig / 2), e = exp(-sig).  Adds to ldyn and ent; returns the seeds on mu
// and lv (no 1/B): the dynamics term's where with_dyn (outside warm-up, not dropped), the entropy's where with_ent.
struct VjfDynSeed { float dmu, dlv; };
__device__ __forceinline__ VjfDynSeed vjf_dyn_term(float mp, float mu, float lv, float plv, float sig, float p, float e,
                                                   bool with_dyn, bool with_ent, float& ldyn, float& ent) {
    const float dsc = mp * p - mu * p;
    const float tr = expf(plv + lv - sig);
    ldyn += 0.5f * (dsc * dsc + sig) + 0.5f * tr;
    ent += 0.5f * lv;
    VjfDynSeed s = {0.f, with_ent ? -0.5f : 0.f};
    if (with_dyn) { s.dmu = -e * (mp - mu); s.dlv += 0.5f * tr; }
    return s;
}
