// vjf_mega_kernel.h -- vjf_filter_seq / vjf_filter_step on a single rank as ONE launch (a grid resident as a whole) per chunk of steps.
//
// Every piece of a filtering step (vjf/model.py:179-221) is a ROLE played by workgroups of the same grid, one workgroup per
// compute unit, all resident for the whole chunk (the host launches the grid only if the occupancy query says all of it fits):
//
//   RLS roles        workgroup 0: the Cholesky loop (vjf_chol_loop), 1: the y / W loop, 2 .. 1 + 2 nbl: the inverse loops
//                    (vjf_rls_post_loop) -- module.py:94-102, model.py:373-377, exactly as before
//   trial role       n_trial workgroups; workgroup w owns the 32-trial tiles w, w + n_trial, ..  Per tile and step: reparametrise,
//                    RBF features, recognition network, posterior, decoder (model.py:97-122), Phi^T dx of the tile; then -- behind the
//                    RLS update of the previous step -- predictive mean / variance, loss terms (model.py:124-154), hand-derived backward
//                     and the tile's weight / bias gradients on the matrix cores (K = 32 trials).  A workgroup's sums
//                    over its tiles leave as two slabs: early [Phi^T dx | sum dx^2], late [gradients | loss sums].
//   Gram role        n_gram workgroups: Phi^T Phi (module.py:96) one step AHEAD -- its rows of Phi formed here from the posterior, in LDS, all 28 lower 32x32 tiles per
//                    workgroup on v_mfma_f32_32x32x2_f32, partial tiles to a slab, then every workgroup sums its share of the slabs
//   operand role     ceil(n / 16) workgroups: sum of the early slabs -> Phi^T dx, g = P W + Phi^T dx / v, P += Phi^T Phi / v (module.py:94-96)
//   SGD role         n_sgd workgroups: sum of the late slabs, finite guards and loss (model.py:138-154), clip + SGD (model.py:210-211),
//                    likelihood running variance (likelihood.py:28-40)
//
// Hand-offs are monotone workgroup counters in memory: producer = write-through stores, every storing wavefront drains vmcnt, the
// workgroup barrier, one relaxed agent-scope add; consumer = one lane polls about once a microsecond (bounded; VJF_POLL_SLEEP,
// vjf_handoff.h), the workgroup barrier, and every handed-off byte is read with an sc1 load (MI355X guide, "sc1 loads in place of the
// acquire"; VJF_HANDOFF_ACQUIRE=1 adds an agent-scope acquire behind every wait).  Nothing ever waits for work of a launch that has not been submitted: every
// producer is a workgroup of this grid, and the grid is resident as a whole.  All sums are taken in a fixed order: results do not
// depend on timing, and a sequence cut into chunks gives the same bits as one piece.
//
// This file holds the four kernels.  Each role is in its own header (vjf_mega_trial.h, _moments.h, _gram.h, _prep.h, _sgd.h); what
// they share -- arguments, counters, layouts, loads and stores, the MFMA product routines -- is in vjf_mega_common.h.
#pragma once
#include "vjf_mega_common.h"
#include "vjf_mega_trial.h"
#include "vjf_mega_moments.h"
#include "vjf_mega_gram.h"
#include "vjf_mega_prep.h"
#include "vjf_mega_sgd.h"

// ------------------------------------------------------------------------------------------------ the kernel
__global__ __launch_bounds__(VJF_MG_THREADS) void vjf_mega_kernel(VjfPlan P, VjfMegaArgs A, VjfCholArgs C, VjfPostArgs Q) {
    static_assert(VJF_CHOL_THREADS == VJF_MG_THREADS && VJF_POST_THREADS == VJF_MG_THREADS, "one workgroup size for every role");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_dead;
    if (threadIdx.x == 0) s_dead = 0;
    __syncthreads();
    int b = (int)blockIdx.x;
    // the NEXT launch's counters are zeroed here, by one workgroup of the operand role, before anything else (that block belongs to the
    // launch before this one, which is complete; the kernel boundary makes the zeros visible to the next launch): no memset in
    // front of a launch
    if (b == A.n_rls + A.n_trial + A.n_gram)
        for (int i = threadIdx.x; i < MG_C_WORDS; i += VJF_MG_THREADS) A.cnt_next[i] = 0u;
    float* stw = A.state + P.off[VJF_SLOT_SCALARS] + VJF_SC_STATUS;
    if (mg_grid_resident(A.cnt, stw, A.alive_extra)) {
        if (b == 0) vjf_chol_loop<16>(P, C, lds, &s_dead);
        else if (b == 1) vjf_rls_post_loop(P, Q, lds, &s_dead, 2, 0);
        else if (b < A.n_rls) vjf_rls_post_loop(P, Q, lds, &s_dead, 1, b - 2);
        else if ((b -= A.n_rls) < A.n_trial) vjf_mega_trial<true>(P, A, lds, b);
        else if ((b -= A.n_trial) < A.n_gram) vjf_mega_gram(P, A, lds, b);
        else if ((b -= A.n_gram) < A.n_prep) vjf_mega_prep(P, A, lds, b);
        else vjf_mega_sgd<true>(P, A, lds, b - A.n_prep);
    }
    mg_tell_host(stw, A.host_word);
}

// The flag sets of VJF.filter that have no RLS update -- warm_up=True (the first epochs of fit: vjf/model.py:243-259, 148, 370),
// update=False, sgd=False (a deployed filter: model.py:180, 206, 215) -- as ONE launch too: trial and SGD roles only (W, w_chol are
// constants of the launch; in warm-up the SGD role's scalar lane also keeps the state-noise variance, from the residual sums the
// trial role hands over with its loss sums).  Without sgd and update nothing changes between steps and no role waits for another
// except through the ring of loss sums.
__global__ __launch_bounds__(VJF_MG_THREADS) void vjf_mega_lite_kernel(VjfPlan P, VjfMegaArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int b = (int)blockIdx.x;
    if (b == A.n_trial)                                 // (the next launch's counter block: see vjf_mega_kernel)
        for (int i = threadIdx.x; i < MG_C_WORDS; i += VJF_MG_THREADS) A.cnt_next[i] = 0u;
    float* stw = A.state + P.off[VJF_SLOT_SCALARS] + VJF_SC_STATUS;
    if (mg_grid_resident(A.cnt, stw, A.alive_extra)) {
        const int idx = b - A.n_trial;
        if (b < A.n_trial) vjf_mega_trial<false>(P, A, lds, b);
        else if (!(A.flags & (VJF_FLAG_SGD | VJF_FLAG_UPDATE))) {
            // nothing changes between the steps: no SGD role -- the first n_sgd of these workgroups build the parameter image, and all
            // n_mom of them (n_mom >= n_sgd, or none) are the moments role; the loss sums are the trial role's own (its last arriver)
            if (idx < A.n_sgd) mg_build_image(P, A, idx, A.n_sgd);
            if (idx < A.n_mom) vjf_mega_moments(P, A, lds, idx);
        }
        else if (idx < A.n_mom) vjf_mega_moments(P, A, lds, idx);
        else vjf_mega_sgd<false>(P, A, lds, idx - A.n_mom);
    }
    mg_tell_host(stw, A.host_word);
}

// The same two grids with the recognition layers' activation `act` (vjf_act.h; vjf_set_activation) in place of tanh: extra
// instantiations of the same roles, the Tanh kernels above keep their code.  The two bodies are pasted ON PURPOSE: as two
// `template <bool ACT>` device functions behind one-line kernels, vjf_mega_kernel's scratch goes from 100 to 128 bytes and
// vjf_mega_lite_kernel's v_writelane / v_readlane count from 2936 to 3500 (profiles/mega_split_isa.txt, candidate 2).
__global__ __launch_bounds__(VJF_MG_THREADS) void vjf_mega_act_kernel(VjfPlan P, VjfMegaArgs A, VjfCholArgs C, VjfPostArgs Q, VjfAct act) {
    static_assert(VJF_CHOL_THREADS == VJF_MG_THREADS && VJF_POST_THREADS == VJF_MG_THREADS, "one workgroup size for every role");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_dead;
    if (threadIdx.x == 0) s_dead = 0;
    __syncthreads();
    int b = (int)blockIdx.x;
    // the NEXT launch's counters are zeroed here, by one workgroup of the operand role, before anything else (that block belongs to the
    // launch before this one, which is complete; the kernel boundary makes the zeros visible to the next launch): no memset in
    // front of a launch
    if (b == A.n_rls + A.n_trial + A.n_gram)
        for (int i = threadIdx.x; i < MG_C_WORDS; i += VJF_MG_THREADS) A.cnt_next[i] = 0u;
    float* stw = A.state + P.off[VJF_SLOT_SCALARS] + VJF_SC_STATUS;
    if (mg_grid_resident(A.cnt, stw, A.alive_extra)) {
        if (b == 0) vjf_chol_loop<16>(P, C, lds, &s_dead);
        else if (b == 1) vjf_rls_post_loop(P, Q, lds, &s_dead, 2, 0);
        else if (b < A.n_rls) vjf_rls_post_loop(P, Q, lds, &s_dead, 1, b - 2);
        else if ((b -= A.n_rls) < A.n_trial) vjf_mega_trial<true, true>(P, A, lds, b, act);
        else if ((b -= A.n_trial) < A.n_gram) vjf_mega_gram(P, A, lds, b);
        else if ((b -= A.n_gram) < A.n_prep) vjf_mega_prep(P, A, lds, b);
        else vjf_mega_sgd<true>(P, A, lds, b - A.n_prep);
    }
    mg_tell_host(stw, A.host_word);
}

__global__ __launch_bounds__(VJF_MG_THREADS) void vjf_mega_lite_act_kernel(VjfPlan P, VjfMegaArgs A, VjfAct act) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int b = (int)blockIdx.x;
    if (b == A.n_trial)                                 // (the next launch's counter block: see vjf_mega_kernel)
        for (int i = threadIdx.x; i < MG_C_WORDS; i += VJF_MG_THREADS) A.cnt_next[i] = 0u;
    float* stw = A.state + P.off[VJF_SLOT_SCALARS] + VJF_SC_STATUS;
    if (mg_grid_resident(A.cnt, stw, A.alive_extra)) {
        const int idx = b - A.n_trial;
        if (b < A.n_trial) vjf_mega_trial<false, true>(P, A, lds, b, act);
        else if (!(A.flags & (VJF_FLAG_SGD | VJF_FLAG_UPDATE))) {
            // nothing changes between the steps: no SGD role -- the first n_sgd of these workgroups build the parameter image, and all
            // n_mom of them (n_mom >= n_sgd, or none) are the moments role; the loss sums are the trial role's own (its last arriver)
            if (idx < A.n_sgd) mg_build_image(P, A, idx, A.n_sgd);
            if (idx < A.n_mom) vjf_mega_moments(P, A, lds, idx);
        }
        else if (idx < A.n_mom) vjf_mega_moments(P, A, lds, idx);
        else vjf_mega_sgd<false>(P, A, lds, idx - A.n_mom);
    }
    mg_tell_host(stw, A.host_word);
}
