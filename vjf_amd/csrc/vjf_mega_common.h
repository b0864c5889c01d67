// vjf_mega_common.h -- what the roles of the one-launch route (vjf_mega_kernel.h) share: the counter block and the launch's
// arguments, the LDS and slab layouts, the MFMA product routines, the grid's first and last act (waits, sc1 loads and write-through
// stores: vjf_handoff.h).
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_chol_kernel.h"
#include "vjf_rls_operands.h"   // VJF_PREPG_LDP
#include "vjf_handoff.h"
#include "vjf_plan.h"
#include "vjf_post_kernel.h"
#include "vjf_trial_mfma_kernel.h"   // vjf_f32x4
#include "vjf_act.h"

#define VJF_MG_THREADS 512
#define VJF_MG_WAVES 8
#define VJF_MG_TR 32                 // trials per tile: two column groups of v_mfma_f32_16x16x4_f32 share every A operand
#define VJF_MG_LD 33                 // LDS matrices are feature-major [feature][32 trials + 1 pad]
#define VJF_MG_GROWS 96              // rows of Phi formed per pass of the Gram role
#define VJF_MG_MAXQ 4                // 32x32 tiles of Phi^T Phi per wavefront of a Gram workgroup (28 lower tiles / 8)
#define VJF_MG_RING 32               // loss sums of a late slab: a ring over the steps (a launch without parameter updates has no gate
                                     // between its steps: the trial role may run this many steps ahead of the role that sums them)
#define VJF_MG_TAG_TILES 512         // most tiles a launch with a moments role has (B <= 16384)
#define RS_RESID 5                   // late slab only: sum |dx - Phi W|^2 of a workgroup's trials (warm-up: the state-noise update
                                     // without an RLS update, model.py:373-377 with the old W)

// counters: one per 64-byte line of the block -- times MG_C_SPREAD (experiment: 64 puts every counter into a 4-KB page of its own)
#ifndef MG_C_SPREAD
#define MG_C_SPREAD 1
#endif
enum {
    MG_C_FWD = 16 * MG_C_SPREAD,       // trial workgroups whose early slab of step t is in memory           target (t + 1) n_trial
    MG_C_K1 = 32 * MG_C_SPREAD,        // trial workgroups that have read W, w_chol, sigma of step t - 1      target (t + 1) n_trial
    MG_C_BWD = 48 * MG_C_SPREAD,       // trial workgroups whose late slab of step t is in memory            target (t + 1) n_trial
    MG_C_GRAM = 64 * MG_C_SPREAD,      // Gram workgroups whose partial tiles of event e are in memory       target (e + 1) n_gram
    MG_C_STAT = 80 * MG_C_SPREAD,      // Gram workgroups whose share of Phi^T Phi of event e is reduced      target (e + 1) n_gram
    MG_C_PREP = 96 * MG_C_SPREAD,      // operand workgroups done with step t                                target (t + 1) n_prep
    MG_C_SGD = 112 * MG_C_SPREAD,      // SGD workgroups done with step t                                    target (t + 1) n_sgd
    MG_C_PDONE = 128 * MG_C_SPREAD,    // RLS workgroups (y / W loop + inverse loops) done with step t       target (t + 1) (2 nbl + 1)
    MG_C_STARTED = 144 * MG_C_SPREAD,
    MG_C_REDO_B = 0 * MG_C_SPREAD,     // trial workgroups whose REPLAYED late slab is in memory             target (replays so far) n_trial
    MG_C_REDO_S = 176 * MG_C_SPREAD,   // SGD workgroups done with a replayed step                         target (replays so far) n_sgd
    MG_C_IMG = 208 * MG_C_SPREAD,      // SGD workgroups whose share of the parameter image is in memory (start of the launch)  target n_sgd
    MG_C_SIGW = 224 * MG_C_SPREAD,     // 8 bytes: {epoch, sigma} from the y / W loop to the Cholesky loop of the next step
    MG_C_XT = 240 * MG_C_SPREAD,       // inverse workgroups whose share of xt = w_chol^T is in memory (start of the launch)              target 2 nbl
                                       // [+ 1]: launches without an RLS update: trial workgroups that met a nonzero BELOW the diagonal of w_chol
    MG_C_MASK = 192 * MG_C_SPREAD,     // (step + 1) << 8 | non-finite loss components (1 recon, 2 dynamics, 4 entropy) of the last step that had one
    MG_C_COLFLAGS = 160 * MG_C_SPREAD, // [0 .. VJF_CHOL_MAXBLK]: column flags of the Cholesky loop; [VJF_CHOL_MAXBLK + 2]: its "operands loaded" word
    MG_C_ALIVE = 256 * MG_C_SPREAD,    // workgroups of the grid that have started (all of them: the launch goes on; else it ends untouched)  target gridDim.x
    // per-TILE step tags of the launches without an RLS update that have a moments role (vjf_mega_moments): one producer, one consumer each
    MG_C_ARR = 272 * MG_C_SPREAD,      // [step % VJF_MG_RING]: trial workgroups whose loss sums of that step are in memory (a launch without
                                       // parameter updates: the LAST arriver sums them; it puts the word back to 0)
    MG_C_TAG_POST = (272 + 32) * MG_C_SPREAD, // [tile]: t + 1 once the posterior of step t of the tile is in memory (trial role -> moments role)
    MG_C_TAG_MOM = MG_C_TAG_POST + VJF_MG_TAG_TILES,   // [tile]: t + 1 once the predictive moments of step t of the tile are (moments role -> trial role)
    MG_C_WORDS = MG_C_TAG_MOM + VJF_MG_TAG_TILES
};

// The last act of every workgroup of a one-launch grid: if a wait of the launch has been given up (by this workgroup or another),
// say so where the host sees it without a synchronisation (vjf_plan.h, VJF_MIRROR_SLOT).
__device__ __forceinline__ void mg_tell_host(const float* status, unsigned* host_word) {
    if (threadIdx.x == 0 && host_word && vjf_abort_seen(status)) __hip_atomic_store(host_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The first act of every workgroup of a one-launch grid: count itself in and wait until the WHOLE grid has -- every wait of the
// launch is for a workgroup of the same grid.  Within a process the launches of this route are chained (vjf_abi.hip), so a grid
// never shares the device with another one of its kind; a grid of ANOTHER process can hold compute units (each of these
// workgroups wants a whole unit's LDS), and then neither would ever be placed as a whole.  The bound is short (2^17 polls, about a
// quarter of a second: a grid starts within a microsecond on a free device): the launch ends before any role has written to the
// state, VJF_STATUS_NOT_RESIDENT says so, and the context takes the per-step kernels from its next call on.
__device__ __forceinline__ bool mg_grid_resident(unsigned* cnt, float* status, int extra) {
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(cnt + MG_C_ALIVE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool there = false;
        for (unsigned spins = 0; spins < (1u << 17); ++spins) {        // (its own loop, not vjf_poll_count: the short bound above and a plain >=)
            if (__hip_atomic_load(cnt + MG_C_ALIVE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= gridDim.x + (unsigned)extra) { there = true; break; }
            if ((spins & 255u) == 255u && vjf_abort_seen(status)) break;
            __builtin_amdgcn_s_sleep(VJF_POLL_SLEEP);
        }
        if (!there && !vjf_abort_seen(status)) vjf_status_or(status, VJF_STATUS_RLS_FAILED | VJF_STATUS_NOT_RESIDENT);
        vjf_s_abort_word = there ? 0 : 1;
    }
    __syncthreads();
    return vjf_s_abort_word == 0;
}

struct VjfMegaArgs {
    int T, B, ntiles;
    int n_rls, n_trial, n_gram, n_prep, n_sgd;        // grid = their sum
    unsigned* host_word;                              // this context's word of the pinned host page (null: none), see mg_tell_host
    int alive_extra;                                  // test hook (VJF_DEBUG_ABSENT=1): workgroups the residency count waits for beyond the grid's own
    int n_mom;                                        // launches without an RLS update: workgroups of the moments role (0: the trial role forms the moments itself)
    float* mom;                                       // [tile][step parity][(2 dz + 1) x 32]: pt.mean | Phi W | pt.logvar of the tile's trials, moments role -> trial role
    int n_sgd_live;                                   // SGD workgroups that stay for the steps (all of them; ONE when flags has no VJF_FLAG_SGD:
                                                      // the others only help to build the parameter image at the start of the launch)
    const float* y; const float* u; const float* eps; const float* mu0; const float* lv0;
    float* mu; float* lv; float* loss;
    float* state; float* aux;
    const float* img;                                 // the optimised parameters as the trial role's LDS holds them (vjf_mega_trial_lds: theta region)
    float* pmsave;                                    // (B, dz + 1): pt.mean | pt.logvar of every trial at its last step (for a replayed backward pass)
    float* slab_early; float* slab_late; float* gslab;
    float* red0; float* red1;                         // reduce buffers of even / odd steps ([G | FDX | sums], as the RLS loops read them)
    float* gbuf;                                      // g (n, dz)
    const float* xt;                                  // (n, n) row-major L^-1 = w_chol^T: the inverse loops keep it beside w_chol (vjf_post_kernel.h)
    unsigned* cnt;
    unsigned* cnt_next;                               // the other counter block: zeroed by this launch for the next one
    unsigned flags;
    int early_len, late_len;                          // floats per trial workgroup
    int lds_floats;                                   // dynamic LDS of the launch (floats): decides whether the parameters are staged in it
    int gram_rows;                                    // rows of Phi per Gram workgroup (a multiple of 2)
    int slab_len;                                     // floats of gradient per late slab (vjf_mega_slab_layout)
    const int* sl_pidx;                               // per slab float: the parameter it is the gradient of (index in the train region; -1: padding)
    const int* sl_cidx;                               // per slab float: that parameter's copy the trial role reads (LDS image, or the transposed aux copy; -1: none)
    const int* sl_grp;                                // per slab QUAD: 0 recognition, 1 decoder group (learning rate, freeze flag)
                                                      // behind its slab_len / 4 words (VJF_GT_AT): the step's gradient tiles (vjf_mega_grad_tiles) -- no
                                                      // argument of their own: a longer argument block cost vjf_mega_act_kernel scratch
    unsigned long long* stamps;                       // diagnostic (null in normal runs): s_memrealtime of workgroup 0 of each role, 32 per step
};

// ---- LDS of the trial role (floats); the host uses the same function to size the launch
struct VjfMegaTrialLds {
    int cen, iw, in, xu, phi, act, dd, mu, lv, xt, e2, pm, dmu, dlv, dx, xn, py, dpy, one, zero, sc, red, plv, wg, part, total;
    int nd;
    // the optimised parameters, staged once per step when they fit (theta = 1): matrices in their torch layout [rows][ld], ld = the
    // row length rounded up to 2 (mod 4) -- the rows an MFMA operand read walks then fall on distinct banks
    int th0, th_len;                                  // first float / length (a multiple of 4) of the region
    int theta, th_w[VJF_MAX_HIDDEN], th_ldw[VJF_MAX_HIDDEN], th_head, th_ldh, th_dec, th_ldd, th_b[VJF_MAX_HIDDEN], th_bl, th_bd;
};
__host__ __device__ inline int vjf_mega_ld(int K) { return ((K + 1) & ~3) + 2; }
// LAYERS = false (device code): the per-layer arrays are left alone -- filling them in a loop with a run-time index would put the
// whole struct into scratch memory; the kernels get a layer's entries from mg_theta_layer
template <bool LAYERS = true>
__host__ __device__ inline VjfMegaTrialLds vjf_mega_trial_lds(const VjfPlan& P, int lds_limit_floats = 0) {
    VjfMegaTrialLds l;
    const int LD = VJF_MG_LD;
    int o = 0;
    auto take = [&](int nfl) { const int at = o; o += (nfl + 3) & ~3; return at; };
    l.cen = take(((P.n + 3) & ~3) * P.dxu); l.iw = take((P.n + 3) & ~3);   // centroids transposed [dxu][n rounded to 4]
    l.in = take(P.din * LD); l.xu = take(P.dxu * LD); l.phi = take(P.n * LD); l.act = take(P.hsum * LD);
    const bool compact = P.dy >= P.hmax;              // the first delta buffer lives in the (by then dead) decoder-mean rows
    l.nd = compact ? (P.L > 1 ? 1 : 0) : (P.L > 1 ? 2 : 1);
    l.dd = take(l.nd * P.hmax * LD);
    l.mu = take(P.dz * LD); l.lv = take(P.dz * LD); l.xt = take(P.dz * LD); l.e2 = take(P.dz * LD); l.pm = take(P.dz * LD);
    l.dmu = take(P.dz * LD); l.dlv = take(P.dz * LD); l.dx = take(P.dz * LD); l.xn = take(P.dxu * LD);
    l.py = take(P.dy * LD); l.dpy = take(P.dy * LD);
    l.one = take(LD); l.zero = take(LD);
    l.sc = take(VJF_MG_TR * RS_N); l.red = take(VJF_MG_WAVES * VJF_MG_TR); l.plv = take(VJF_MG_TR); l.wg = take(16);
    // partial tiles of the K-split products (heads, pt.mean), VJF_MG_WAVES x 16 rows: in the delta buffers (free until the backward
    // pass) or the dpy rows (free until the losses) when those are large enough, else rows of their own
    const int alias_rows = compact ? P.dy : l.nd * P.hmax;
    l.part = alias_rows >= VJF_MG_WAVES * 16 ? (compact ? l.dpy : l.dd) : take(VJF_MG_WAVES * 16 * LD);
    l.total = o;
    {
        int prev = P.din;
        l.th0 = o;
        if (LAYERS) for (int k = 0; k < VJF_MAX_HIDDEN; ++k) { l.th_w[k] = l.th_ldw[k] = l.th_b[k] = 0; }
        for (int k = 0; k < P.L; ++k) {
            const int ldw = vjf_mega_ld(prev), w = take(P.h[k] * ldw), b = take(P.h[k]);
            if (LAYERS) { l.th_ldw[k] = ldw; l.th_w[k] = w; l.th_b[k] = b; }
            prev = P.h[k];
        }
        l.th_ldh = vjf_mega_ld(prev); l.th_head = take(2 * P.dz * l.th_ldh); l.th_bl = take(P.dz);
        l.th_ldd = vjf_mega_ld(P.dz); l.th_dec = take(P.dy * l.th_ldd); l.th_bd = take(P.dy);
        l.th_len = o - l.th0;
        l.theta = (lds_limit_floats > 0 && o <= lds_limit_floats) ? 1 : 0;
        if (l.theta) l.total = o;
    }
    return l;
}
// the mu / lv / xt / e2 / pm / dmu / dlv / dx rows must be adjacent in this order (the heads write 2 dz rows at mu, the ahead
// features park xs' in the 3 dz rows at dmu): take() pads to 4 floats, so dz * LD must be a multiple of 4 or the code below
// addresses through the struct's offsets only -- it does (no pointer arithmetic across fields except mu -> lv and dmu -> dlv,
// which are handled explicitly).

// Late slab of a trial workgroup: its tiles' gradients, one block per weight tensor, each block TRANSPOSED -- row j = the input
// (activation) index, then the bias row; columns = the output units, padded to a multiple of 4 -- so that the four accumulator
// registers of a lane (four consecutive output units of one input) leave as ONE 16-byte write-through store.  Blocks in the order
// the backward pass produces them: decoder, mean head, log-variance head, recognition layers L-1 .. 0.
struct VjfMegaSlab { int off[VJF_MAX_HIDDEN + 3], ldm[VJF_MAX_HIDDEN + 3], rows[VJF_MAX_HIDDEN + 3], len; };
__host__ __device__ inline VjfMegaSlab vjf_mega_slab_layout(const VjfPlan& P) {
    VjfMegaSlab L;
    int o = 0, k = 0;
    auto blk = [&](int M, int rows) { L.off[k] = o; L.ldm[k] = (M + 3) & ~3; L.rows[k] = rows; o += rows * L.ldm[k]; ++k; };
    const int hL = P.h[P.L - 1];
    blk(P.dy, P.dz + 1);                               // 0: decoder  (dy, dz) + bias
    blk(P.dz, hL);                                     // 1: mean head (dz, hL), no bias
    blk(P.dz, hL + 1);                                 // 2: log-variance head + bias
    for (int l = P.L - 1; l >= 0; --l) blk(P.h[l], (l > 0 ? P.h[l - 1] : P.din) + 1);   // 3 + (L-1-l): layer l + bias
    for (; k < VJF_MAX_HIDDEN + 3; ++k) { L.off[k] = o; L.ldm[k] = 4; L.rows[k] = 0; }
    L.len = o;
    return L;
}

// One entry of the layouts above for a layer / block index that is only known at run time, recomputed from the plan by a short
// scalar loop: indexing the structs' arrays with it would put them into scratch memory (the kernel then needs a scratch buffer
// at launch and pays memory round trips for what is a handful of integer additions).
__device__ __forceinline__ void mg_theta_layer(const VjfPlan& P, int th0, int l, int& w, int& ldw, int& b) {
    int o = th0, prev = P.din;
    w = ldw = b = 0;
    for (int k = 0; k <= l && k < P.L; ++k) {
        ldw = vjf_mega_ld(prev);
        w = o; o += (P.h[k] * ldw + 3) & ~3;
        b = o; o += (P.h[k] + 3) & ~3;
        prev = P.h[k];
    }
}
__device__ __forceinline__ void mg_slab_block(const VjfPlan& P, int blk, int& off, int& ldm, int& rows) {
    const int hL = P.h[P.L - 1];
    int o = 0;
    auto step = [&](int M, int r, bool take_it) { if (take_it) { off = o; ldm = (M + 3) & ~3; rows = r; } o += r * ((M + 3) & ~3); };
    off = 0; ldm = 4; rows = 0;
    step(P.dy, P.dz + 1, blk == 0);
    step(P.dz, hL, blk == 1);
    step(P.dz, hL + 1, blk == 2);
    for (int l = P.L - 1, k = 3; l >= 0; --l, ++k) step(P.h[l], (l > 0 ? P.h[l - 1] : P.din) + 1, blk == k);
}

static inline size_t vjf_mega_gram_lds_floats(const VjfPlan& P) {      // rows of Phi | tile table | centroids^T | -1/(2 w^2) | xs rows
    const size_t npad = (size_t)((P.n + 3) & ~3);
    return (size_t)VJF_MG_GROWS * P.ldE + 64 + npad * P.dxu + npad + (size_t)VJF_MG_GROWS * P.dxu + 16;
}
static inline size_t vjf_mega_prep_lds_floats(const VjfPlan& P) {
    return (size_t)16 * VJF_PREPG_LDP(P.n) + (size_t)P.n * 17 + (size_t)VJF_MG_WAVES * 16 * 17 + 16 * 17 + 64;
}

// (mg_tanh, the Tanh kernels' tanh: vjf_act.h)

// acc_g(row = 4*(lane>>4)+r, col = lane&15) += sum_{kb <= k < ke} Ag[k*lda + m0 + row] * Xs[k*LD + 16 g + col]   (g = 0, 1)
// Rows m0 + i >= M contribute 0 (their A operand is read from a clamped address and masked at use).  kb is a multiple of 4.  The A operands come straight from L2 (k-major matrices: row k contiguous over the output features), 16 k-steps per batch,
// two batches in flight: while one batch's 32 MFMAs issue the next one's loads are on their way (and the SIMD's other wavefront
// fills what latency is left).  The loads are sc1 (they bypass this CU's vector L1): these matrices are rewritten every step by
// other roles, and the waits in front of them do not acquire.
// one batch of mg_mma2 (below) on its own: the 16 A-operand loads of k-steps s0 .. s0 + 15, and their MFMAs -- for a product
// whose loads are issued long before its turn (pt.mean: in front of the variance tiles)
__device__ __forceinline__ void mg_mma2_ld16(float (&a)[16], const float* __restrict__ Ag, int lda, int M, int m0, int kb, int ke, int s0, int lane) {
    const int i = lane & 15, kk = lane >> 4;
    const bool rv = (m0 + i) < M;
    const unsigned row = rv ? (unsigned)(m0 + i) : 0u;
    const int klast = ke - 1;
#pragma unroll
    for (int q = 0; q < 16; ++q) { const int k = min(kb + 4 * (s0 + q) + kk, klast); a[q] = vjf_ld_sc1(Ag + row + (unsigned)k * (unsigned)lda); }
    // (rows beyond M are masked where the value is USED: a select on a load's destination right behind the load makes the compiler
    //  wait for the load there, and the batch would no longer be in flight beside the previous batch's MFMAs)
}
// (mg_mmaN_mm16<2, VJF_MG_LD> written out ON PURPOSE: forwarding to the template grows vjf_mega_lite_kernel by 5612 bytes and its
//  v_writelane / v_readlane count from 2936 to 3769 -- profiles/mega_split_isa.txt, candidate 4)
template <bool SPLIT = true>
__device__ __forceinline__ void mg_mma2_mm16(vjf_f32x4& acc0, vjf_f32x4& acc1, const float (&a)[16], const float* Xs, int M, int m0, int kb, int ke, int s0, int lane) {
    constexpr int LD = VJF_MG_LD;
    const int i = lane & 15, kk = lane >> 4;
    const bool rv = (m0 + i) < M;
    const float* xp = Xs + i;
    const int nst = (ke - kb + 3) >> 2, klast = ke - 1;
    // full k-steps (4 (s + 1) <= ke - kb; kb is a multiple of 4): no clamp, the A operand masked by its row alone, B operands in chunks
    // of four steps at immediate offsets 4 q LD and + 16 floats from one base (at most 60 LD + 16 floats = 7984 bytes), the next chunk's
    // reads in front of this chunk's MFMAs (a chunk's steps behind the last full one read LDS rows that are not used: mg_mma2_lds).
    // Then the one partial step, clamped and masked as before.  !SPLIT: every step that way (see mg_var2).
    const int nf = SPLIT ? ((ke - kb) >> 2) - s0 : 0;   // full steps of this batch (uniform)
    const float* xb = xp + (kb + 4 * s0 + kk) * LD;
    float b[2][8];
    auto rdb = [&](float (&bq)[8], int c4) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { bq[2 * c] = xb[4 * (c4 + c) * LD]; bq[2 * c + 1] = xb[4 * (c4 + c) * LD + 16]; }
    };
    if (nf > 0) rdb(b[0], 0);
#pragma unroll
    for (int c4 = 0; c4 < 16; c4 += 4) {
        if (c4 < nf) {                                 // (uniform)
            if (c4 + 4 < 16 && c4 + 4 < nf) rdb(b[((c4 >> 2) + 1) & 1], c4 + 4);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c4 + c < nf) {                     // (uniform)
                    const float av = rv ? a[c4 + c] : 0.f;
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[(c4 >> 2) & 1][2 * c], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[(c4 >> 2) & 1][2 * c + 1], acc1, 0, 0, 0);
                }
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if ((!SPLIT || q == nf) && s0 + q < nst) {     // (uniform) the partial step (!SPLIT: every step)
            const int k = kb + 4 * (s0 + q) + kk;
            const int kc = min(k, klast);
            const float av = (rv && k < ke) ? a[q] : 0.f;
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xp[kc * LD], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xp[kc * LD + 16], acc1, 0, 0, 0);
        }
    }
}

template <bool DEEP = false>
__device__ __forceinline__ void mg_mma2(vjf_f32x4& acc0, vjf_f32x4& acc1, const float* __restrict__ Ag, int lda, int M, int m0,
                                        const float* Xs, int kb, int ke, int lane) {
    constexpr int LD = VJF_MG_LD;
    const int i = lane & 15, kk = lane >> 4;
    const bool rv = (m0 + i) < M;
    const unsigned row = rv ? (unsigned)(m0 + i) : 0u;
    const unsigned ulda = (unsigned)lda;
    const float* xp = Xs + i;
    const int nst = (ke - kb + 3) >> 2;                // k-steps
    const int klast = ke - 1;
    // (ld16 / mm16 are mg_mma2_ld16 / mg_mma2_mm16 written out again ON PURPOSE: as calls they move the SGPR spill lanes of all four
    //  resident kernels and take vjf_mega_lite_act_kernel's scratch from 100 to 104 bytes -- profiles/mega_split_isa.txt, candidate 3)
    auto ld16 = [&](float (&a)[16], int s0) {          // steps s0 .. s0 + 15: clamped rows, masked at use
#pragma unroll
        for (int q = 0; q < 16; ++q) { const int k = min(kb + 4 * (s0 + q) + kk, klast); a[q] = vjf_ld_sc1(Ag + row + (unsigned)k * ulda); }
    };
    auto mm16 = [&](const float (&a)[16], int s0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (s0 + q < nst) {                        // (uniform)
                const int k = kb + 4 * (s0 + q) + kk;
                const int kc = min(k, klast);
                const float av = (rv && k < ke) ? a[q] : 0.f;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xp[kc * LD], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xp[kc * LD + 16], acc1, 0, 0, 0);
            }
        }
    };
    if (nst <= 0) return;
    if (DEEP) {
        // up to 64 k-steps (K <= 256): every load of the tile is issued before the first MFMA
        float a0[16], a1[16], a2[16], a3[16];
        ld16(a0, 0);
        if (nst > 16) ld16(a1, 16);
        if (nst > 32) ld16(a2, 32);
        if (nst > 48) ld16(a3, 48);
        mm16(a0, 0);
        if (nst > 16) mm16(a1, 16);
        if (nst > 32) mm16(a2, 32);
        if (nst > 48) mm16(a3, 48);
        for (int s0 = 64; s0 < nst; s0 += 16) { ld16(a0, s0); mm16(a0, s0); }
        return;
    }
    float a0[16], a1[16];
    ld16(a0, 0);
    if (nst > 16) ld16(a1, 16);
    for (int s0 = 0; s0 < nst; s0 += 32) {
        mm16(a0, s0);
        if (s0 + 32 < nst) ld16(a0, s0 + 32);
        if (s0 + 16 < nst) {
            mm16(a1, s0 + 16);
            if (s0 + 48 < nst) ld16(a1, s0 + 48);
        }
    }
}

// The predictive variance's share of one wavefront: sum over its (at most two) 16-row tiles of the ROW-major inverse factor Xt = L^-1
// of the squares of  acc_g(row, col) = sum_{k < K} Xt[(j0 + row) * n + k] * Xs[k * LD + 16 g + col],  into v2a / v2b (the two 16-trial
// column groups).  A lane takes 16 bytes along k: lane (i, kk) loads Xt[j0 + i][16 t + 4 kk .. + 3] with one sc1 load and feeds
// component c to the MFMA of step (t, c), whose k index is 16 t + 4 kk + c -- any order of the k indices is a valid product as long
// as both operands use it (the B operand reads that row of Xs).  Batches of four loads (64 k); the two tiles' batches form ONE
// stream with three batches in flight: the second tile's first loads are out while the first tile still multiplies (a pipeline
// drained between the tiles exposes an L2 round trip per tile).  Each tile's products run in ascending batch order, then its sum of
// squares: the bits do not depend on how the batches are interleaved.
// j0B < 0: no second tile; j0A < 0: none at all.
// SPLIT (the Tanh training kernel): a tile's k range splits into full steps (16 (t + 1) <= K: with the triangle flag all of them, except in
// the last row tile when n % 16 != 0) and at most one partial step (the dense walk's last one when n % 16 != 0).  A full step has no
// clamp and no mask: its eight B operands are read at immediate offsets (16 q + c) LD and + 16 floats from ONE base per batch,
// Xs + i + (4 kk + 16 t0) LD -- at most (48 + 3) LD + 16 floats = 6796 bytes, inside the 16 bits of the ds offset field; the base
// advances with the batch, so the offsets do not grow with n (the route admits n <= 32 VJF_CHOL_MAXBLK = 224) -- and the next step's
// reads are issued in front of this step's MFMAs.  rx must then be BOUNDED to the n x n floats of Xt (vjf_rsrc(base, n * n)): a lane
// whose row j0 + i is >= n (the last row tile when n is no multiple of 16) loads zeros, what the select on (row valid) makes of its
// operand.  The partial step keeps the clamped row of Xs and the masked A operand.  The k indices and the order of each accumulator's
// MFMAs are those of the plain loop: the same bits (tools/var_mma_bench.hip, profiles/var_interior_bench.txt: V1).
// !SPLIT (the other three kernels, see vjf_mega_trial.h: VSPLIT): every step is clamped and masked, rows >= n read row 0, rx may be
// unbounded.
// (mg_varN below is this routine for NG column groups, plain loads and batched B operands.  Two copies ON PURPOSE: with this one
//  an instantiation of mg_varN, vjf_mega_kernel's scratch goes from 100 to 132 bytes -- profiles/mega_split_isa.txt, candidate 5)
template <bool SPLIT = true>
__device__ __forceinline__ void mg_var2(float& v2a, float& v2b, __amdgpu_buffer_rsrc_t rx, int n, int j0A, int KA, int j0B, int KB,
                                        const float* Xs, int lane) {
    constexpr int LD = VJF_MG_LD;
    if (j0A < 0) return;
    const int i = lane & 15, kk = lane >> 4;
    const bool rvA = (j0A + i) < n, rvB = j0B >= 0 && (j0B + i) < n;
    const int offA = (SPLIT || rvA ? j0A + i : 0) * n + 4 * kk, offB = (j0B >= 0 && (SPLIT || rvB) ? j0B + i : 0) * n + 4 * kk;   // (SPLIT, rows >= n: behind the descriptor's end)
    const float* xp = Xs + i;
    const float* xq = xp + 4 * kk * LD;                                       // the full steps' base: + 16 t0 LD per batch
    const int ntA = (KA + 15) >> 4, ntB = j0B >= 0 ? (KB + 15) >> 4 : 0;
    const int SA = (ntA + 3) >> 2, SB = (ntB + 3) >> 2, S = SA + SB;
    vjf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    auto fold = [&]() {
        v2a = fmaf(acc0[0], acc0[0], fmaf(acc0[1], acc0[1], fmaf(acc0[2], acc0[2], fmaf(acc0[3], acc0[3], v2a))));
        v2b = fmaf(acc1[0], acc1[0], fmaf(acc1[1], acc1[1], fmaf(acc1[2], acc1[2], fmaf(acc1[3], acc1[3], v2b))));
    };
    auto ldb = [&](float4 (&a)[4], int sb) {
        const bool inB = sb >= SA;                                            // (uniform)
        const int t0 = 4 * (inB ? sb - SA : sb), off = inB ? offB : offA;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int kq = 16 * (t0 + q) + 4 * kk; a[q] = vjf_ld4_sc1(rx, off + (kq + 3 < n ? 16 * (t0 + q) : 0)); }
    };
    auto mmb = [&](const float4 (&a)[4], int sb) {
        const bool inB = sb >= SA;
        const int t0 = 4 * (inB ? sb - SA : sb), nt = inB ? ntB : ntA, ke = inB ? KB : KA;
        const bool rv = inB ? rvB : rvA;
        if (sb == SA && SA > 0) {                                             // the first batch of the second tile
            fold();
            acc0 = vjf_f32x4{0.f, 0.f, 0.f, 0.f}; acc1 = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const int nf = SPLIT ? (ke >> 4) - t0 : 0;                            // full steps of this batch (uniform; <= 0: none, >= 4: all)
        const float* xb = xq + 16 * t0 * LD;
        float b[2][8];
        auto rdb = [&](float (&bq)[8], int q) {
#pragma unroll
            for (int c = 0; c < 4; ++c) { bq[2 * c] = xb[(16 * q + c) * LD]; bq[2 * c + 1] = xb[(16 * q + c) * LD + 16]; }
        };
        if (nf > 0) rdb(b[0], 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < nf) {                                                     // (uniform) a full step: no clamp, no mask
                if (q + 1 < 4 && q + 1 < nf) rdb(b[(q + 1) & 1], q + 1);      // the next step's reads in front of this step's MFMAs
                const float av[4] = {a[q].x, a[q].y, a[q].z, a[q].w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], b[q & 1][2 * c], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], b[q & 1][2 * c + 1], acc1, 0, 0, 0);
                }
            } else if (t0 + q < nt) {                                         // (uniform) the tile's one partial step
                const int k0 = 16 * (t0 + q) + 4 * kk;
                const float av[4] = {a[q].x, a[q].y, a[q].z, a[q].w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k = k0 + c, kc = min(k, ke - 1);
                    const float v = (rv && k < ke) ? av[c] : 0.f;             // (masked at use: see mg_mma2)
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(v, xp[kc * LD], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(v, xp[kc * LD + 16], acc1, 0, 0, 0);
                }
            }
        }
    };
    float4 a0[4], a1[4], a2[4];
    ldb(a0, 0);
    if (S > 1) ldb(a1, 1);
    if (S > 2) ldb(a2, 2);
    for (int sb = 0; sb < S; sb += 3) {
        mmb(a0, sb);
        if (sb + 3 < S) ldb(a0, sb + 3);
        if (sb + 1 < S) { mmb(a1, sb + 1); if (sb + 4 < S) ldb(a1, sb + 4); }
        if (sb + 2 < S) { mmb(a2, sb + 2); if (sb + 5 < S) ldb(a2, sb + 5); }
    }
    fold();
}

// The same product with the A operand in LDS: Ws is a matrix [rows][ldw] as torch stores it.
//   TR = false: A[m][k] = Ws[(m0 + m) * ldw + k]       (out = W x:  forward products)
//   TR = true : A[m][k] = Ws[k * ldw + m0 + m]         (out = W^T x: backward products)
template <bool TRN>
__device__ __forceinline__ void mg_mma2_lds(vjf_f32x4& acc0, vjf_f32x4& acc1, const float* Ws, int ldw, int M, int m0, const float* Xs,
                                            int kb, int ke, int lane) {
    // The shape is the plan's -- run-time values -- and a plain loop over the k-steps (clamped k, masked A, addresses recomputed per
    // step, an LDS round trip per unrolled group) took 2.85 us for a (128, 70) layer where the same loop with the shape as compile-time
    // constants takes 1.6 (tools/lds_mma_bench.hip).  So: chunks of four k-steps whose operands are read with immediate offsets from one
    // base per chunk -- no clamp, no mask: rows beyond M are computed from row 0 and discarded by every caller, only the last, partial
    // k-step is clamped and masked -- and the next chunk's reads are issued before this chunk's MFMAs: 1.67 us.  (A chunk's steps
    // beyond the last full one read LDS behind the operands -- inside the allocation or, past its end, zeros --; their MFMAs are skipped.)
    constexpr int LD = VJF_MG_LD, CH = 4;
    if (ke <= kb) return;                              // (uniform: an empty K slice)
    const int i = lane & 15, kk = lane >> 4;
    const int mi = (m0 + i) < M ? m0 + i : 0;
    const int nf = (ke - kb) >> 2;                     // full k-steps (kb is a multiple of 4)
    const int astep = TRN ? 4 * ldw : 4;               // floats between two k-steps of the A operand
    const float* wp = TRN ? Ws + (size_t)(kb + kk) * ldw + mi : Ws + (size_t)mi * ldw + kb + kk;
    const float* xp = Xs + i + (kb + kk) * LD;
    float a0[CH], p0[CH], q0[CH], a1[CH], p1[CH], q1[CH];
    auto ld = [&](float (&a)[CH], float (&b0)[CH], float (&b1)[CH], int s0) {
        const float* w = wp + s0 * astep; const float* x = xp + 4 * s0 * LD;
#pragma unroll
        for (int q = 0; q < CH; ++q) { a[q] = w[q * astep]; b0[q] = x[4 * q * LD]; b1[q] = x[4 * q * LD + 16]; }
    };
    auto mm = [&](const float (&a)[CH], const float (&b0)[CH], const float (&b1)[CH], int s0) {
#pragma unroll
        for (int q = 0; q < CH; ++q)
            if (s0 + q < nf) {                         // (uniform)
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b0[q], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b1[q], acc1, 0, 0, 0);
            }
    };
    if (nf > 0) ld(a0, p0, q0, 0);
    for (int s0 = 0; s0 < nf; s0 += 2 * CH) {
        if (s0 + CH < nf) ld(a1, p1, q1, s0 + CH);
        mm(a0, p0, q0, s0);
        if (s0 + 2 * CH < nf) ld(a0, p0, q0, s0 + 2 * CH);
        if (s0 + CH < nf) mm(a1, p1, q1, s0 + CH);
    }
    if ((ke - kb) & 3) {                               // the partial step: clamped row of X, masked A
        const int k = kb + 4 * nf + kk, kc = min(k, ke - 1);
        const float w = TRN ? Ws[(size_t)kc * ldw + mi] : Ws[(size_t)mi * ldw + kc];
        const float av = k < ke ? w : 0.f;
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Xs[kc * LD + i], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Xs[kc * LD + i + 16], acc1, 0, 0, 0);
    }
}

// e / d for e d < 2^32 without the ~30-instruction integer division: one v_mul_hi_u32 with m = ceil(2^32 / d) (d >= 2)
__device__ __forceinline__ unsigned mg_magic(unsigned d) { return d < 2 ? 0u : (unsigned)((0x100000000ull + d - 1) / d); }
__device__ __forceinline__ int mg_div(int e, unsigned m) { return m ? (int)__umulhi((unsigned)e, m) : e; }

// L2 warm-up.  Parameters that another role has just rewritten (write-through) sit in memory, and the trial workgroups of an
// XCD all walk them in the same order at the same time: every batch of operand loads would be a miss that all of them wait
// for together.  Instead each workgroup first touches one sixteenth of the range (16-byte loads, all in flight, nothing kept):
// between them the 16 trial workgroups that usually share an XCD bring all of it into that XCD's L2 in ONE round trip.
// Which workgroups share an XCD is a placement guess (blockIdx round-robin); a wrong guess costs speed, never correctness.
__device__ __forceinline__ void mg_warm(const float* base, int nfloats, int wg, int tid) {
    const int nq = nfloats >> 2, per = (nq + 15) >> 4, q0 = ((wg >> 3) & 15) * per;
    const __amdgpu_buffer_rsrc_t rb = vjf_rsrc(base);
    for (int q = q0 + tid; q < min(nq, q0 + per); q += VJF_MG_THREADS) {
        const float4 v = vjf_ld4_sc1(rb, q * 4);
        asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
    }
}

// the same with the loads left in flight (two per thread; a longer range finishes the blocking way): the caller goes on issuing
// its own loads and retires these behind them
__device__ __forceinline__ void mg_warm_issue(const float* base, int nfloats, int wg, int tid, float4 (&r)[2]) {
    const int nq = nfloats >> 2, per = (nq + 15) >> 4, q0 = ((wg >> 3) & 15) * per, q1 = min(nq, q0 + per);
    const __amdgpu_buffer_rsrc_t rb = vjf_rsrc(base);
    r[0] = r[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q0 + tid < q1) r[0] = vjf_ld4_sc1(rb, (q0 + tid) * 4);
    if (q0 + tid + VJF_MG_THREADS < q1) r[1] = vjf_ld4_sc1(rb, (q0 + tid + VJF_MG_THREADS) * 4);
    for (int q = q0 + tid + 2 * VJF_MG_THREADS; q < q1; q += VJF_MG_THREADS) {
        const float4 v = vjf_ld4_sc1(rb, q * 4);
        asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
    }
}
__device__ __forceinline__ void mg_warm_retire(const float4 (&r)[2]) {
    asm volatile("" ::"v"(r[0].x), "v"(r[0].y), "v"(r[0].z), "v"(r[0].w), "v"(r[1].x), "v"(r[1].y), "v"(r[1].z), "v"(r[1].w));
}

// centroids (transposed: [input dim][centre], 16-byte rows) and -1/(2 w^2): constants of the launch (functional.py:11-22).  Every
// role that forms RBF features (trial, moments, Gram) stages them with this one routine: all of them hold the same bytes.
__device__ __forceinline__ void mg_stage_centres(const VjfPlan& P, const float* S, float* s_cen, float* s_iw, const int tid) {
    constexpr int NT = VJF_MG_THREADS;
    const int n = P.n, dxu = P.dxu, npad = (n + 3) & ~3;
    const float* cen = S + P.off[VJF_SLOT_CENTROID];
    const float* lw = S + P.off[VJF_SLOT_LOGWIDTH];
    for (int e = tid; e < npad * dxu; e += NT) { const int c = e / npad, k = e - c * npad; s_cen[e] = k < n ? cen[k * dxu + c] : 0.f; }
    for (int e = tid; e < npad; e += NT) { float v = 0.f; if (e < n) { const float w = expf(lw[e]); v = -0.5f / (w * w); } s_iw[e] = v; }
}

#define VJF_MG_STAMP(i)                                                                     \
    do {                                                                                    \
        if (A.stamps && wg == 0 && tid == 0) {                                              \
            unsigned long long t_;                                                          \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");  \
            A.stamps[(size_t)(t & 31) * 32 + (i)] = t_;                                     \
        }                                                                                   \
    } while (0)

// latest (i) / earliest (j, stored complemented) time over ALL trial workgroups
#define VJF_MG_STAMPX(i, j)                                                                 \
    do {                                                                                    \
        if (A.stamps && tid == 0) {                                                         \
            unsigned long long t_;                                                          \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");  \
            atomicMax(A.stamps + (size_t)(t & 31) * 32 + (i), t_);                          \
            if ((j) >= 0) atomicMax(A.stamps + (size_t)(t & 31) * 32 + (j), ~t_);           \
        }                                                                                   \
    } while (0)

// per-workgroup times of the LAST step of a launch (8 words per trial workgroup behind the 32 x 32 ring)
#define VJF_MG_STAMPW(i)                                                                    \
    do {                                                                                    \
        if (A.stamps && tid == 0 && t == A.T - 1 && !replay) {                              \
            unsigned long long t_;                                                          \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");  \
            A.stamps[1024 + (size_t)wg * 8 + (i)] = t_;                                     \
        }                                                                                   \
    } while (0)

// one 16x16 tile of  G[m][j] = sum_{b<32} D[m0+m][b] * Bop[j0+j][b],  Bop = [Bact (Kin rows) | ones | 0..]  -> block `blk` of the
// late slab ([j][ldm], see vjf_mega_slab_layout): a lane's four registers are G[m .. m+3][j], one 16-byte store
__device__ __forceinline__ void mg_grad_tile(const float* D, int M, int m0, const float* Bact, int Kin, int j0, const float* s_one,
                                             const float* s_zero, float* blk, int ldm, int rows, bool first, int lane) {
    constexpr int LD = VJF_MG_LD;
    const int i = lane & 15, kk = lane >> 4;
    const float* arow = ((m0 + i) < M ? D + (size_t)(m0 + i) * LD : s_zero) + kk;
    const int jj = j0 + i;
    const float* brow = (jj < Kin ? Bact + (size_t)jj * LD : (jj == Kin ? s_one : s_zero)) + kk;
    float a[8], b[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) { a[s] = arow[4 * s]; b[s] = brow[4 * s]; }
    vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 8; s += 2) {                   // two chains: the MFMAs issue back to back
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s + 1], b[s + 1], acc1, 0, 0, 0);
    }
    acc += acc1;
    const int mq = m0 + 4 * (lane >> 4), j = j0 + (lane & 15);      // (rows m >= M of D are the zero row: the padding columns get 0)
    if (j < rows && mq < ldm) {
        float* p = blk + (size_t)j * ldm + mq;
        if (!first) { acc[0] += vjf_ld_sc1(p); acc[1] += vjf_ld_sc1(p + 1); acc[2] += vjf_ld_sc1(p + 2); acc[3] += vjf_ld_sc1(p + 3); }   // (a later tile of the workgroup)
        vjf_st4_wt(p, acc[0], acc[1], acc[2], acc[3]);
    }
}

// ---- the gradient tiles of a step as ONE table (vjf_mega_kernel: `GTAB` in vjf_mega_trial.h).  Which tiles a step has, where their
// operands lie in the trial role's LDS and where they go in the late slab is a function of the plan alone: the host builds the list
// once per context (vjf_abi.hip), the kernel reads it with scalar loads.  VJF_GT_HDR header words -- [0] tiles, [1] segments, [2 + s]
// the end (exclusive) of segment s -- then VJF_GT_ENT words per tile, in the order the per-tensor loops walk them:
//   [0] first float of row m0 of D in LDS        [1] M - m0: rows of D from there on (lanes beyond read the zero row)
//   [2] first float of row j0 of Bact in LDS     [3] Kin - j0: rows of Bact from there on (the lane AT it reads the ones row, beyond: zeros)
//   [4] first float of the tile in the late slab: off + j0 ldm + m0      [5] ldm
//   [6] rows - j0: slab rows the tile stores     [7] ldm - m0: slab columns it stores
// A tile that would store nothing is not listed (the mean head has no bias: its column tile that holds the ones row alone).
// The table starts on a 32-byte boundary (an entry is one s_load_dwordx8): VJF_GT_AT(slab_len) words behind the slab's group words.
// Segment 0: decoder, both heads, the last two layers -- everything whose deltas exist when the walk starts; one more segment per
// deeper layer (its delta is formed in between).  Wavefront w takes tiles w, w + 8, ... of the WHOLE list, segment by segment, so
// the eight shares differ by at most one tile.
#define VJF_GT_HDR 16
#define VJF_GT_ENT 8
#define VJF_GT_AT(slab_len) ((((slab_len) >> 2) + 7) & ~7)
static inline int vjf_mega_grad_tiles(const VjfPlan& P, int* tab) {      // -> words of the table; tab == nullptr: only that
    constexpr int LD = VJF_MG_LD;
    const VjfMegaTrialLds Lo = vjf_mega_trial_lds(P);
    const VjfMegaSlab SL = vjf_mega_slab_layout(P);
    const bool compact = P.dy >= P.hmax;
    const int d0 = compact ? Lo.py : Lo.dd, d1 = compact ? Lo.dd : Lo.dd + P.hmax * LD;
    const int hL = P.h[P.L - 1];
    int nt = 0, nseg = 0;
    if (tab) for (int k = 0; k < VJF_GT_HDR; ++k) tab[k] = 0;
    auto tensor = [&](int D, int M, int Bact, int Kin, int blk) {
        const int ntm = (M + 15) >> 4, ntj = (Kin + 1 + 15) >> 4, ldm = SL.ldm[blk], rows = SL.rows[blk];
        for (int tm = 0; tm < ntm; ++tm)
            for (int tj = 0; tj < ntj; ++tj) {
                const int m0 = 16 * tm, j0 = 16 * tj;
                if (rows - j0 <= 0 || ldm - m0 <= 0) continue;
                if (tab) {
                    int* e = tab + VJF_GT_HDR + VJF_GT_ENT * nt;
                    e[0] = D + m0 * LD; e[1] = M - m0; e[2] = Bact + j0 * LD; e[3] = Kin - j0;
                    e[4] = SL.off[blk] + j0 * ldm + m0; e[5] = ldm; e[6] = rows - j0; e[7] = ldm - m0;
                }
                ++nt;
            }
    };
    auto layer = [&](int l) {
        int aoff = 0;
        for (int q = 0; q < l - 1; ++q) aoff += P.h[q];
        tensor(((P.L - 1 - l) & 1) ? d1 : d0, P.h[l], l > 0 ? Lo.act + aoff * LD : Lo.in, l > 0 ? P.h[l - 1] : P.din, 3 + (P.L - 1 - l));
    };
    auto close = [&]() { if (tab) tab[2 + nseg] = nt; ++nseg; };
    tensor(Lo.dpy, P.dy, Lo.xt, P.dz, 0);
    tensor(Lo.dmu, P.dz, Lo.act + (P.hsum - hL) * LD, hL, 1);
    tensor(Lo.dlv, P.dz, Lo.act + (P.hsum - hL) * LD, hL, 2);
    layer(P.L - 1);
    if (P.L >= 2) layer(P.L - 2);
    close();
    for (int l = P.L - 3; l >= 0; --l) { layer(l); close(); }
    if (tab) { tab[0] = nt; tab[1] = nseg; }
    return VJF_GT_HDR + VJF_GT_ENT * nt;
}

typedef __attribute__((address_space(4))) const int mg_cst_i;       // constant address space: a uniform load from it is a scalar load
typedef int mg_i8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(4))) const mg_i8 mg_cst_i8;     // (a table entry: 32 bytes, 32-byte aligned)
typedef __attribute__((address_space(3))) const float mg_lds_cf;    // an LDS pointer by type / a global-memory pointer by type: a value that
typedef __attribute__((address_space(1))) const float mg_glb_cf;    // lives in LDS in one plan and in memory in another is read through one of
                                                                    // these on either side of a select, never through a selected generic pointer

// This wavefront's tiles q, q + 8, ... < qend of the table above: mg_grad_tile's arithmetic -- the same operands, the same two chains
// (even k-steps / odd k-steps), acc += acc1, the same store -- with the row offsets from the table and all sixteen operand reads at
// immediate offsets from two per-lane bases.  LOOK: the NEXT tile's sixteen reads are issued in front of this tile's chains and
// store (sixteen more live registers); they stay in front of the store because that is an asm with a memory clobber, and the
// compiler's own wait for them comes behind it, at their use.  `q` is left at the wavefront's first tile of the next segment.
// (LOOK fits vjf_mega_kernel's registers and is slower than none -- profiles/grad_tiles_bench.txt --: the kernel walks without it; the
//  form stays for tools/grad_tile_bench.hip.)
template <bool LOOK>
__device__ __forceinline__ void mg_grad_walk(const int* table, int& q, const int qend, const float* smem, const int one, const int zero,
                                             float* late, const bool first, const int lane) {
    constexpr int LD = VJF_MG_LD, NW = VJF_MG_WAVES;
    mg_cst_i* tab = (mg_cst_i*)table + VJF_GT_HDR;
    mg_lds_cf* lds = (mg_lds_cf*)smem;
    const int i = lane & 15, kk = lane >> 4, row = i * LD + kk;
    // a tile's eight words by ONE scalar load, in front of everything that uses them (word by word, each at its first use, they were
    // seven dependent round trips a tile -- and a scalar load's wait is lgkmcnt(0): it waits for every LDS read in flight as well)
    auto ent = [&](int qq) { return *(const mg_cst_i8*)(tab + VJF_GT_ENT * qq); };
    auto rd = [&](const mg_i8 e, float (&a)[8], float (&b)[8]) {
        const int ao = i < e[1] ? e[0] + row : zero + kk;
        const int bo = i < e[3] ? e[2] + row : ((i == e[3] ? one : zero) + kk);
#pragma unroll
        for (int s = 0; s < 8; ++s) { a[s] = lds[ao + 4 * s]; b[s] = lds[bo + 4 * s]; }
    };
    auto fin = [&](const mg_i8 e, const float (&a)[8], const float (&b)[8]) {
        vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; s += 2) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s + 1], b[s + 1], acc1, 0, 0, 0);
        }
        acc += acc1;
        if (i < e[6] && 4 * kk < e[7]) {
            float* p = late + e[4] + i * e[5] + 4 * kk;
            if (!first) { acc[0] += vjf_ld_sc1(p); acc[1] += vjf_ld_sc1(p + 1); acc[2] += vjf_ld_sc1(p + 2); acc[3] += vjf_ld_sc1(p + 3); }   // (a later tile of the workgroup)
            vjf_st4_wt(p, acc[0], acc[1], acc[2], acc[3]);
        }
    };
    if (LOOK) {
        float a0[8], b0[8], a1[8], b1[8];
        mg_i8 e0 = {}, e1 = {};
        if (q < qend) { e0 = ent(q); rd(e0, a0, b0); }
        while (q < qend) {
            if (q + NW < qend) { e1 = ent(q + NW); rd(e1, a1, b1); }
            fin(e0, a0, b0);
            q += NW;
            if (q >= qend) break;
            if (q + NW < qend) { e0 = ent(q + NW); rd(e0, a0, b0); }
            fin(e1, a1, b1);
            q += NW;
        }
    } else {
        float a[8], b[8];
        for (; q < qend; q += NW) { const mg_i8 e = ent(q); rd(e, a, b); fin(e, a, b); }
    }
}
// loss sums of step t over the trial workgroups' late slabs: fp64, 32 strided partial sums per scalar, then a fixed xor tree -> s_sc[RS_*]
// (the residual leaves as the mean square).  A workgroup-wide call (one barrier); read with sc1 loads behind the caller's wait.
__device__ __forceinline__ void mg_sum_losses(const VjfMegaArgs& A, int t, float* s_sc, int tid, float Bf, int dz, bool want_resid) {
    const int ring = 8 * (t % VJF_MG_RING);
    if (tid < 32 * 5) {
        const int sc = tid >> 5, l = tid & 31, slot = sc < RS_SDX2 ? sc : RS_RESID;
        double d = 0.0;
        if (sc < RS_SDX2 || want_resid)
            for (int w = l; w < A.n_trial; w += 32) d += (double)vjf_ld_sc1(A.slab_late + (size_t)w * A.late_len + A.slab_len + ring + slot);
        d = vjf_sum32(d);
        // (the residual leaves as the mean square: its sum over 32768 x 16 elements has more digits than a float keeps)
        if (l == 0) s_sc[slot] = slot == RS_RESID ? (float)(d / ((double)Bf * (double)dz)) : (float)d;
    }
    __syncthreads();
}

#define MG_PHASE()                                                        \
    do {                                                                  \
        tid = tid0;                                                       \
        asm volatile("" : "+v"(tid));                                     \
        lane = tid & 63;                                                  \
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);                  \
    } while (0)

// mg_var2 / mg_mma2_mm16 for NG column groups of 16 trials (NG = 2: one tile, LD = 33; NG = 4: two tiles side by side, LD = 65 --
// every operand load of L^-1 and W then feeds twice the multiply-adds).  A trial's sums run over k in the same order whatever NG
// is: the same bits.  Every k-step is clamped and masked here: the split of mg_var2 into full and partial steps takes the moments
// role's kernels from 92 / 100 to 224 bytes of scratch, with or without look-ahead (profiles/var_interior_isa.txt).
template <int NG, int LD>
__device__ __forceinline__ void mg_varN(float (&v2)[NG], __amdgpu_buffer_rsrc_t rx, int n, int j0A, int KA, int j0B, int KB, mg_lds_cf* Xs, int lane,
                                        const bool upper = true) {        // upper = false (uniform): column groups 2, 3 hold no trials, their multiply-adds are skipped
    if (j0A < 0) return;
    const int i = lane & 15, kk = lane >> 4;
    const bool rvA = (j0A + i) < n, rvB = j0B >= 0 && (j0B + i) < n;
    const int offA = (rvA ? j0A + i : 0) * n + 4 * kk, offB = (rvB ? j0B + i : 0) * n + 4 * kk;
    mg_lds_cf* xp = Xs + i;
    const int ntA = (KA + 15) >> 4, ntB = j0B >= 0 ? (KB + 15) >> 4 : 0;
    const int SA = (ntA + 3) >> 2, SB = (ntB + 3) >> 2, S = SA + SB;
    vjf_f32x4 acc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
    auto fold = [&]() {
#pragma unroll
        for (int g = 0; g < NG; ++g) v2[g] = fmaf(acc[g][0], acc[g][0], fmaf(acc[g][1], acc[g][1], fmaf(acc[g][2], acc[g][2], fmaf(acc[g][3], acc[g][3], v2[g]))));
    };
    auto ldb = [&](float4 (&a)[4], int sb) {
        const bool inB = sb >= SA;
        const int t0 = 4 * (inB ? sb - SA : sb), off = inB ? offB : offA;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int kq = 16 * (t0 + q) + 4 * kk; a[q] = vjf_ld4_plain(rx, off + (kq + 3 < n ? 16 * (t0 + q) : 0)); }   // (plain: L^-1 of a launch without an RLS update is written once, before its first read)
    };
    auto mmb = [&](const float4 (&a)[4], int sb) {
        const bool inB = sb >= SA;
        const int t0 = 4 * (inB ? sb - SA : sb), nt = inB ? ntB : ntA, ke = inB ? KB : KA;
        const bool rv = inB ? rvB : rvA;
        if (sb == SA && SA > 0) {
            fold();
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (t0 + q < nt) {
                const int k0 = 16 * (t0 + q) + 4 * kk;
                const float av[4] = {a[q].x, a[q].y, a[q].z, a[q].w};
                // the four k-steps' B operands first, then their multiply-adds: ONE LDS round trip per block of 16 k instead of one per
                // k-step (the ISA of the trial role's mg_var2 waits on lgkmcnt in front of nearly every pair of MFMAs)
                float bv[4][NG];
                float vv[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k = k0 + c, kc = min(k, ke - 1);
                    vv[c] = (rv && k < ke) ? av[c] : 0.f;
#pragma unroll
                    for (int g = 0; g < (NG < 2 ? NG : 2); ++g) bv[c][g] = xp[kc * LD + 16 * g];
                    if (NG > 2 && upper) {
#pragma unroll
                        for (int g = 2; g < NG; ++g) bv[c][g] = xp[kc * LD + 16 * g];
                    }
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
#pragma unroll
                    for (int g = 0; g < (NG < 2 ? NG : 2); ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[c], bv[c][g], acc[g], 0, 0, 0);
                    if (NG > 2 && upper) {
#pragma unroll
                        for (int g = 2; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[c], bv[c][g], acc[g], 0, 0, 0);
                    }
                }
            }
        }
    };
    float4 a0[4], a1[4], a2[4];
    ldb(a0, 0);
    if (S > 1) ldb(a1, 1);
    if (S > 2) ldb(a2, 2);
    for (int sb = 0; sb < S; sb += 3) {
        mmb(a0, sb);
        if (sb + 3 < S) ldb(a0, sb + 3);
        if (sb + 1 < S) { mmb(a1, sb + 1); if (sb + 4 < S) ldb(a1, sb + 4); }
        if (sb + 2 < S) { mmb(a2, sb + 2); if (sb + 5 < S) ldb(a2, sb + 5); }
    }
    fold();
}
template <int NG, int LD>
__device__ __forceinline__ void mg_mmaN_mm16(vjf_f32x4 (&acc)[NG], const float (&a)[16], const float* Xs, int M, int m0, int kb, int ke, int s0, int lane,
                                             const bool upper = true) {
    const int i = lane & 15, kk = lane >> 4;
    const bool rv = (m0 + i) < M;
    const float* xp = Xs + i;
    const int nst = (ke - kb + 3) >> 2, klast = ke - 1;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (s0 + q < nst) {
            const int k = kb + 4 * (s0 + q) + kk;
            const int kc = min(k, klast);
            const float av = (rv && k < ke) ? a[q] : 0.f;
#pragma unroll
            for (int g = 0; g < (NG < 2 ? NG : 2); ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xp[kc * LD + 16 * g], acc[g], 0, 0, 0);
            if (NG > 2 && upper) {
#pragma unroll
                for (int g = 2; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xp[kc * LD + 16 * g], acc[g], 0, 0, 0);
            }
        }
    }
}
