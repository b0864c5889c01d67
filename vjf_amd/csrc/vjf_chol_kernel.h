// vjf_chol_kernel.h -- fast path of the once-per-step serial half for n_rbf <= 224.
//
//   vjf_chol_lds_kernel (one workgroup, 8 wavefronts): L = chol(P) (module.py:99),
//       W = P^-1 g (module.py:101), w_chol = L^-T (module.py:102), residual -> state-noise
//       running variance (model.py:373-377).  The matrix lives in LDS as 32x32 blocks with
//       33-float rows; all block products run on the f32 matrix cores (v_mfma_f32_32x32x2_f32).
//       The two column-sequential pieces (diagonal-block Cholesky, triangular block solve) are
//       written as chains of rank-1 MFMA updates on an accumulator tile: the symmetric tile has
//       row j already spread over the lanes (column index on the lane), which is exactly the
//       A- and B-operand layout, so a column step is  readlane(pivot) -> rsqrt -> scale -> MFMA
//       with no cross-lane data movement.
// (the operand / SGD kernels in front of it: vjf_rls_operands.h; the block primitives and the diagonal chain: vjf_chol_blocks.h)
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_chol_blocks.h"
#include "vjf_gram_kernel.h"   // vjf_f32x16
#include "vjf_handoff.h"
#include "vjf_plan.h"
#include "vjf_step_math.h"

#define VJF_CHOL_THREADS 512
#define VJF_CHOL_MAXBLK 7                 // n <= 224

struct VjfCholArgs {
    float* state;
    const float* red;
    const float* gbuf;     // from vjf_prep_kernel
    int B_total;
    unsigned flags;
    unsigned long long* stamps;   // diagnostic only (null in normal runs): s_memrealtime (100 MHz, one clock for the whole device) at phase boundaries
    float* dinv_out;       // post mode: nbl blocks (32x32 row-major) of inverted diagonal blocks for vjf_rls_post_kernel
    int* ok_out;           // post mode: 1 = factor valid
    int post;              // 1: stop after L and the inverted diagonal blocks; the many-CU post kernels do the rest
    float* lscr;           // post mode: (n, n) scratch that receives L column by column while the factorisation runs
    unsigned* flags_out;   // post mode: flags_out[k] = (epoch << 1) | failed once column k of L and Dinv_k are in global memory:
    unsigned epoch;        //   vjf_rls_post_kernel, launched beside this kernel, consumes the columns as they appear
    float* pscr;           // post mode: lower 32x32 blocks of P (with the identity padding), block after block, row-major: written
                           //   here with P_new; self_prep reads P_old from it (the copy a Cholesky kernel left for the next one)
    int self_prep;         // post mode: 1 = P_new = P_old (pscr) + Phi^T Phi / v is formed HERE, in registers, once sigma of the
                           //   previous step is there (wait_count reaches wait_target): the operand kernel that updates the state's
                           //   P and forms g runs beside this kernel, on the post kernel's stream, instead of before it
    const unsigned* wait_count; unsigned wait_target;
    int src_state;         // self_prep: P_old comes from the state's P (first step of a sequence) instead of pscr
    // looping form (the Cholesky role of the one-launch route, vjf_mega_kernel.h): nsteps > 0 -> ONE launch runs the factorisations of nsteps consecutive steps on its CU
    // (a kernel of this size is not placed while trial-kernel workgroups hold LDS on every CU; resident, it starts the moment
    // sigma arrives).  Step `it`: epoch + it, statistics in red (even step0 + it) or red2 (odd), ready when *stat_count has
    // reached stat_target + it * stat_stride; sigma when *wait_count has reached wait_target + it * wait_stride.
    int nsteps, step0;
    unsigned inject_epoch; // test hook (VJF_DEBUG_INJECT=k): at this epoch the statistics wait is reported as timed out
    const float* red2;
    const unsigned* stat_count; unsigned stat_target, stat_stride, wait_stride;
    const unsigned long long* sig_word;   // non-null (self_prep): sigma of the previous step arrives as ONE 8-byte word {epoch, bits} from the
                                          //   y / W loop; *wait_count is then only awaited before the first column goes out (the scratch
                                          //   copies of L and the inverted diagonal blocks must have been read by everybody)
    int no_triclean;       // post mode: the caller clears the zero halves of w_chol / w_pchol itself (vjf_triclean_kernel)
                           //            (vjf_rls_post_kernel copies it to w_pchol once the factor is known to be good)
};

#define VJF_STAMP(i)                                                                        \
    do {                                                                                    \
        if (A.stamps && tid == 0) {                                                         \
            unsigned long long t_;                                                          \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");      \
            A.stamps[((it_epoch & 7u) << 5) * (A.nsteps > 0 ? 1 : 0) + (i)] = t_;              \
        }                                                                                   \
    } while (0)

static inline int vjf_chol_dzp(int dz) { return dz <= 4 ? 4 : dz <= 8 ? 8 : dz <= 12 ? 12 : dz <= 16 ? 16 : 32; }
// The control words behind s_g: [0] ok, [2] [3] sigma's bits / "there", [4..13] the column loop's hand-off words, [16..31] eight
// doubles of the final reduction.  (The block-row / block-column table of the lower blocks needs no room here: entry b sits in
// the one float of block b that belongs to no element.)  With 32 floats the largest plans keep the sizes they had with
// 1024-float blocks and 192 control floats within the same budget: nbl = 6, dzp = 32 is 163,328 B, the bound itself.
#define VJF_CHOL_CTL_FLOATS 32
static inline size_t vjf_chol_lds_bytes(const VjfPlan& P, int dzp) {            // dynamic LDS of vjf_chol_loop<dzp>
    const int nbl = (P.n + 31) / 32;
    const size_t blocks = (size_t)(nbl * (nbl + 1) / 2 + nbl) * VJF_BLK_FLOATS;
    return (blocks + (size_t)nbl * 32 * dzp * (dzp <= 16 ? 1 : 2) + VJF_CHOL_CTL_FLOATS) * 4;   // dzp = 32: y = L^-1 g has a region of its own
}
static inline size_t vjf_chol_lds_bytes(const VjfPlan& P) { return vjf_chol_lds_bytes(P, vjf_chol_dzp(P.dz)); }
static inline bool vjf_chol_lds_ok(const VjfPlan& P) {
    return (P.n + 31) / 32 <= VJF_CHOL_MAXBLK && P.n % 4 == 0 && P.dz <= 32 && vjf_chol_lds_bytes(P) <= 160 * 1024 - 512;
}

#define VJF_CHOL_Q 14          // float4 chunks per thread when sweeping the <= 28 lower blocks

// acc[0..DZP) += x * row[0..DZP)   (row: 16-byte aligned LDS, same address on every lane => broadcast)
template <int DZP>
__device__ __forceinline__ void axpy_row(float (&acc)[DZP], float x, const float* row) {
#pragma unroll
    for (int j = 0; j < DZP; j += 4) {
        const float4 w = *reinterpret_cast<const float4*>(row + j);
        acc[j] = fmaf(x, w.x, acc[j]); acc[j + 1] = fmaf(x, w.y, acc[j + 1]);
        acc[j + 2] = fmaf(x, w.z, acc[j + 2]); acc[j + 3] = fmaf(x, w.w, acc[j + 3]);
    }
}

// The lower block triangle is swept as float4 chunks, 256 per 32x32 block: chunk idx -> block, row in the block, first of its four columns
__device__ __forceinline__ void chol_tile_of(int idx, int& b, int& r, int& c4) { b = idx >> 8; r = (idx >> 3) & 31; c4 = (idx & 7) * 4; }

// The off-diagonal blocks on the other side of the diagonal (upper for w_pchol, lower for w_chol) are zero and stay zero: they
// are cleared once per state blob (VJF_SC_TRI_CLEAN), not every step.  Element e of the (n, n) matrices.
// (one element, not the sweep: as a routine that takes first element and stride, vjf_triclean_kernel needs 10 VGPRs for 8 --
//  profiles/chol_split_isa.txt)
__device__ __forceinline__ void chol_triclean_at(float* Lm, float* Wc, int n, int e) {
    const int i = e / n, j = e - i * n;
    if ((i >> 5) < (j >> 5)) Lm[e] = 0.f;
    if ((i >> 5) > (j >> 5)) Wc[e] = 0.f;
}

template <int DZP>
__device__ __forceinline__ void vjf_chol_body(const VjfPlan& P, const VjfCholArgs& A, float* lds, int* s_dead, const unsigned it_epoch,
                                              const float* it_red, const unsigned it_wait_target, const unsigned it_stat_target,
                                              const bool it_src_state) {
    int tid = threadIdx.x;
    // (the looping form calls this body once per step: without the barrier the compiler hoists every lane-dependent address
    //  of the body out of that loop and spills hundreds of registers)
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const int n = P.n, dz = P.dz;
    const int nbl = (n + 31) / 32, npad = nbl * 32, ntri = nbl * (nbl + 1) / 2;
    float* S = A.state;
    float* SC = S + P.off[VJF_SLOT_SCALARS];
    const bool do_upd = A.flags & VJF_FLAG_UPDATE, warm = A.flags & VJF_FLAG_WARM_UP;
    if (!do_upd) return;
    if (A.post && warm) return;                      // no RLS in warm-up; the residual / sigma kernels run on their own
    // "running": the caller keeps the post kernel (2 nbl + 1 workgroups that each take a whole CU's LDS) behind a one-wavefront
    // gate on this word, so that they do not sit on 15 CUs before there is anything for them to do
    // (self_prep: the word is stored once this step's operands are in registers -- the operand kernel, which overwrites the
    //  state's P, starts behind a gate on it)
    if (A.post && !A.self_prep && tid == 0) vjf_st_wt(A.flags_out + VJF_CHOL_MAXBLK + 2, it_epoch);
    float* s_blk = lds;                               // ntri blocks: lower block triangle of P -> L -> L^-1
    float* s_aux = s_blk + (size_t)ntri * VJF_BLK_FLOATS;       // nbl blocks: inverted diagonal blocks of L; later scratch
    float* s_g = s_aux + (size_t)nbl * VJF_BLK_FLOATS;          // npad x DZP  g, later W
    // (y = L^-1 g overwrites g in place; for DZP = 32 a second npad x DZP region behind g is reserved)
    int* s_flag = (int*)(s_g + (size_t)npad * DZP * (DZP <= 16 ? 1 : 2));   // [0] ok
    double* s_d = (double*)(s_flag + 16);             // 8 doubles for the final reduction (one per wavefront)
    int* s_tab = (int*)s_blk + (VJF_BLK_FLOATS - 1);  // s_tab[b * VJF_BLK_FLOATS]: first row << 16 | first column of lower block b
    auto tile_at = [&](int b, int& gi0, int& gj0) { const int v = s_tab[(size_t)b * VJF_BLK_FLOATS]; gi0 = v >> 16; gj0 = v & 0xffff; };

    float* Wm = S + P.off[VJF_SLOT_W_MEAN];
    float* Wc = S + P.off[VJF_SLOT_W_CHOL];
    float* Pm = S + P.off[VJF_SLOT_W_PREC];
    float* Lm = S + P.off[VJF_SLOT_W_PCHOL];
    const float* G = it_red + P.red_G;
    const float* FDX = it_red + P.red_FDX;
    float sig = S[P.off[VJF_SLOT_TR_LOGVAR]];
    const float lam = vjf_shrink_of(SC[VJF_SC_SHRINK]);
    const float Bf = (float)A.B_total;
    unsigned st = 0;
    const bool sp = A.post && A.self_prep;
    VJF_STAMP(0);
    // (the entries of the table sit in ONE bank, VJF_BLK_FLOATS % 32 == 0: 28 lanes of a wavefront storing them was a 28-way
    //  conflict; lane 0 of every wavefront stores its <= 4 entries one after the other instead.  Readers of an entry are the
    //  lanes of one wavefront with the same b: a broadcast)
    if (lane == 0)
        for (int b = wave; b < ntri; b += VJF_CHOL_THREADS / 64) {
            int bi = 0;
            while ((bi + 1) * (bi + 2) / 2 <= b) ++bi;
            s_tab[(size_t)b * VJF_BLK_FLOATS] = (bi * 32) << 16 | (b - bi * (bi + 1) / 2) * 32;
        }
    if (tid == 0) s_flag[0] = 1;
    if (tid < 10) s_flag[4 + tid] = 0;                  // the column loop's hand-off words (below)
    __syncthreads();
    // (the statistics of the step: the Gram role's write-through stores, read with sc1 loads behind their count -- an acquire as
    //  well only in the VJF_HANDOFF_ACQUIRE=1 form.  The wait sits below, between this thread's loads of P, which do not depend on
    //  the statistics, and its loads of G: at the first step of a launch nothing else hides the 108 KB of P)
    auto stat_wait = [&]() {
        if (A.stat_count && (!vjf_wg_wait_sc1(A.stat_count, it_stat_target, tid, SC + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u) || (A.inject_epoch && tid == 0 && it_epoch == A.inject_epoch))) {
            vjf_status_or(SC + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_STATS);
            *s_dead = 1;
        }
    };
    if (warm) stat_wait();

    // The phases below stay in this function: as routines of their own the intake, the column loop (one routine per kind of
    // wavefront), the roll-back and the one-workgroup tail each put a kernel's lane-spill count above the parent's, and the
    // state-noise tail moves code in eleven kernels, which no GPU run has timed (profiles/chol_split_isa.txt has the figures
    // of every form that was tried).
    if (!warm) {
        // ==== the intake
        // ---- load the lower block triangle of P_new (vjf_prep_kernel already added Phi^T Phi / v).  Wavefront 0 takes the
        //      first diagonal block alone and starts its column chain; the other seven bring in the rest meanwhile.
        //      All loads of a thread are issued before its first LDS store.
        auto diag_chain = [&](int k) {                                  // L_kk and L_kk^-1 in one chain (one wavefront)
            float* dk = s_blk + (size_t)vtri(k, k) * VJF_BLK_FLOATS;
            const bool good = potrf_inv_chain2(dk, s_aux + (size_t)k * VJF_BLK_FLOATS, lane, min(32, n - 32 * k));
            if (!good && lane == 0) s_flag[0] = 0;
            return good;
        };
        bool chain_good = true;                                         // wavefront 0: every pivot so far was positive
        auto pad4 = [](int gi, int gj) {                                // identity padding outside the matrix
            return make_float4(gi == gj ? 1.f : 0.f, gi == gj + 1 ? 1.f : 0.f, gi == gj + 2 ? 1.f : 0.f, gi == gj + 3 ? 1.f : 0.f);
        };
        // self_prep: every thread first issues its loads of P_old (pscr) and of G, then the workgroup waits for sigma of the
        // previous step, and P_new = lambda P_old + G / v is formed in the registers (as vjf_prepg_kernel forms the state's P).
        // Either way the blocks of P_new go to pscr for the next step's kernel.
        bool lscr_guard = false;                                        // the post workgroups' exit count is still to be checked
        auto sigma_wait = [&]() {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // operands in registers: the state's P may now be overwritten
            __syncthreads();
            if (tid == 0) vjf_st_wt(A.flags_out + VJF_CHOL_MAXBLK + 2, it_epoch);
            vjf_chaos(tid, A.wait_count, 1);
            if (A.sig_word && it_wait_target != 0u) {
                // sigma inside the hand-off word: one poll, no second load; the exit count of the post workgroups is checked by the
                // wavefront that writes the first column out (below)
                if (tid == 0) {
                    bool there = false;
                    unsigned bits = 0u;
                    for (unsigned spins = 0; spins < VJF_WAIT_SPINS; ++spins) {          // (its own loop, not vjf_poll_count: 64 bits, the payload rides in the word)
                        const unsigned long long v = __hip_atomic_load(A.sig_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if ((unsigned)(v >> 32) == it_epoch - 1u) { there = true; bits = (unsigned)v; break; }
                        if ((spins & 255u) == 255u && vjf_abort_seen(SC + VJF_SC_STATUS)) break;
                        __builtin_amdgcn_s_sleep(1);
                    }
                    s_flag[2] = (int)bits; s_flag[3] = there ? 1 : 0;
                }
                __syncthreads();
                sig = __uint_as_float((unsigned)s_flag[2]);
                if (!s_flag[3] && tid == 0) { vjf_status_or(SC + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_SIGMA); *s_dead = 1; }
                lscr_guard = true;
                return;
            }
            // (no acquire: the one thing read behind this wait is sigma, with an sc1 load)
            if (!vjf_wg_wait_sc1(A.wait_count, it_wait_target, tid, SC + VJF_SC_STATUS, (A.flags & VJF_FLAG_HANDOFF_ACQUIRE) != 0u)) { vjf_status_or(SC + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_SIGMA); *s_dead = 1; }
            sig = __hip_atomic_load(S + P.off[VJF_SLOT_TR_LOGVAR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        };
        const __amdgpu_buffer_rsrc_t r_G = vjf_rsrc(G);
        auto g4 = [&](int gi, int gj) {                                 // 4 entries of G, zero outside the matrix
            if (!(gi < n && gj < n)) return make_float4(0.f, 0.f, 0.f, 0.f);
            if (A.stat_count) return vjf_ld4_sc1(r_G, gi * n + gj);       // (another role's stores of this launch: sc1, past this CU's L1)
            return *reinterpret_cast<const float4*>(G + (size_t)gi * n + gj);
        };
        constexpr int NT = VJF_CHOL_THREADS - 64, NQ = ((VJF_CHOL_MAXBLK * (VJF_CHOL_MAXBLK + 1) / 2 - 1) * 256 + NT - 1) / NT;
        const int t2 = tid - 64;
        float4 v[NQ], g[NQ];                                            // (wavefront 0 uses the first four)
        auto idx_of = [&](int q) { return wave == 0 ? (q < 4 ? lane + 64 * q : ntri * 256) : 256 + t2 + q * NT; };
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int idx = idx_of(q);
            v[q] = make_float4(0.f, 0.f, 0.f, 0.f); g[q] = v[q];
            if (idx < ntri * 256) {
                int b, r, c4; chol_tile_of(idx, b, r, c4);
                int gi, gj; tile_at(b, gi, gj); gi += r; gj += c4;
                if (sp && !it_src_state) v[q] = *reinterpret_cast<const float4*>(A.pscr + (size_t)idx * 4);
                else v[q] = (gi < n && gj < n) ? *reinterpret_cast<const float4*>(Pm + (size_t)gi * n + gj) : pad4(gi, gj);
            }
        }
        stat_wait();
        if (sp) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int idx = idx_of(q);
                if (idx < ntri * 256) {
                    int b, r, c4; chol_tile_of(idx, b, r, c4);
                    int gi, gj; tile_at(b, gi, gj);
                    g[q] = g4(gi + r, gj + c4);
                }
            }
        }
        if (sp) {
            sigma_wait();
            const float inv_v = expf(-sig);
            // (the identity padding of the last block is scaled too and decays as lambda^t in pscr within a launch: harmless --
            //  the diagonal chain skips the padded rounds (n % 4 == 0) and writes identity into the factor there, and the
            //  roll-back touches entries inside the matrix only)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                v[q].x = fmaf(g[q].x, inv_v, vjf_lam_mul(v[q].x, lam)); v[q].y = fmaf(g[q].y, inv_v, vjf_lam_mul(v[q].y, lam));
                v[q].z = fmaf(g[q].z, inv_v, vjf_lam_mul(v[q].z, lam)); v[q].w = fmaf(g[q].w, inv_v, vjf_lam_mul(v[q].w, lam));
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int idx = idx_of(q);
            if (idx < ntri * 256) {
                int b, r, c4; chol_tile_of(idx, b, r, c4);
                float* p = s_blk + (size_t)b * VJF_BLK_FLOATS + vsw(r, c4);   // (four dword stores: a row is not 16-byte aligned)
                p[0] = v[q].x; p[1] = v[q].y; p[2] = v[q].z; p[3] = v[q].w;
                if (A.post) *reinterpret_cast<float4*>(A.pscr + (size_t)idx * 4) = v[q];
            }
        }
        if (wave == 0) chain_good = diag_chain(0);
        else if (!A.post)                                               // (post mode: g goes to vjf_rls_post_kernel, not here)
            for (int e = t2; e < npad * DZP; e += NT) {
                const int r = e / DZP, j = e - r * DZP;
                s_g[e] = (r < n && j < dz) ? A.gbuf[(size_t)r * dz + j] : 0.f;
            }
        __syncthreads();
        VJF_STAMP(1);

        // ==== the column loop
        // ---- blocked right-looking Cholesky with look-ahead: while wavefronts 1..7 finish the trailing update of
        //      step k, wavefront 0 updates block (k+1,k+1) first and runs the next diagonal chain
        // post mode: one finished 32x32 block out to global memory (one wavefront, 4 float4 per lane)
        // Write-through (sc1) 16-byte stores: the bytes are in memory, visible to every XCD, once the storing wavefront's vmcnt
        // has drained -- no release fence (cdna guide, Guideline 16 R1); the publishing code below drains them by hand (vjf_st4_wt).
        auto put_block = [&](const float* blk, float* dst, int ld, int gi0, int gj0, bool lower_only) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = lane + 64 * q, r = idx >> 3, c4 = (idx & 7) * 4;
                const float* p = blk + vsw(r, c4);
                vjf_f32x4 o;
                o[0] = (!lower_only || c4 <= r) ? p[0] : 0.f;
                o[1] = (!lower_only || c4 + 1 <= r) ? p[1] : 0.f;
                o[2] = (!lower_only || c4 + 2 <= r) ? p[2] : 0.f;
                o[3] = (!lower_only || c4 + 3 <= r) ? p[3] : 0.f;
                if (gi0 + r < ld && gj0 + c4 < ld) vjf_st4_wt(dst + (size_t)(gi0 + r) * ld + gj0 + c4, o);
            }
        };
        auto publish = [&](int k0, int k1, unsigned fail) {             // one wavefront: its stores drained, then the flags
            vjf_chaos(lane, A.flags_out + k0, 2);                       // (diagnostic builds: the wavefront is held)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane >= k0 && lane < k1) vjf_st_wt(A.flags_out + lane, (it_epoch << 1) | fail);
        };
        // ---- The column loop without a workgroup barrier in it.  The dependent chain -- Dinv_k from the factor chain of block (k,k),
        //      the one panel tile L_{k+1,k} = A_{k+1,k} Dinv_k^T, the last update of block (k+1,k+1), the next chain -- runs on
        //      wavefront 0 alone, back to back (3.4 us a column); it never waits for the bulk of a column's multiply-adds.  Those --
        //      the other panel tiles and the trailing updates of column k -- belong to six helper wavefronts (1-3, 5-7: the three
        //      other SIMDs), which work one column behind it in two stages per column (panels | trailing tiles) separated by a
        //      counter barrier of their own, and which take the two tiles the chain needs next, (k+2,k+1) and (k+2,k+2), first.
        //      Wavefront 4 (the chain's SIMD: no matrix-core work) writes finished columns out.  All hand-offs are words in LDS:
        //        c_chain  = columns whose Dinv is in LDS             (wavefront 0)
        //        c_p1     = columns whose tile L_{k+1,k} is in LDS   (wavefront 0)
        //        c_a, c_b = columns k whose update of tile (k+2,k+1) / (k+2,k+2) is done (helpers)
        //        c_hb[h]  = stages helper h has completed: stage s is complete when every c_hb[h] > s
        //      Every update of a tile is applied in column order by construction (stage barriers), so the bits do not depend on
        //      timing.  Polls are bounded: a logic error shows as a failed factorisation, not as a hang.
        volatile int* s_ctl = s_flag + 4;                              // C_HB + 6 = 10 words
        enum { C_CHAIN = 0, C_P1 = 1, C_A = 2, C_B = 3, C_HB = 4 };
        volatile int* v_ok = s_flag;                                   // [0]: 1 while every pivot was positive (wavefront 0 clears it)
        auto lds_wait = [&](int w, int target) {                       // one wavefront: all lanes poll the same word
            for (unsigned spins = 0; spins < (1u << 22); ++spins) {
                if (s_ctl[w] >= target || !v_ok[0]) break;
                __builtin_amdgcn_s_sleep(1);
            }
            if (s_ctl[w] < target && v_ok[0]) v_ok[0] = 0;             // (cannot happen: ends the step as a failed factorisation)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        };
        auto lds_post = [&](int w, int v) {                            // this wavefront's LDS writes first, then the word
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) s_ctl[w] = v;
        };
        auto hb_arrive = [&](int hw, int stages_done) {                // a helper's stage is done: its own word (no atomic: one writer)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) s_ctl[C_HB + hw] = stages_done;
        };
        auto hb_wait = [&](int stages_done) {                          // every helper has that many stages behind it
            for (unsigned spins = 0; spins < (1u << 22); ++spins) {
                int lo = s_ctl[C_HB];
#pragma unroll
                for (int h2 = 1; h2 < 6; ++h2) lo = min(lo, (int)s_ctl[C_HB + h2]);
                if (lo >= stages_done || !v_ok[0]) break;
                __builtin_amdgcn_s_sleep(1);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        };
        auto panel_tile = [&](int bi, int k) {                         // L_ik = A_ik Dinv_k^T, in place (one wavefront reads all of it first)
            float* pb = s_blk + (size_t)vtri(bi, k) * VJF_BLK_FLOATS;
            vjf_f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            blk_mma<true>(acc, pb, s_aux + (size_t)k * VJF_BLK_FLOATS, lane);
            blk_store(acc, pb, lane);
        };
        auto trail_tile = [&](int bi, int bj, int k) {                 // A_ij -= L_ik L_jk^T
            float* cb = s_blk + (size_t)vtri(bi, bj) * VJF_BLK_FLOATS;
            vjf_f32x16 acc;
            blk_load(acc, cb, lane);
            blk_mma<true, true>(acc, s_blk + (size_t)vtri(bi, k) * VJF_BLK_FLOATS, s_blk + (size_t)vtri(bj, k) * VJF_BLK_FLOATS, lane);
            blk_store(acc, cb, lane);
        };
        int kdone = 0;                                                  // wavefront 4: columns written out (their flags stored)
        if (wave == 0) {
            // Nothing but the chain's own work on this wavefront's path: it is the only one that can fail a pivot, so the verdict
            // stays in a register (v_ok[0] re-read from LDS was a round trip at each of three places per column), and the two words
            // it waits for per column -- both posted by the helpers ~2 us earlier -- are read together, once.
            auto wait_ab = [&](int target) {                            // tiles (k+1,k) and (k+1,k+1) carry the updates of columns < k
                for (unsigned spins = 0; spins < (1u << 22); ++spins) {
                    const int a = s_ctl[C_A], b = s_ctl[C_B];
                    if (a >= target && b >= target) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); return true; }
                    if (!v_ok[0]) return false;
                    __builtin_amdgcn_s_sleep(1);
                }
                v_ok[0] = 0;                                            // (cannot happen: ends the step as a failed factorisation)
                return false;
            };
            bool good = chain_good;
            for (int k = 0; k < nbl && good; ++k) {                     // (chain(0) ran before the barrier above)
                lds_post(C_CHAIN, k + 1);
                if (k + 1 < nbl) {
                    if (k >= 1 && !wait_ab(k)) break;
                    panel_tile(k + 1, k);
                    lds_post(C_P1, k + 1);
                    if (k == 0) VJF_STAMP(8);
                    trail_tile(k + 1, k + 1, k);
                    if (k == 0) VJF_STAMP(4);
                    good = diag_chain(k + 1);
                    if (k == 0) VJF_STAMP(5);
                }
                if (k < 7) VJF_STAMP(9 + k);
            }
        } else if (wave == 4) {
            if (A.post) {
                for (int k = 0; k < nbl; ++k) {
                    // column k of L and Dinv_k out, write-through, as soon as they are final; their flag once the stores have
                    // drained (nobody waits for this wavefront inside the workgroup)
                    lds_wait(C_CHAIN, k + 1);
                    if (k + 1 < nbl) { lds_wait(C_P1, k + 1); hb_wait(2 * k + 1); }
                    if (!v_ok[0]) break;
                    if (k == 0 && lscr_guard) {                         // (this wavefront alone writes the scratch copies)
                        bool there = false;
                        for (unsigned spins = 0; spins < VJF_WAIT_SPINS; ++spins) {      // (its own loop, not vjf_poll_count: as a call it moves code in the pair and one-launch kernels)
                            if ((int)(__hip_atomic_load(A.wait_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - it_wait_target) >= 0) { there = true; break; }
                            if ((spins & 255u) == 255u && vjf_abort_seen(SC + VJF_SC_STATUS)) break;
                            __builtin_amdgcn_s_sleep(1);
                        }
                        if (!there && lane == 0) { vjf_status_or(SC + VJF_SC_STATUS, VJF_STATUS_RLS_FAILED | VJF_STATUS_WAIT_SIGMA); *s_dead = 1; }
                    }
                    for (int it = 0; it < nbl - k; ++it) put_block(s_blk + (size_t)vtri(k + it, k) * VJF_BLK_FLOATS, A.lscr, n, (k + it) * 32, k * 32, it == 0);
                    put_block(s_aux + (size_t)k * VJF_BLK_FLOATS, A.dinv_out + (size_t)k * 1024, 32, 0, 0, false);
                    publish(k, k + 1, 0u);
                    kdone = k + 1;
                }
            }
        } else {
            const int hw = wave < 4 ? wave - 1 : wave - 2;              // helper 0 .. 5
            int stage = 0;
            for (int k = 0; k + 1 < nbl; ++k) {
                lds_wait(C_CHAIN, k + 1);
                if (!v_ok[0]) break;
                for (int bi = k + 2 + hw; bi < nbl; bi += 6) panel_tile(bi, k);
                hb_arrive(hw, ++stage);
                hb_wait(stage);
                if (!v_ok[0]) break;
                // trailing tiles of column k: (k+1+r, k+1+c), 0 <= c <= r < m, without (0,0) (the chain's own)
                const int m = nbl - 1 - k;
                if (m >= 2) {
                    if (hw == 0) { lds_wait(C_P1, k + 1); if (v_ok[0]) { trail_tile(k + 2, k + 1, k); lds_post(C_A, k + 1); } }
                    if (hw == 1) { trail_tile(k + 2, k + 2, k); lds_post(C_B, k + 1); }
                    for (int r = 2; r < m; ++r)                         // the rest of block column k + 1
                        if (r % 6 == hw) { lds_wait(C_P1, k + 1); if (v_ok[0]) trail_tile(k + 1 + r, k + 1, k); }
                    int q = m;
                    for (int r = 2; r < m; ++r)
                        for (int c2 = 1; c2 <= r; ++c2, ++q)
                            if (q % 6 == hw) trail_tile(k + 1 + r, k + 1 + c2, k);
                }
                hb_arrive(hw, ++stage);
                hb_wait(stage);
            }
        }
        __syncthreads();
        const bool ok = s_flag[0] != 0;
        VJF_STAMP(2);
        if (!ok) {                                                      // ==== the roll-back of a failed factorisation
            // Reference: the fallback calls the removed torch.eig and raises (module.py:104-112).  Here:
            // undo P = lambda P + G / v (to rounding: (P' - G / v) / lambda) and leave W, w_chol, w_pchol as they were.
            st |= VJF_STATUS_RLS_FAILED;
            const float inv_v = expf(-sig);
            // (self_prep: the state's P is in the hands of the operand kernel on the post kernel's stream; that kernel's y / W
            //  workgroup, which follows it there, takes the update back)
            if (!sp) for (int e = tid; e < n * n; e += VJF_CHOL_THREADS) Pm[e] = __fdiv_rn(fmaf(-G[e], inv_v, Pm[e]), lam);
            if (A.post) {
                for (int idx = tid; idx < ntri * 256; idx += VJF_CHOL_THREADS) {   // the copy for the next kernel, likewise
                    int b, r, c4; chol_tile_of(idx, b, r, c4);
                    int gi, gj; tile_at(b, gi, gj); gi += r; gj += c4;
                    if (gi < n && gj < n) {
                        float4 pv = *reinterpret_cast<const float4*>(A.pscr + (size_t)idx * 4);
                        const float4 gv = g4(gi, gj);          // (another role's stores on the one-launch route: an sc1 load there, found by tools/audit_plain_loads.py)
                        pv.x = fmaf(-gv.x, inv_v, pv.x); pv.y = fmaf(-gv.y, inv_v, pv.y); pv.z = fmaf(-gv.z, inv_v, pv.z); pv.w = fmaf(-gv.w, inv_v, pv.w);
                        pv.x = __fdiv_rn(pv.x, lam); pv.y = __fdiv_rn(pv.y, lam); pv.z = __fdiv_rn(pv.z, lam); pv.w = __fdiv_rn(pv.w, lam);
                        *reinterpret_cast<float4*>(A.pscr + (size_t)idx * 4) = pv;
                    }
                }
                // columns published so far are those of iterations that completed; every other flag says "failed"
                if (wave == 4) publish(kdone, VJF_CHOL_MAXBLK + 1, 1u);
                if (tid == 0) { A.ok_out[0] = 0; vjf_status_or(SC + VJF_SC_STATUS, st); }
                return;
            }
        } else {
            if (A.post) {
                // L and the inverted diagonal blocks already left column by column; one-time clearing of the zero halves; done
                if (!A.no_triclean && SC[VJF_SC_TRI_CLEAN] == 0.f) {
                    for (int e = tid; e < n * n; e += VJF_CHOL_THREADS) chol_triclean_at(Lm, Wc, n, e);
                    __syncthreads();
                    if (tid == 0) SC[VJF_SC_TRI_CLEAN] = 1.f;
                }
                if (tid == 0) A.ok_out[0] = 1;
                if (wave == 4) publish(VJF_CHOL_MAXBLK, VJF_CHOL_MAXBLK + 1, 0u);   // the factor as a whole is good
                return;
            }
            // ==== the one-workgroup tail (post == 0)
            // ---- w_pchol = L (lower, module.py:99-100)
            {
                float4 v[VJF_CHOL_Q];
#pragma unroll
                for (int q = 0; q < VJF_CHOL_Q; ++q) {
                    const int idx = tid + q * VJF_CHOL_THREADS;
                    if (idx < ntri * 256) {
                        int b, r, c4; chol_tile_of(idx, b, r, c4);
                        const float* p = s_blk + (size_t)b * VJF_BLK_FLOATS + vsw(r, c4);
                        int gi0, gj0; tile_at(b, gi0, gj0);
                        const bool dg = gi0 == gj0;
                        v[q].x = (!dg || c4 <= r) ? p[0] : 0.f;
                        v[q].y = (!dg || c4 + 1 <= r) ? p[1] : 0.f;
                        v[q].z = (!dg || c4 + 2 <= r) ? p[2] : 0.f;
                        v[q].w = (!dg || c4 + 3 <= r) ? p[3] : 0.f;
                    }
                }
#pragma unroll
                for (int q = 0; q < VJF_CHOL_Q; ++q) {
                    const int idx = tid + q * VJF_CHOL_THREADS;
                    if (idx < ntri * 256) {
                        int b, r, c4; chol_tile_of(idx, b, r, c4);
                        int gi, gj; tile_at(b, gi, gj); gi += r; gj += c4;
                        if (gi < n && gj < n) *reinterpret_cast<float4*>(Lm + (size_t)gi * n + gj) = v[q];
                    }
                }
            }
            VJF_STAMP(3);
            VJF_STAMP(4);
            // ---- X = L^-1, block row by block row, in place over L:
            //      X_ij = -Dinv_i * sum_{k=j}^{i-1} L_ik X_kj   (X_jj = Dinv_j)
            for (int bi = 1; bi < nbl; ++bi) {
                vjf_f32x16 xacc;
                const int bj = wave;                                   // bi <= 6 < 8 wavefronts
                if (bj < bi) {
                    vjf_f32x16 t;
#pragma unroll
                    for (int r = 0; r < 16; ++r) t[r] = 0.f;
                    for (int k = bj; k < bi; ++k) {
                        const float* xb = (k == bj) ? s_aux + (size_t)bj * VJF_BLK_FLOATS : s_blk + (size_t)vtri(k, bj) * VJF_BLK_FLOATS;
                        blk_mma<false>(t, s_blk + (size_t)vtri(bi, k) * VJF_BLK_FLOATS, xb, lane);
                    }
                    // X_ij = -Dinv_i * T with T taken straight from the accumulator: register r of T holds
                    // rows vrow(r,0) / vrow(r,1) on the two lane halves = the k pair of MFMA step r.
                    const float* di = s_aux + (size_t)bi * VJF_BLK_FLOATS + vsw(lane & 31, 4 * (lane >> 5));
#pragma unroll
                    for (int r = 0; r < 16; ++r) xacc[r] = 0.f;
                    float da[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) da[r] = -di[vrow(r, 0)];          // Dinv_i[c][vrow(r, h)]
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < 16; ++r) xacc = __builtin_amdgcn_mfma_f32_32x32x2f32(da[r], t[r], xacc, 0, 0, 0);
                }
                __syncthreads();                                       // every reader of row bi of L is done
                if (bj < bi) blk_store(xacc, s_blk + (size_t)vtri(bi, bj) * VJF_BLK_FLOATS, lane);
                __syncthreads();
            }
            VJF_STAMP(5);
            // diagonal blocks of X
            // (element by element: the last float of a block of s_blk is its entry of the tile table)
            for (int e = tid; e < nbl * 1024; e += VJF_CHOL_THREADS) {
                const int o = vsw((e >> 5) & 31, e & 31);
                s_blk[(size_t)vtri(e >> 10, e >> 10) * VJF_BLK_FLOATS + o] = s_aux[(size_t)(e >> 10) * VJF_BLK_FLOATS + o];
            }
            __syncthreads();
            // ---- w_chol = X^T (upper, module.py:102): row (bj*32+c) of w_chol, 4 consecutive r per store
            {
                float4 v[VJF_CHOL_Q];
#pragma unroll
                for (int q = 0; q < VJF_CHOL_Q; ++q) {
                    const int idx = tid + q * VJF_CHOL_THREADS;
                    if (idx < ntri * 256) {
                        int b, c, r4; chol_tile_of(idx, b, c, r4);
                        const float* p = s_blk + (size_t)b * VJF_BLK_FLOATS + vsw(r4, c);
                        int gi0, gj0; tile_at(b, gi0, gj0);
                        const bool dg = gi0 == gj0;
                        v[q].x = (!dg || c <= r4) ? p[0] : 0.f;
                        v[q].y = (!dg || c <= r4 + 1) ? p[VJF_BLK_LD] : 0.f;
                        v[q].z = (!dg || c <= r4 + 2) ? p[2 * VJF_BLK_LD] : 0.f;
                        v[q].w = (!dg || c <= r4 + 3) ? p[3 * VJF_BLK_LD] : 0.f;
                    }
                }
#pragma unroll
                for (int q = 0; q < VJF_CHOL_Q; ++q) {
                    const int idx = tid + q * VJF_CHOL_THREADS;
                    if (idx < ntri * 256) {
                        int b, c, r4; chol_tile_of(idx, b, c, r4);
                        int gi, gj; tile_at(b, gi, gj); gi += r4; gj += c;                // X[gi..gi+3][gj]
                        if (gi < n && gj < n) *reinterpret_cast<float4*>(Wc + (size_t)gj * n + gi) = v[q];
                    }
                }
            }
            if (SC[VJF_SC_TRI_CLEAN] == 0.f) {
                for (int e = tid; e < n * n; e += VJF_CHOL_THREADS) chol_triclean_at(Lm, Wc, n, e);
                __syncthreads();
                if (tid == 0) SC[VJF_SC_TRI_CLEAN] = 1.f;
            }
            VJF_STAMP(6);
            // ---- y = X g ; W = X^T y  (cholesky_solve, module.py:101) as block products on the matrix cores.
            //      Block row br of y sums br+1 products; wavefront w takes the even-offset products of row w and the
            //      odd-offset products of row nbl-1-w (<= ceil((nbl+1)/2) products each), partial tiles meet in LDS.
            {
                float* s_pe = s_aux;                          // even partials, npad x DZP   (s_aux = Dinv is free now)
                // odd partials: behind the even ones in s_aux; DZP = 32: s_aux holds one set only, the region reserved behind g
                float* s_po = DZP <= 16 ? s_aux + (size_t)npad * DZP : s_g + (size_t)npad * DZP;
                const int c = lane & 31, h = lane >> 5;
                auto store_part = [&](const vjf_f32x16& acc, float* dst, int blk) {
                    if (c < DZP) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) dst[(blk * 32 + vrow(r, h)) * DZP + c] = acc[r];
                    }
                };
                for (int pass = 0; pass < 2; ++pass) {                      // pass 0: y = X g ; pass 1: W = X^T y
                    const float* src = s_g;                                 // g, then y
                    for (int par = 0; par < 2; ++par) {
                        const int row = par == 0 ? wave : nbl - 1 - wave;   // block row of the output
                        if (wave < nbl && row >= 0 && row < nbl) {
                            vjf_f32x16 acc;
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                            // pass 0: column blocks cb = row - par, row - par - 2, ... >= 0 of X(row, cb)
                            // pass 1: row blocks    rb = row + par, row + par + 2, ... < nbl of X(rb, row)^T
                            for (int o = par; pass == 0 ? (row - o >= 0) : (row + o < nbl); o += 2) {
                                const int ob = pass == 0 ? row - o : row + o;
                                const float* xb = s_blk + (size_t)(pass == 0 ? vtri(row, ob) : vtri(ob, row)) * VJF_BLK_FLOATS;
                                const float* sb = src + (size_t)ob * 32 * DZP;
                                if (pass == 0)
                                    blk_mma_f<false>(acc, lane, xb, [&](int m, int j) { return j < DZP ? sb[m * DZP + j] : 0.f; });
                                else
                                    blk_mma_f<true>(acc, lane, xb, [&](int m, int j) { return j < DZP ? sb[m * DZP + j] : 0.f; });
                            }
                            store_part(acc, par == 0 ? s_pe : s_po, row);
                        }
                    }
                    __syncthreads();
                    for (int e = tid; e < npad * DZP; e += VJF_CHOL_THREADS) {
                        const float v = s_pe[e] + s_po[e];
                        s_g[e] = v;                                         // y after pass 0, W after pass 1
                        if (pass == 1) {
                            const int rw = e / DZP, j = e - rw * DZP;
                            if (rw < n && j < dz) Wm[(size_t)rw * dz + j] = v;
                        }
                    }
                    __syncthreads();
                }
            }
        }
    }
    if (warm || st) {                                                  // residual needs W in LDS
        for (int e = tid; e < npad * DZP; e += VJF_CHOL_THREADS) {
            const int r = e / DZP, j = e - r * DZP;
            s_g[e] = (r < n && j < dz) ? Wm[(size_t)r * dz + j] : 0.f;
        }
        __syncthreads();
    }
    VJF_STAMP(7);
    // ==== the state-noise tail
    // ---- residual mean square:  sum|dx|^2 - 2 tr(W^T FDX) + tr(W^T G W), fp64 accumulation (model.py:373-374).
    //      thread (i, part) forms half of row i of G W:  G row chunks as float4 (8 in flight), W rows broadcast
    double part_sum = 0.0;
    {
        const int i = tid & 255, part = tid >> 8;
        if (i < n) {
            float acc[DZP];
#pragma unroll
            for (int j = 0; j < DZP; ++j) acc[j] = 0.f;
            const int half = (n / 4 + 1) / 2 * 4;                      // columns [0,half) and [half,n), multiples of 4
            const int c0 = part ? half : 0, c1 = part ? n : half;
            const float* grow = G + (size_t)i * n;
            for (int cb = c0; cb < c1; cb += 32) {
                float4 gv[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) gv[q] = (cb + 4 * q < c1) ? *reinterpret_cast<const float4*>(grow + cb + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int c = cb + 4 * q;
                    if (c < c1) {
                        axpy_row<DZP>(acc, gv[q].x, s_g + c * DZP);
                        axpy_row<DZP>(acc, gv[q].y, s_g + (c + 1) * DZP);
                        axpy_row<DZP>(acc, gv[q].z, s_g + (c + 2) * DZP);
                        axpy_row<DZP>(acc, gv[q].w, s_g + (c + 3) * DZP);
                    }
                }
            }
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < DZP; ++j) q = fmaf(s_g[i * DZP + j], acc[j], q);
            part_sum = (double)q;
            if (part == 0) {
                float f = 0.f;
                for (int j = 0; j < dz; ++j) f = fmaf(s_g[i * DZP + j], FDX[(size_t)i * dz + j], f);
                part_sum -= 2.0 * (double)f;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part_sum += __shfl_xor(part_sum, o, 64);
    if (lane == 0) s_d[wave] = part_sum;
    __syncthreads();
    if (tid == 0) {
        double t = (double)it_red[P.red_SC + RS_SDX2];
        for (int w = 0; w < VJF_CHOL_THREADS / 64; ++w) t += s_d[w];
        float tot;
        S[P.off[VJF_SLOT_TR_LOGVAR]] = vjf_running_logvar(sig, SC[VJF_SC_N_TR], VJF_TR_VAR_CAP, Bf, vjf_resid_mse(t, Bf, dz), tot);
        SC[VJF_SC_N_TR] = tot;
        if (st) vjf_status_or(SC + VJF_SC_STATUS, st);
    }
    VJF_STAMP(8);
}

// One-time clearing of the halves that the post kernel never writes (block-lower part of w_chol, block-upper part of
// w_pchol), for callers that run the Cholesky kernel beside a reader of w_chol (vjf_filter_seq).  grid-stride.
// One pass (nsteps <= 0) or the looping form: nsteps factorisations, one after the other (see VjfCholArgs::nsteps).  The
// per-step values travel as scalars beside the kernel arguments, which stay in scalar registers.
template <int DZP>
__device__ __forceinline__ void vjf_chol_loop(const VjfPlan& P, const VjfCholArgs& A, float* lds, int* s_dead) {
    const int steps = A.nsteps > 0 ? A.nsteps : 1;
    for (int it = 0; it < steps; ++it) {
        const float* red = ((A.step0 + it) & 1) ? A.red2 : A.red;
        vjf_chol_body<DZP>(P, A, lds, s_dead, A.epoch + (unsigned)it, red, A.wait_target + (unsigned)it * A.wait_stride,
                           A.stat_target + (unsigned)it * A.stat_stride, it == 0 && A.src_state != 0);
        __syncthreads();
        if (*s_dead) break;
    }
}

template <int DZP>
__global__ __launch_bounds__(VJF_CHOL_THREADS) void vjf_chol_lds_kernel(VjfPlan P, VjfCholArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_dead;                             // a wait timed out: the looping form stops (status says so)
    if (threadIdx.x == 0) s_dead = 0;
    __syncthreads();
    vjf_chol_loop<DZP>(P, A, lds, &s_dead);
}

__global__ void vjf_triclean_kernel(VjfPlan P, float* state) {
    float* SC = state + P.off[VJF_SLOT_SCALARS];
    if (SC[VJF_SC_TRI_CLEAN] != 0.f) return;
    float* Wc = state + P.off[VJF_SLOT_W_CHOL];
    float* Lm = state + P.off[VJF_SLOT_W_PCHOL];
    const int n = P.n;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n * n; e += gridDim.x * blockDim.x) chol_triclean_at(Lm, Wc, n, e);
}
// (the flag is set by a second, one-thread launch behind it: every workgroup above must have seen it clear)
__global__ void vjf_triclean_done_kernel(VjfPlan P, float* state) { state[P.off[VJF_SLOT_SCALARS] + VJF_SC_TRI_CLEAN] = 1.f; }
