// vjf_smooth_sample_kernel.h -- joint draws from the smoothed posterior of a filtered sequence by backward sampling
// (include/vjf_hip.h: vjf_smooth_sample).  Notation of vjf_smooth_kernel.h: f = x + g the mean map, J = I + A its Jacobian at
// (mu_t, u_{t+1}), sd = exp(lv_t / 2), q the state-noise variance, z standard-normal noise.  Per trial and member s, backwards:
//     Jh = J diag(sd) / sqrt(q),   M = I + Jh^T Jh = L L^T,   G = diag(sd) M^-1 Jh^T / sqrt(q)          (per trial: shared by the members)
//     L^T w = z_t,   x_t = (mu_t + G (x_{t+1} - (mu_t + g))) + sd w                                    (per member)
// so sd w has the conditional covariance diag(sd) M^-1 diag(sd) of the smoother and x_t is affine in x_{t+1}.
//
//   vjf_smooth_sample_kernel   grid (tiles of 16 trials) x (chunks of SC members).  A workgroup walks the whole record backwards for
//                       its tile and its chunk of members; the members' draws (SC x dout x 16) and the noise of the current row are
//                       in LDS.  Per row: flow_evaluate (g and the columns of A), then per trial, sixteen lanes per trial,
//       scale     column j of A -> column j of Jh, in place                                   (a lane owns column j)
//       factor    row j of M from the columns of Jh; L in M's place                           (a lane owns row j; shuffles)
//       gain      column i of G from row i of Jh through the two triangular solves, in place  (a lane owns column i of G)
//       members   lane l of the trial takes members l, l + 16, .. of the chunk, one after the other: the back-substitution
//                 L^T w = z in the noise's place, dl = x_{t+1} - (mu_t + g) in the draw's place, then row by row
//                 x_t[j] = (mu_t[j] + G[j][:] dl) + sd_j w_j in the noise's place; the two buffers then change roles
//     a barrier between the phases.  scale, factor and gain are vjf_smooth_kernel's statements and `factor` is
//     vjf_trial_algebra.h's ta_factor, kept here as copies: with either shared this kernel ran 2 % longer
//     (profiles/trial_algebra_ab.txt); whoever changes one changes both.  The mean sum
//     keeps the smoother's order and the noise term is added last, so zero noise returns the smoother's mean bit for bit.
// Member m of the chunk lies at m * MS + j * 18 + trial with MS = 2 ((9 dout) | 1) floats: in the members phase the sixteen lanes
// of a trial then touch sixteen distinct even banks (mod 32: MS / 2 is odd) and the other trial of the half-wave the odd ones, so
// ds_read_b32 / ds_write_b32 of a member's element have no conflict; L, G, g, mu and sd are one address per trial: a broadcast.
// The rows of step t - 1 (mu, lv, the first of u and VJF_SMS_PF noise values per thread) are loaded into registers at the top of
// step t and go to LDS behind it; noise beyond VJF_SMS_PF x 256 values per chunk and tile is loaded there directly.
// Every per-member sum is serial in a fixed order: a member's bits depend on neither SC, vg, CL, its place in the chunk nor its
// trial's tile-mates.  No trip count depends on data.  A trial whose inputs are not finite at a row, or whose factor has a pivot that
// is not positive and finite, has NaN written over its members' draws by the lanes that own them: they stay NaN down to row 0.
// Workgroups are independent: no cooperative launch, no hand-off, no scratch, no atomics.  Included by vjf_host_smooth_sample.h.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_trial_algebra.h"       // the lane view and helpers (ta_*); vjf_flow_eval.h: flow_evaluate, the x step's FcTile, fc_stage

#define VJF_SMS_MAXDOUT 32           // as VJF_SM_MAXDOUT: two indices per lane, two output tiles of w_mean^T
#define VJF_SMS_LDM 18               // floats between two elements of a member (16 trials and two of padding: see above)
#define VJF_SMS_PF 8                 // noise values of the next row a thread holds in registers while a row computes

namespace {
struct VjfSmsArgs {
    const float* mu; const float* lv;      // (T, B, dout) the filtered means and log-variances
    const float* u;                        // (T, B, du), with `after` (T + 1, B, du), or null
    const float* c; const float* logw;     // centroids (n, d), log widths (n)
    const float* w;                        // w_mean (n, dout)
    const float* z;                        // (S, T, B, dout) standard-normal noise
    const float* after;                    // (S, B, dout) or null: the draws of the row behind the last one
    float* x;                              // (S, T, B, dout)
    int T, S, B, n, d, dout;
    int vg;                                // columns of A per pass
    int sc;                                // members per workgroup
    float rsq;                             // 1 / sqrt(q)
};

// floats of one member in one of the two member buffers
static inline size_t vjf_sms_member_floats(int dout) { return 2 * (size_t)((9 * dout) | 1); }

// the x step's buffers plus 1 / width^2, two vectors (g, sd), the block (A, Jh, G in turn), one triangle (M, L), one pass's partial
// products, the two member buffers (draws and noise) and (cen_lds) w_mean
static inline size_t vjf_sms_lds_floats(int n, int d, int dout, int vg, int sc, bool cen_lds) {
    return vjf_trial_lds_floats(n, d, dout, vg, cen_lds, 2, 1) + 2 * (size_t)sc * vjf_sms_member_floats(dout);
}

// CL: centroids and w_mean in LDS (else read from global memory when they are used);  NO: output tiles of w_mean^T, dout <= 16 NO --
// and so the indices a lane owns in the per-trial linear algebra.
template <bool CL, int NO>
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_smooth_sample_kernel(VjfSmsArgs A) {
    constexpr int TB = 16, LD = VJF_LDT, LM = VJF_SMS_LDM, NW = VJF_FC_WAVES, NTH = VJF_FC_THREADS, PF = VJF_SMS_PF;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FcTile S = fc_tile(smem, A.n, A.d, A.dout, A.B);     // s_phi, s_x ([mu_t, u_{t+1}]), s_part, s_w2: the x step's
    const int n = S.n, d = S.d, dout = S.dout, du = S.du, doutp = S.doutp, ntri = dout * (dout + 1) / 2, T = A.T, B = A.B;
    const int MS = 2 * ((9 * dout) | 1);
    float* s_x = S.s_x;
    float* s_iw2 = S.rest;                        // n            1 / width^2
    float* s_g = s_iw2 + n;                       // dout x LD    g at mu_t
    float* s_sd = s_g + dout * LD;                // dout x LD    exp(lv_t / 2)
    float* s_J = s_sd + dout * LD;                // dout x dout x LD   [j][i][trial]: A[i][j], Jh[i][j], G[j][i] in turn
    float* s_L = s_J + dout * dout * LD;          // ntri x LD    lower triangle of M, then of its factor L, [i (i + 1) / 2 + p][trial]
    float* s_ap = s_L + ntri * LD;                // NW x vg x doutp x LD   the wavefronts' partial products of one pass
    float* xc = s_ap + NW * A.vg * doutp * LD;    // sc x MS      the members' draws of row t + 1, carried: [m][j * LM + trial]
    float* zc = xc + A.sc * MS;                   // sc x MS      the members' noise of row t; the draws of row t behind the members phase
    S.s_c = zc + A.sc * MS;                       // n x d        centroids (CL): behind this kernel's buffers
    float* s_wm = S.s_c + n * d;                  // n x dout     w_mean (CL)
    const int tid = S.tid, b0 = S.b0, nb = S.nb;
    const size_t row0 = (size_t)b0 * dout, rowT = (size_t)B * dout;
    const bool after = A.after != nullptr;
    const int ts = after ? T - 1 : T - 2;         // the first row that is drawn by a step; the row behind it is the carried one
    const int m0 = blockIdx.y * A.sc, mc = min(A.sc, A.S - m0);      // this workgroup's members
    const int ne = nb * dout, tot = mc * ne;      // the live elements of a member's row in this tile; of the chunk's
    const float rsq = A.rsq, qnan = __builtin_nanf("");
    // element e of the chunk's row: member m, element i = trial * dout + j of the tile's rows.  Its offset in (S, T, B, dout)
    // without the row's t * rowT -- in (S, B, dout) with T = 1 -- and its place in a member buffer
    auto place = [&](int e, size_t rows, size_t& go, int& lo) {
        const int m = e / ne, i = e - m * ne, bb = i / dout, j = i - bb * dout;
        go = (size_t)(m0 + m) * rows * rowT + row0 + i;
        lo = m * MS + j * LM + bb;
    };
    // the first PF elements of this thread: what it prefetches and stores in every row
    size_t go[PF];
    int lo[PF];
#pragma unroll
    for (int r = 0; r < PF; ++r) {
        go[r] = 0; lo[r] = 0;
        if (tid + r * NTH < tot) place(tid + r * NTH, T, go[r], lo[r]);
    }

    // ---- stage: widths, centroids, [mu_ts, u_{ts+1}], sd of row ts, the carried draws and the noise of row ts
    {
        const int t0 = max(ts, 0);
        fc_stage<CL, true>(S, A.logw, A.c, s_iw2, A.mu + (size_t)t0 * rowT, nullptr,
                           ts >= 0 && du > 0 ? A.u + (size_t)(t0 + 1) * B * du : nullptr);
        if (CL) for (int i = tid; i < n * dout; i += NTH) s_wm[i] = A.w[i];
        for (int i = tid; i < TB * dout; i += NTH) {
            const int b = i / dout, j = i - b * dout;
            s_sd[j * LD + b] = b < nb ? expf(0.5f * A.lv[(size_t)t0 * rowT + row0 + i]) : 1.f;
        }
        for (int e = tid; e < tot; e += NTH) {
            size_t g; int l;
            place(e, T, g, l);
            const int i = e % ne;
            if (after) {
                size_t ga; int la;
                place(e, 1, ga, la);
                xc[l] = A.after[ga];
                zc[l] = A.z[g + (size_t)(T - 1) * rowT];
            } else {                              // the last row of the record: x = mu + sd z
                const size_t gl = (size_t)(T - 1) * rowT;
                xc[l] = fmaf(expf(0.5f * A.lv[gl + row0 + i]), A.z[g + gl], A.mu[gl + row0 + i]);
                zc[l] = ts >= 0 ? A.z[g + (size_t)ts * rowT] : 0.f;
            }
        }
    }
    FlowEval E;
    E.W = CL ? s_wm : A.w; E.c = A.c; E.s_iw2 = s_iw2; E.s_g = s_g; E.s_A = s_J; E.s_ap = s_ap; E.vg = A.vg;
    __syncthreads();

    // the trial of this lane and its indices
    const int b = ta_trial(S), l16 = ta_l16(S);
    // ta_factor's statements (vjf_trial_algebra.h): the lower triangle at s_T becomes its Cholesky factor, a row per lane, column by column
    auto factor = [&](float* s_T) {
        bool ok = true;
        for (int j = 0; j < dout; ++j) {
            const int own = j & 15, ej = j >> 4;
            const int rj = min(l16 + 16 * ej, dout - 1);              // the row of this lane that lane `own` has as row j
            float a[2] = {0.f, 0.f};
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int i = l16 + 16 * e;
                a[e] = (i >= j && i < dout) ? s_T[ta_tri(i, j) * LD + b] : 0.f;
            }
            for (int p = 0; p < j; ++p) {
                const float ljp = __shfl(s_T[ta_tri(rj, min(p, rj)) * LD + b], own, 16);
#pragma unroll
                for (int e = 0; e < NO; ++e) {
                    const int i = l16 + 16 * e;
                    if (i >= j && i < dout) a[e] = fmaf(-s_T[ta_tri(i, p) * LD + b], ljp, a[e]);
                }
            }
            const float piv = __shfl(ej ? a[1] : a[0], own, 16);
            ok = ok && piv > 0.f && piv < INFINITY;
            const float dj = sqrtf(piv);
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int i = l16 + 16 * e;
                if (i >= j && i < dout) s_T[ta_tri(i, j) * LD + b] = i == j ? dj : a[e] / dj;
            }
        }
        return ok;
    };
    // this tile's rows of row t of the chunk's members from the buffer `s`.  All threads; no barrier.
    auto emit = [&](int t, const float* s) {
        const size_t gt = (size_t)t * rowT;
#pragma unroll
        for (int r = 0; r < PF; ++r)
            if (tid + r * NTH < tot) A.x[go[r] + gt] = s[lo[r]];
        for (int e = tid + PF * NTH; e < tot; e += NTH) {
            size_t g; int l;
            place(e, T, g, l);
            A.x[g + gt] = s[l];
        }
    };

    // ---- the last row of the record: a mean that is not finite or a deviation that is not positive and finite poisons the trial
    bool bad = false;
    if (!after) {
        float nf = 0.f;
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int j = l16 + 16 * e;
            if (j < dout && b < nb) {
                const size_t gl = (size_t)(T - 1) * rowT + row0 + (size_t)b * dout + j;
                const float sd = expf(0.5f * A.lv[gl]);
                nf += ta_isfin(A.mu[gl]) && sd > 0.f && sd < INFINITY ? 0.f : 1.f;
            }
        }
        const float nfs = ta_sum16(nf);
        bad = nfs > 0.f;
        if (bad)
            for (int m = l16; m < mc; m += 16)
                for (int j = 0; j < dout; ++j) xc[m * MS + j * LM + b] = qnan;
    }
    __syncthreads();
    if (!after) emit(T - 1, xc);

    for (int t = ts; t >= 0; --t) {
        // the rows of step t - 1, in flight while this step computes: mu and lv (at most two elements per thread), the first of u,
        // PF values of the chunk's noise
        float pm[2] = {0.f, 0.f}, pl[2] = {0.f, 0.f}, pz[PF];
        const float* un = t > 0 && du > 0 ? A.u + ((size_t)t * B + b0) * du : nullptr;
#pragma unroll
        for (int r = 0; r < PF; ++r) pz[r] = 0.f;
        if (t > 0) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int i = tid + r * NTH;
                if (i < nb * dout) { pm[r] = A.mu[(size_t)(t - 1) * rowT + row0 + i]; pl[r] = A.lv[(size_t)(t - 1) * rowT + row0 + i]; }
            }
#pragma unroll
            for (int r = 0; r < PF; ++r)
                if (tid + r * NTH < tot) pz[r] = A.z[go[r] + (size_t)(t - 1) * rowT];
        }
        const float u0 = fc_u_ahead(S, un);

        flow_evaluate<CL, NO>(S, E);              // g, A at [mu_t, u_{t+1}]

        // scale: Jh[i][j] = (delta_ij + A[i][j]) sd_j / sqrt(q) in place, and whether this row's inputs are finite
        {
            float nf = 0.f;
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int j = l16 + 16 * e;
                if (j < dout) {
                    const float sd = s_sd[j * LD + b], sc = sd * rsq, xj = s_x[j * LD + b];
                    float* aj = s_J + (size_t)j * dout * LD + b;
                    for (int i = 0; i < dout; ++i) aj[i * LD] = (aj[i * LD] + (i == j ? 1.f : 0.f)) * sc;
                    nf += ta_isfin(xj) && sd > 0.f && sd < INFINITY ? 0.f : 1.f;
                }
            }
            for (int j = dout + l16; j < d; j += 16) nf += ta_isfin(s_x[j * LD + b]) ? 0.f : 1.f;
            const float nfs = ta_sum16(nf);          // (every lane of the wavefront takes part)
            bad = bad || nfs > 0.f;
        }
        __syncthreads();

        // factor: M = I + Jh^T Jh (row j: the products of column j with the columns before it), L in its place
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int j = l16 + 16 * e;
            if (j < dout) {
                const float* aj = s_J + (size_t)j * dout * LD + b;
                for (int p = 0; p <= j; ++p) {
                    const float* ap = s_J + (size_t)p * dout * LD + b;
                    float m = p == j ? 1.f : 0.f;
                    for (int i = 0; i < dout; ++i) m = fmaf(aj[i * LD], ap[i * LD], m);
                    s_L[ta_tri(j, p) * LD + b] = m;
                }
            }
        }
        const bool okL = factor(s_L);
        bad = bad || !okL;
        __syncthreads();

        // gain: column i of G from row i of Jh, through the two triangular solves, in place
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i < dout) {
                float* yi = s_J + (size_t)i * LD + b;             // element j at yi[j * dout * LD]
                for (int j = 0; j < dout; ++j) {
                    float s = yi[(size_t)j * dout * LD];
                    for (int p = 0; p < j; ++p) s = fmaf(-s_L[ta_tri(j, p) * LD + b], yi[(size_t)p * dout * LD], s);
                    yi[(size_t)j * dout * LD] = s / s_L[ta_tri(j, j) * LD + b];
                }
                for (int j = dout - 1; j >= 0; --j) {
                    float s = yi[(size_t)j * dout * LD];
                    for (int p = j + 1; p < dout; ++p) s = fmaf(-s_L[ta_tri(p, j) * LD + b], yi[(size_t)p * dout * LD], s);
                    yi[(size_t)j * dout * LD] = s / s_L[ta_tri(j, j) * LD + b];
                }
                for (int j = 0; j < dout; ++j) yi[(size_t)j * dout * LD] *= s_sd[j * LD + b] * rsq;
            }
        }
        __syncthreads();

        // members: a lane takes members l16, l16 + 16, .. of its trial, each serially
        if (b < nb)
            for (int m = l16; m < mc; m += 16) {
                float* xm = xc + m * MS + b;
                float* zm = zc + m * MS + b;
                for (int j = dout - 1; j >= 0; --j) {             // L^T w = z
                    float s = zm[j * LM];
                    for (int p = j + 1; p < dout; ++p) s = fmaf(-s_L[ta_tri(p, j) * LD + b], zm[p * LM], s);
                    zm[j * LM] = s / s_L[ta_tri(j, j) * LD + b];
                }
                for (int i = 0; i < dout; ++i) xm[i * LM] = xm[i * LM] - (s_x[i * LD + b] + s_g[i * LD + b]);
                for (int j = 0; j < dout; ++j) {                  // the smoother's mean sum, then the noise term
                    const float* gj = s_J + (size_t)j * dout * LD + b;
                    float mm = 0.f;
                    for (int i = 0; i < dout; ++i) mm = fmaf(gj[i * LD], xm[i * LM], mm);
                    zm[j * LM] = bad ? qnan : fmaf(s_sd[j * LD + b], zm[j * LM], s_x[j * LD + b] + mm);
                }
            }
        __syncthreads();

        { float* sw = xc; xc = zc; zc = sw; }     // the draws of row t are the carried ones; the other buffer takes the next noise
        emit(t, xc);
        // the rows of step t - 1 into LDS
        if (t > 0) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int i = tid + r * NTH;
                if (i < nb * dout) {
                    const int bb = i / dout, j = i - bb * dout;
                    s_x[j * LD + bb] = pm[r];
                    s_sd[j * LD + bb] = expf(0.5f * pl[r]);
                }
            }
            fc_u_advance(S, un, u0);
#pragma unroll
            for (int r = 0; r < PF; ++r)
                if (tid + r * NTH < tot) zc[lo[r]] = pz[r];
            for (int e = tid + PF * NTH; e < tot; e += NTH) {
                size_t g; int l;
                place(e, T, g, l);
                zc[l] = A.z[g + (size_t)(t - 1) * rowT];
            }
        }
        __syncthreads();
    }
}
}  // namespace
