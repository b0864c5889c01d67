// vjf_smooth_kernel.h -- the extended Rauch-Tung-Striebel pass over a filtered sequence (include/vjf_hip.h: vjf_smooth), in its
// information form scaled by D^(1/2):  per trial, backwards over the rows, with f = x + g the mean map of RBFDS.forward(sampling=False),
// J = I + A its Jacobian at (mu_t, u_{t+1}), sd = exp(lv_t / 2), D = diag(sd^2) and q the state-noise variance,
//     Jh = J diag(sd) / sqrt(q),   M = I + Jh^T Jh = L L^T,   G = diag(sd) M^-1 Jh^T / sqrt(q),   C = diag(sd) M^-1 diag(sd),
//     ms_t = mu_t + G (ms_{t+1} - (mu_t + g)),   Ps_t = C + (G Ls)(G Ls)^T,   Ls Ls^T = Ps_{t+1}.
//
//   vjf_smooth_kernel   one workgroup per tile of 16 trials walks the whole horizon inside the kernel; ms and the lower triangle of Ps
//                       stay in LDS.  Per row: the features of [mu_t, u_{t+1}], g and the columns of A (flow_evaluate: MFMA products
//                       that share w_mean^T), then per trial, four trials per wavefront and sixteen lanes per trial, a lane owning
//                       indices l and l + 16:
//       scale     column j of A -> column j of Jh, in place; dl = ms_{t+1} - (mu_t + g)                      (a lane owns column j)
//       factor    row j of M from the columns of Jh; L in M's place; Ls in Ps's place                        (a lane owns row j; shuffles)
//       gain      for row i of Jh: L y = Jh[i][:]^T, L^T z = y, column i of G = sd z / sqrt(q), in Jh's place   (a lane owns column i of G)
//       mean, K   ms_t[j] = mu_t[j] + G[j][:] dl;  K[j][c] = sum_{i >= c} G[j][i] Ls[i][c] for c ascending, in G's place  (row j of G)
//       cov       column i of the triangle: L y = e_i, L^T z = y on rows i .., Ps_t[j][i] = sd_j sd_i z_j + K[j][:] K[i][:]   (column i)
//     a barrier between the phases.  So one dout x dout block and two triangles are all there is beside the vectors.
// The rows of step t - 1 (mu, lv, u) are loaded from global memory into registers at the top of step t and go to LDS behind it.
// Every sum is serial in a fixed order, a trial is one MFMA column, and every decision is a select on per-trial values; no trip count
// depends on data.  A trial whose inputs are not finite, or whose factor has a pivot that is not positive and finite, has NaN written
// over its carried moments: they stay NaN down to row 0, and no other trial sees them.
// Workgroups are independent: no cooperative launch, no hand-off, no scratch, no atomics.  Included by vjf_host_smooth.h.
// The factorisation, the staging of the carried triangle and the rows written out are vjf_trial_algebra.h's, shared with
// vjf_ekf_kernel.h.  vjf_smooth_sample_kernel.h has its own copy of the factorisation and of the scale, factor and gain phases,
// statement for statement: with either shared its kernel ran 2 % longer (profiles/trial_algebra_ab.txt).  Whoever changes one changes both.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_trial_algebra.h"       // the lane view and helpers (ta_*); vjf_flow_eval.h: flow_evaluate, the x step's FcTile, fc_stage

#define VJF_SM_MAXDOUT 32            // dout <= 32: two indices per lane in the per-trial linear algebra, two output tiles of w_mean^T

namespace {
struct VjfSmArgs {
    const float* mu; const float* lv;      // (T, B, dout) the filtered means and log-variances
    const float* u;                        // (T, B, du), with `after` (T + 1, B, du), or null
    const float* c; const float* logw;     // centroids (n, d), log widths (n)
    const float* w;                        // w_mean (n, dout)
    const float* after_mean;               // (B, dout) or null: the smoothed moments of the row behind the last one
    const float* after_cov;                // (B, dout, dout), its lower triangle is read
    float* mean; float* var;               // (T, B, dout)
    float* cov;                            // (T, B, dout, dout) or null
    float* cov0;                           // (B, dout, dout)
    int T, B, n, d, dout;
    int vg;                                // columns of A per pass
    float rsq;                             // 1 / sqrt(q)
};

// the x step's buffers plus 1 / width^2, four vectors (g, ms, sd, dl), the block (A, Jh, G, K in turn), the two triangles (M and L; Ps
// and Ls), one pass's partial products and (cen_lds) w_mean
static inline size_t vjf_smooth_lds_floats(int n, int d, int dout, int vg, bool cen_lds) {
    return vjf_trial_lds_floats(n, d, dout, vg, cen_lds, 4, 2);
}

// CL: centroids and w_mean in LDS (else read from global memory when they are used);  NO: output tiles of w_mean^T, dout <= 16 NO --
// and so the indices a lane owns in the per-trial linear algebra.
template <bool CL, int NO>
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_smooth_kernel(VjfSmArgs A) {
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_FC_WAVES, NTH = VJF_FC_THREADS;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FcTile S = fc_tile(smem, A.n, A.d, A.dout, A.B);     // s_phi, s_x ([mu_t, u_{t+1}]), s_part, s_w2: the x step's
    const int n = S.n, d = S.d, dout = S.dout, du = S.du, doutp = S.doutp, ntri = dout * (dout + 1) / 2, T = A.T, B = A.B;
    float* s_x = S.s_x;
    float* s_iw2 = S.rest;                        // n            1 / width^2
    float* s_g = s_iw2 + n;                       // dout x LD    g at mu_t
    float* s_ms = s_g + dout * LD;                // dout x LD    the smoothed mean, carried
    float* s_sd = s_ms + dout * LD;               // dout x LD    exp(lv_t / 2)
    float* s_dl = s_sd + dout * LD;               // dout x LD    ms_{t+1} - (mu_t + g)
    float* s_J = s_dl + dout * LD;                // dout x dout x LD   [j][i][trial]: A[i][j], Jh[i][j], G[j][i], K[j][i] in turn
    float* s_L = s_J + dout * dout * LD;          // ntri x LD    lower triangle of M, then of its factor L, [i (i + 1) / 2 + p][trial]
    float* s_P = s_L + ntri * LD;                 // ntri x LD    lower triangle of Ps, carried; of its factor Ls between `factor` and `cov`
    float* s_ap = s_P + ntri * LD;                // NW x vg x doutp x LD   the wavefronts' partial products of one pass
    S.s_c = s_ap + NW * A.vg * doutp * LD;        // n x d        centroids (CL): behind this kernel's buffers
    float* s_wm = S.s_c + n * d;                  // n x dout     w_mean (CL)
    const int tid = S.tid, b0 = S.b0, nb = S.nb;
    const size_t row0 = (size_t)b0 * dout, rowT = (size_t)B * dout;
    const bool after = A.after_mean != nullptr;
    const int ts = after ? T - 1 : T - 2;         // the first row that is smoothed by a step; the row behind it is the carried one
    const float rsq = A.rsq, qnan = __builtin_nanf("");

    // ---- stage: widths, centroids, [mu_ts, u_{ts+1}], sd of row ts, and the carried moments
    {
        const int t0 = max(ts, 0);
        fc_stage<CL, true>(S, A.logw, A.c, s_iw2, A.mu + (size_t)t0 * rowT, nullptr,
                           ts >= 0 && du > 0 ? A.u + (size_t)(t0 + 1) * B * du : nullptr);
        if (CL) for (int i = tid; i < n * dout; i += NTH) s_wm[i] = A.w[i];
        for (int i = tid; i < TB * dout; i += NTH) {
            const int b = i / dout, j = i - b * dout;
            const bool live = b < nb;
            s_sd[j * LD + b] = live ? expf(0.5f * A.lv[(size_t)t0 * rowT + row0 + i]) : 1.f;
            s_ms[j * LD + b] = live ? (after ? A.after_mean[row0 + i] : A.mu[(size_t)(T - 1) * rowT + row0 + i]) : 0.f;
        }
        ta_stage_triangle(S, s_P, after ? A.after_cov : nullptr, A.lv + (size_t)(T - 1) * rowT);
    }
    FlowEval E;
    E.W = CL ? s_wm : A.w; E.c = A.c; E.s_iw2 = s_iw2; E.s_g = s_g; E.s_A = s_J; E.s_ap = s_ap; E.vg = A.vg;
    __syncthreads();

    // the trial of this lane and its indices
    const int b = ta_trial(S), l16 = ta_l16(S);
    // this tile's rows of mean, var and (if asked for) cov of row t from the carried moments; cov0 at row 0.  All threads; no barrier.
    auto emit = [&](int t) { ta_emit_moments(S, s_ms, s_P, t, rowT, A.mean, A.var, A.cov, t == 0, A.cov0); };

    // ---- the carried row: a moment that is not finite, or (the last row of the record) a variance that is not positive, poisons the trial
    bool bad;
    {
        float nf = 0.f;
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int j = l16 + 16 * e;
            if (j < dout) {
                const float pj = s_P[ta_tri(j, j) * LD + b];
                nf += ta_isfin(s_ms[j * LD + b]) && (after || (pj > 0.f && pj < INFINITY)) ? 0.f : 1.f;
            }
        }
        const float nfs = ta_sum16(nf);
        bad = nfs > 0.f;
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int j = l16 + 16 * e;
            if (j < dout && bad) {
                s_ms[j * LD + b] = qnan;
                for (int p = 0; p <= j; ++p) s_P[ta_tri(j, p) * LD + b] = qnan;
            }
        }
    }
    __syncthreads();
    if (!after) emit(T - 1);

    for (int t = ts; t >= 0; --t) {
        // the rows of step t - 1, in flight while this step computes: mu and lv (at most two elements per thread), the first of u
        float pm[2] = {0.f, 0.f}, pl[2] = {0.f, 0.f};
        const float* un = t > 0 && du > 0 ? A.u + ((size_t)t * B + b0) * du : nullptr;
        if (t > 0) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int i = tid + r * NTH;
                if (i < nb * dout) { pm[r] = A.mu[(size_t)(t - 1) * rowT + row0 + i]; pl[r] = A.lv[(size_t)(t - 1) * rowT + row0 + i]; }
            }
        }
        const float u0 = fc_u_ahead(S, un);

        flow_evaluate<CL, NO>(S, E);              // g, A at [mu_t, u_{t+1}]

        // scale: Jh[i][j] = (delta_ij + A[i][j]) sd_j / sqrt(q) in place, dl, and whether this row's inputs are finite
        {
            float nf = 0.f;
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int j = l16 + 16 * e;
                if (j < dout) {
                    const float sd = s_sd[j * LD + b], sc = sd * rsq, xj = s_x[j * LD + b];
                    float* aj = s_J + (size_t)j * dout * LD + b;
                    for (int i = 0; i < dout; ++i) aj[i * LD] = (aj[i * LD] + (i == j ? 1.f : 0.f)) * sc;
                    s_dl[j * LD + b] = s_ms[j * LD + b] - (xj + s_g[j * LD + b]);
                    nf += ta_isfin(xj) && sd > 0.f && sd < INFINITY ? 0.f : 1.f;
                }
            }
            for (int j = dout + l16; j < d; j += 16) nf += ta_isfin(s_x[j * LD + b]) ? 0.f : 1.f;
            const float nfs = ta_sum16(nf);          // (every lane of the wavefront takes part)
            bad = bad || nfs > 0.f;
        }
        __syncthreads();

        // factor: M = I + Jh^T Jh (row j: the products of column j with the columns before it), L in its place; Ls in Ps's place
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
        const bool okL = ta_factor<NO>(b, l16, dout, s_L);
        const bool okP = ta_factor<NO>(b, l16, dout, s_P);
        bad = bad || !okL || !okP;
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

        // mean and K = G Ls: row j of G; K[j][c] needs G[j][i] for i >= c only, so it takes G's place for c ascending
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int j = l16 + 16 * e;
            if (j < dout) {
                float* gj = s_J + (size_t)j * dout * LD + b;
                float m = 0.f;
                for (int i = 0; i < dout; ++i) m = fmaf(gj[i * LD], s_dl[i * LD + b], m);
                s_ms[j * LD + b] = bad ? qnan : s_x[j * LD + b] + m;
                for (int c = 0; c < dout; ++c) {
                    float k = 0.f;
                    for (int i = c; i < dout; ++i) k = fmaf(gj[i * LD], s_P[ta_tri(i, c) * LD + b], k);
                    gj[c * LD] = k;
                }
            }
        }
        __syncthreads();

        // cov: column i of the new triangle in Ps's place -- M^-1 e_i on rows i .. through the two solves, then C + K K^T
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i < dout) {
                for (int j = i; j < dout; ++j) {
                    float s = j == i ? 1.f : 0.f;
                    for (int p = i; p < j; ++p) s = fmaf(-s_L[ta_tri(j, p) * LD + b], s_P[ta_tri(p, i) * LD + b], s);
                    s_P[ta_tri(j, i) * LD + b] = s / s_L[ta_tri(j, j) * LD + b];
                }
                for (int j = dout - 1; j >= i; --j) {
                    float s = s_P[ta_tri(j, i) * LD + b];
                    for (int p = j + 1; p < dout; ++p) s = fmaf(-s_L[ta_tri(p, j) * LD + b], s_P[ta_tri(p, i) * LD + b], s);
                    s_P[ta_tri(j, i) * LD + b] = s / s_L[ta_tri(j, j) * LD + b];
                }
                const float* ki = s_J + (size_t)i * dout * LD + b;
                const float sdi = s_sd[i * LD + b];
                for (int j = i; j < dout; ++j) {
                    const float* kj = s_J + (size_t)j * dout * LD + b;
                    float kk = 0.f;
                    for (int c = 0; c < dout; ++c) kk = fmaf(kj[c * LD], ki[c * LD], kk);
                    s_P[ta_tri(j, i) * LD + b] = bad ? qnan : fmaf(s_sd[j * LD + b] * sdi, s_P[ta_tri(j, i) * LD + b], kk);
                }
            }
        }
        __syncthreads();

        emit(t);
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
        }
        __syncthreads();
    }
}
}  // namespace
