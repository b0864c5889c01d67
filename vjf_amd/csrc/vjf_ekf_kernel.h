// vjf_ekf_kernel.h -- the extended Kalman filter of the learned generative model over a record (include/vjf_hip.h: vjf_ekf), forwards:
// per trial, with f = x + g the mean map of RBFDS.forward(sampling=False), J = I + A its Jacobian at (m, u_t), q the state-noise
// variance, y = C x + b the decoder, r the observation variance and Gc = C^T C / r,
//     predict   m^- = m + g,   Ls Ls^T = P,   K = J Ls,   P^- = K K^T + q I = Lp Lp^T
//     update    M = I + Lp^T Gc Lp = Lm Lm^T,   Lm Y = Lp^T,   P = Y^T Y,   s = C^T (y - b - C m^-) / r,   m = m^- + P s
//     evidence  ll = -1/2 (dy log 2 pi + dy log r + 2 sum log diag(Lm) + |y - b - C m|^2 / r + |Lp^-1 (m - m^-)|^2)
// No dy x dy matrix, no difference of covariances: P^- and P are Gram matrices and M is bounded below by I.
//
//   vjf_ekf_kernel   one workgroup per tile of 16 trials walks the whole record inside the kernel; m (in the x step's s_x) and the lower
//                    triangle of P stay in LDS.  Per row: the features of [m, u_t], g and the columns of A (flow_evaluate: MFMA
//                    products that share w_mean^T), then per trial, four trials per wavefront and sixteen lanes per trial, a lane
//                    owning indices l and l + 16:
//       factor    Ls in P's place; m^-                                                               (a lane owns row i; shuffles)
//       K         K[i][c] = sum_{k >= c} J[i][k] Ls[k][c] for c ascending, in A's place                (row i of J)
//       predict   row i of P^- from the rows of K; Lp in its place
//       W         column p of Gc Lp, in K's place -- zero for a trial whose row is not observed          (column p)
//       M         row i of I + Lp^T W; Lm in its place
//       Y         column c of Lm^-1 Lp^T by the forward solve, in W's place                             (column c)
//       cov       row i of Y^T Y, in Ls's place
//     then the two decodes as MFMA products with the shared operand C, the trial on the MFMA column, dy walked in rounds of
//     four tiles of 16 rows (one per wavefront):  v = y - b - C m^- of a tile goes through 16 x VJF_LDT floats of LDS into
//     C^T v (accumulated over the wavefront's tiles; the four wavefronts' sums added in a fixed order), m = m^- + P s, and
//     |y - b - C m|^2 summed per lane over its tiles and then over the sixteen partials of a trial in a fixed order.
//     A barrier between the phases.  One dout x dout block and three triangles are all there is beside the vectors.
// A row that is not observed: W = 0 makes M = I, Lm = I and Y = Lp^T exactly, so P = Lp Lp^T = P^-; v = 0 makes s = 0; m = m^- and
// ll = 0 are selects.  Its y is loaded and never enters arithmetic.
// The first round of the next row's y, its `observed` flags and its u are loaded into registers at the top of a row and go to LDS
// behind it.  Every sum is serial in a fixed order, a trial is one MFMA column, and every decision is a select on per-trial values; no
// trip count depends on data.  A trial with a non-finite m, u or observed y, or a pivot that is not positive and finite, has NaN written
// over its carried moments and its log-likelihood: they stay NaN to the last row, and no other trial sees them.
// Workgroups are independent: no cooperative launch, no hand-off, no scratch, no atomics.  Included by vjf_host_ekf.h.
// The factorisation, the staging of the prior's triangle and the rows written out are vjf_trial_algebra.h's, shared with vjf_smooth_kernel.h.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_trial_algebra.h"       // the lane view and helpers (ta_*); vjf_flow_eval.h: flow_evaluate, the x step's FcTile, fc_stage

#define VJF_EKF_MAXDOUT 32           // dout <= 32: two indices per lane in the per-trial linear algebra, two output tiles of w_mean^T

namespace {
struct VjfEkfArgs {
    const float* y;                        // (T, B, dy)
    const float* u;                        // (T, B, du) or null: u[t] drives the step into row t
    const unsigned char* obs;              // (T, B) or null: every row observed
    const float* c; const float* logw;     // centroids (n, d), log widths (n)
    const float* w;                        // w_mean (n, dout)
    const float* dec_W; const float* dec_b;   // (dy, dout), (dy)
    const float* prior_mean;               // (B, dout)
    const float* prior_lv;                 // (B, dout) or null
    const float* prior_cov;                // (B, dout, dout) or null: its lower triangle is read
    float* mean; float* var;               // (T, B, dout)
    float* cov;                            // (T, B, dout, dout) or null
    float* ll;                             // (T, B)
    float* cov_last;                       // (B, dout, dout)
    int T, B, n, d, dout, dy;
    int vg;                                // columns of A per pass
    float q, r;
};

// rows of the decoder's two LDS copies: k-major (the decode reads 16 consecutive y rows of one k; two k are 16 banks apart) and
// j-major (C^T v reads 16 consecutive k of one y row; two rows are 16 banks apart)
__host__ __device__ static inline size_t vjf_ekf_ldc(int dy) { return ((size_t)dy + 31) / 32 * 32 + 16; }
__host__ __device__ static inline size_t vjf_ekf_ldt(int dout) { return dout <= 16 ? 16 : 48; }
// the x step's buffers plus 1 / width^2, three vectors (g then m - m^-; m^-; s), the block (A, K, W, Y in turn), the three triangles
// (P and Ls; P^- and Lp; M and Lm), one pass's partial products (v of a round lies there too), Gc, the sixteen partial sums of
// |y - b - C m|^2, the observed flags and (dec_lds) the decoder twice, (cen_lds) w_mean
static inline size_t vjf_ekf_lds_floats(int n, int d, int dout, int dy, int vg, bool cen_lds, bool dec_lds) {
    const size_t dyp = ((size_t)dy + 15) / 16 * 16, LD = VJF_LDT;
    return vjf_trial_lds_floats(n, d, dout, vg, cen_lds, 3, 3) + (size_t)dout * dout + 16 * LD + LD +
           (dec_lds ? (size_t)dout * vjf_ekf_ldc(dy) + dyp * vjf_ekf_ldt(dout) : 0);
}

// CL: centroids and w_mean in LDS (else read from global memory when they are used);  NO: output tiles of w_mean^T, dout <= 16 NO --
// and so the indices a lane owns in the per-trial linear algebra;  DL: the decoder in LDS, else read from global memory (L2) as torch
// stores it.  All forms issue the same operations on the same operands in the same order.
template <bool CL, int NO, bool DL>
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_ekf_kernel(VjfEkfArgs A) {
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_FC_WAVES, NTH = VJF_FC_THREADS;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FcTile S = fc_tile(smem, A.n, A.d, A.dout, A.B);     // s_phi, s_x ([m, u_t]), s_part, s_w2: the x step's
    const int n = S.n, d = S.d, dout = S.dout, du = S.du, doutp = S.doutp, ntri = dout * (dout + 1) / 2, T = A.T, B = A.B, dy = A.dy;
    const int dyp = (dy + 15) / 16 * 16, ntile = dyp / 16, ldc = (int)vjf_ekf_ldc(dy), ldt = (int)vjf_ekf_ldt(dout);
    float* s_x = S.s_x;
    float* s_iw2 = S.rest;                        // n            1 / width^2
    float* s_g = s_iw2 + n;                       // dout x LD    g at m; m - m^- and Lp^-1 (m - m^-) behind the update
    float* s_mp = s_g + dout * LD;                // dout x LD    m^-
    float* s_sv = s_mp + dout * LD;               // dout x LD    s = C^T v / r
    float* s_J = s_sv + dout * LD;                // dout x dout x LD   A[i][j] at [j][i]; K[i][c] at [c][i]; W[a][p] at [a][p]; Y[k][c] at [k][c]
    float* s_P = s_J + dout * dout * LD;          // ntri x LD    lower triangle of P, carried; of its factor Ls between `factor` and `cov`
    float* s_Pp = s_P + ntri * LD;                // ntri x LD    lower triangle of P^-, then of its factor Lp
    float* s_M = s_Pp + ntri * LD;                // ntri x LD    lower triangle of M, then of its factor Lm
    float* s_ap = s_M + ntri * LD;                // NW x vg x doutp x LD   the wavefronts' partial products of one pass; v of a round
    float* s_G = s_ap + NW * A.vg * doutp * LD;   // dout x dout  Gc = C^T C / r
    float* s_q = s_G + dout * dout;               // 16 x LD      partial sums of |y - b - C m|^2
    float* s_obs = s_q + 16 * LD;                 // LD           1 where this row of the trial is observed
    float* s_dec = s_obs + LD;                    // dout x ldc   the decoder, k-major (DL)
    float* s_dect = s_dec + (DL ? dout * ldc : 0);   // dyp x ldt the decoder, j-major (DL)
    S.s_c = s_dect + (DL ? dyp * ldt : 0);        // n x d        centroids (CL): behind this kernel's buffers
    float* s_wm = S.s_c + n * d;                  // n x dout     w_mean (CL)
    float* s_v = s_ap;
    const int tid = S.tid, wave = S.wave, b0 = S.b0, nb = S.nb, mi = S.mi, kk = S.kk, r4 = S.r4;
    const size_t rowT = (size_t)B * dout;
    const float q = A.q, r = A.r, qnan = __builtin_nanf("");
    const float lconst = (float)dy * (1.8378770664093453f + logf(r));

    // ---- stage: widths, centroids, [prior mean, u_0], the prior's triangle, the flags of row 0, the decoder and Gc
    fc_stage<CL, true>(S, A.logw, A.c, s_iw2, A.prior_mean, nullptr, du > 0 ? A.u : nullptr);
    if (CL) for (int i = tid; i < n * dout; i += NTH) s_wm[i] = A.w[i];
    ta_stage_triangle(S, s_P, A.prior_cov, A.prior_lv);
    if (tid < TB) s_obs[tid] = tid < nb && (!A.obs || A.obs[b0 + tid]) ? 1.f : 0.f;
    if (DL)
        for (int e = tid; e < dyp * dout; e += NTH) {
            const int j = e / dout, k = e - j * dout;
            const float v = j < dy ? A.dec_W[(size_t)j * dout + k] : 0.f;
            s_dec[k * ldc + j] = v;
            s_dect[j * ldt + k] = v;
        }
    for (int e = tid; e < dout * dout; e += NTH) {                   // Gc[i][p], p <= i, k ascending; mirrored
        const int i = e / dout, p = e - i * dout;
        if (p <= i) {
            float s = 0.f;
            for (int k = 0; k < dy; ++k) s = fmaf(A.dec_W[(size_t)k * dout + i], A.dec_W[(size_t)k * dout + p], s);
            s /= r;
            s_G[i * dout + p] = s;
            s_G[p * dout + i] = s;
        }
    }
    FlowEval E;
    E.W = CL ? s_wm : A.w; E.c = A.c; E.s_iw2 = s_iw2; E.s_g = s_g; E.s_A = s_J; E.s_ap = s_ap; E.vg = A.vg;

    // this lane's y of a tile of 16 rows in the MFMA accumulator's layout: rows 16 yt + r4 .. + 3 of trial mi (zeros beyond dy / the batch)
    auto y_load = [&](int t, int yt, float (&v)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 16 * yt + r4 + e;
            v[e] = j < dy && mi < nb ? A.y[((size_t)t * B + b0 + mi) * dy + j] : 0.f;
        }
    };
    float yr[4];                                  // the first round of this row's y
    y_load(0, wave, yr);
    __syncthreads();

    // the trial of this lane and its indices
    const int b = ta_trial(S), l16 = ta_l16(S);
    // rows 16 yt .. 16 yt + 15 of C x for the tile's 16 trials, x at xs: K = dout in MFMA steps of 4, k ascending, the last step
    // padded with zeros.  Addresses beyond dy / dout are clamped and the value masked: nothing is read outside the arrays.
    auto decode = [&](const float* xs, int yt) {
        vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int j = 16 * yt + mi;
        const bool rv = j < dy;
        for (int k0 = 0; k0 < dout; k0 += 4) {
            const bool kv = k0 + kk < dout;
            const int k = kv ? k0 + kk : 0;
            const float cv = DL ? s_dec[k * ldc + j] : A.dec_W[rv ? (size_t)j * dout + k : 0];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32((rv && kv) ? cv : 0.f, kv ? xs[k * LD + mi] : 0.f, acc, 0, 0, 0);
        }
        return acc;
    };
    // this tile's rows of mean, var and (if asked for) cov of row t from the carried moments; cov_last at the last row.  All threads.
    auto emit = [&](int t) { ta_emit_moments(S, s_x, s_P, t, rowT, A.mean, A.var, A.cov, t == T - 1, A.cov_last); };

    bool bad = false;
    for (int t = 0; t < T; ++t) {
        // the rows of step t + 1, in flight while this step computes: the first round of y, the flags, the first of u
        const bool more = t + 1 < T;
        float yn[4] = {0.f, 0.f, 0.f, 0.f};
        if (more) y_load(t + 1, wave, yn);
        const float on = more && tid < nb && (!A.obs || A.obs[(size_t)(t + 1) * B + b0 + tid]) ? 1.f : 0.f;
        const float* un = more && du > 0 ? A.u + ((size_t)(t + 1) * B + b0) * du : nullptr;
        const float u0 = fc_u_ahead(S, un);

        flow_evaluate<CL, NO>(S, E);              // g, A at [m, u_t]
        const bool obs = s_obs[b] > 0.f;

        // factor: Ls in P's place; m^-; whether this row's inputs are finite
        {
            float nf = 0.f;
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int i = l16 + 16 * e;
                if (i < dout) {
                    const float xi = s_x[i * LD + b];
                    s_mp[i * LD + b] = xi + s_g[i * LD + b];
                    nf += ta_isfin(xi) ? 0.f : 1.f;
                }
            }
            for (int j = dout + l16; j < d; j += 16) nf += ta_isfin(s_x[j * LD + b]) ? 0.f : 1.f;
            const float nfs = ta_sum16(nf);          // (every lane of the wavefront takes part)
            bad = bad || nfs > 0.f;
        }
        const bool okS = ta_factor<NO>(b, l16, dout, s_P);
        __syncthreads();

        // K = J Ls: row i of J; K[i][c] needs J[i][k] for k >= c only, so it takes A's place for c ascending
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i < dout) {
                float* ji = s_J + (size_t)i * LD + b;             // J[i][k] - delta_ik at ji[k * dout * LD]
                for (int c = 0; c < dout; ++c) {
                    float k = 0.f;
                    for (int p = c; p < dout; ++p) k = fmaf(ji[(size_t)p * dout * LD] + (p == i ? 1.f : 0.f), s_P[ta_tri(p, c) * LD + b], k);
                    ji[(size_t)c * dout * LD] = k;
                }
            }
        }
        __syncthreads();

        // predict: row i of P^- = K K^T + q I; Lp in its place
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i < dout) {
                const float* ki = s_J + (size_t)i * LD + b;
                for (int p = 0; p <= i; ++p) {
                    const float* kp = s_J + (size_t)p * LD + b;
                    float s = p == i ? q : 0.f;
                    for (int c = 0; c < dout; ++c) s = fmaf(ki[(size_t)c * dout * LD], kp[(size_t)c * dout * LD], s);
                    s_Pp[ta_tri(i, p) * LD + b] = s;
                }
            }
        }
        const bool okP = ta_factor<NO>(b, l16, dout, s_Pp);
        __syncthreads();

        // W = Gc Lp: column p, in K's place; zero where the row is not observed
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int p = l16 + 16 * e;
            if (p < dout) {
                for (int a = 0; a < dout; ++a) {
                    float s = 0.f;
                    for (int c = dout - 1; c >= p; --c) s = fmaf(s_G[a * dout + c], s_Pp[ta_tri(c, p) * LD + b], s);
                    s_J[((size_t)a * dout + p) * LD + b] = obs ? s : 0.f;
                }
            }
        }
        __syncthreads();

        // M = I + Lp^T W: row i; Lm in its place
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i < dout) {
                for (int p = 0; p <= i; ++p) {
                    float s = p == i ? 1.f : 0.f;
                    for (int a = dout - 1; a >= i; --a) s = fmaf(s_Pp[ta_tri(a, i) * LD + b], s_J[((size_t)a * dout + p) * LD + b], s);
                    s_M[ta_tri(i, p) * LD + b] = s;
                }
            }
        }
        const bool okM = ta_factor<NO>(b, l16, dout, s_M);
        __syncthreads();

        // Y = Lm^-1 Lp^T: column c by the forward solve, in W's place
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int c = l16 + 16 * e;
            if (c < dout) {
                float* yc = s_J + (size_t)c * LD + b;             // Y[k][c] at yc[k * dout * LD]
                for (int k = 0; k < dout; ++k) {
                    float s = k <= c ? s_Pp[ta_tri(c, min(k, c)) * LD + b] : 0.f;
                    for (int p = 0; p < k; ++p) s = fmaf(-s_M[ta_tri(k, p) * LD + b], yc[(size_t)p * dout * LD], s);
                    yc[(size_t)k * dout * LD] = s / s_M[ta_tri(k, k) * LD + b];
                }
            }
        }
        __syncthreads();

        // cov: row i of P = Y^T Y, in Ls's place
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i < dout) {
                const float* yi = s_J + (size_t)i * LD + b;
                for (int p = 0; p <= i; ++p) {
                    const float* yp = s_J + (size_t)p * LD + b;
                    float s = 0.f;
                    for (int k = 0; k < dout; ++k) s = fmaf(yi[(size_t)k * dout * LD], yp[(size_t)k * dout * LD], s);
                    s_P[ta_tri(i, p) * LD + b] = s;
                }
            }
        }

        // s = C^T v / r, v = y - b - C m^-: rounds of four tiles of 16 rows of y, one per wavefront (s_mp is complete since the
        // barrier behind `factor`; s_ap and s_part are free behind flow_evaluate)
        {
            vjf_f32x4 sacc[NO];
#pragma unroll
            for (int ot = 0; ot < NO; ++ot) sacc[ot] = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
            const bool om = s_obs[mi] > 0.f;
            for (int y0 = 0; y0 < ntile; y0 += NW) {
                const int yt = y0 + wave;
                const bool tv = yt < ntile;                          // (uniform over the wavefront)
                if (tv) {
                    const vjf_f32x4 acc = decode(s_mp, yt);
                    float yv[4];
                    if (y0 == 0) { yv[0] = yr[0]; yv[1] = yr[1]; yv[2] = yr[2]; yv[3] = yr[3]; }
                    else y_load(t, yt, yv);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int j = 16 * yt + r4 + e;
                        const float bj = A.dec_b[j < dy ? j : 0];
                        s_v[(wave * 16 + r4 + e) * LD + mi] = om && j < dy ? yv[e] - bj - acc[e] : 0.f;
                    }
                }
                __syncthreads();
                if (tv) {
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int j = 16 * yt + 4 * qq + kk;
                        const float bv = s_v[(wave * 16 + 4 * qq + kk) * LD + mi];
#pragma unroll
                        for (int ot = 0; ot < NO; ++ot)
                            if (ot * 16 < dout) {                    // (uniform)
                                const int i = ot * 16 + mi;
                                const bool ok = j < dy && i < dout;
                                const float cv = DL ? s_dect[j * ldt + i] : A.dec_W[ok ? (size_t)j * dout + i : 0];
                                sacc[ot] = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? cv : 0.f, bv, sacc[ot], 0, 0, 0);
                            }
                    }
                }
                __syncthreads();
            }
#pragma unroll
            for (int ot = 0; ot < NO; ++ot)
                if (ot * 16 < dout) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) S.s_part[(wave * doutp + ot * 16 + r4 + e) * LD + mi] = sacc[ot][e];
                }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i < dout) {
                float s = S.s_part[i * LD + b];
#pragma unroll
                for (int w = 1; w < NW; ++w) s += S.s_part[(w * doutp + i) * LD + b];
                s_sv[i * LD + b] = s / r;
            }
        }
        __syncthreads();

        // mean: m = m^- + P s (row i of the symmetric P); m - m^- for the evidence
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i < dout) {
                float s = 0.f;
                for (int p = 0; p < dout; ++p) s = fmaf(s_P[ta_tri(max(i, p), min(i, p)) * LD + b], s_sv[p * LD + b], s);
                const float mp = s_mp[i * LD + b];
                s_x[i * LD + b] = obs ? mp + s : mp;
                s_g[i * LD + b] = s;
            }
        }
        __syncthreads();

        // |y - b - C m|^2: per lane over its tiles, rows ascending
        {
            const bool om = s_obs[mi] > 0.f;
            float qs = 0.f;
            for (int y0 = 0; y0 < ntile; y0 += NW) {
                const int yt = y0 + wave;
                if (yt < ntile) {
                    const vjf_f32x4 acc = decode(s_x, yt);
                    float yv[4];
                    if (y0 == 0) { yv[0] = yr[0]; yv[1] = yr[1]; yv[2] = yr[2]; yv[3] = yr[3]; }
                    else y_load(t, yt, yv);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int j = 16 * yt + r4 + e;
                        const float bj = A.dec_b[j < dy ? j : 0];
                        const float v = om && j < dy ? yv[e] - bj - acc[e] : 0.f;
                        qs = fmaf(v, v, qs);
                    }
                }
            }
            s_q[(wave * 4 + kk) * LD + mi] = qs;
        }
        __syncthreads();

        // evidence: one lane per trial solves Lp z = m - m^- in place and adds the terms up; then the selects
        float ll = 0.f;
        if (l16 == 0) {
            float q2 = 0.f, ld = 0.f, q1 = 0.f;
            for (int k = 0; k < dout; ++k) {
                float s = s_g[k * LD + b];
                for (int p = 0; p < k; ++p) s = fmaf(-s_Pp[ta_tri(k, p) * LD + b], s_g[p * LD + b], s);
                s /= s_Pp[ta_tri(k, k) * LD + b];
                s_g[k * LD + b] = s;
                q2 = fmaf(s, s, q2);
                ld += logf(s_M[ta_tri(k, k) * LD + b]);
            }
            for (int p = 0; p < 16; ++p) q1 += s_q[p * LD + b];
            ll = -0.5f * (lconst + 2.f * ld + q1 / r + q2);
        }
        ll = __shfl(ll, 0, 16);
        bad = bad || !okS || !okP || (obs && (!okM || !ta_isfin(ll)));
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i < dout && bad) {
                s_x[i * LD + b] = qnan;
                for (int p = 0; p <= i; ++p) s_P[ta_tri(i, p) * LD + b] = qnan;
            }
        }
        if (l16 == 0 && b < nb) A.ll[(size_t)t * B + b0 + b] = bad ? qnan : (obs ? ll : 0.f);
        __syncthreads();

        emit(t);
        // the rows of step t + 1 into LDS
        if (more) {
            if (tid < TB) s_obs[tid] = on;
            fc_u_advance(S, un, u0);
            yr[0] = yn[0]; yr[1] = yn[1]; yr[2] = yn[2]; yr[3] = yn[3];
        }
        __syncthreads();
    }
}
}  // namespace
