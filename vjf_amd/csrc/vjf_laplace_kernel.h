// vjf_laplace_kernel.h -- the filter of the learned generative model with count observations over a record (include/vjf_hip.h:
// vjf_laplace_filter), forwards: per trial, with f = x + g the mean map, J = I + A its Jacobian at (m, u_t), q the state-noise variance,
// eta = C x + b the decoder and y_j ~ Poisson(exp(eta_j)),
//     predict    m^- = m + g,   Ls Ls^T = P,   K = J Ls,   P^- = K K^T + q I = Lp Lp^T                       (vjf_ekf_kernel.h's, copied)
//     mode       x = m^- + Lp z;  phi(z) = sum_j (lam_j - y_j eta_j) + |z|^2 / 2,  lam = exp(eta);  Newton steps on z with the step
//                halved twice where phi does not fall:  H = sum_j lam_j c_j c_j^T,  M = I + Lp^T H Lp = Lm Lm^T,
//                grad = z - Lp^T C^T (y - lam),  dz = -M^-1 grad
//     posterior  m = m^- + Lp z,   Lm Y = Lp^T,   P = Y^T Y
//     evidence   ll = sum_j (y_j eta_j - lam_j - lgamma(y_j + 1)) - |z|^2 / 2 - sum log diag(Lm)
// M is bounded below by I and P is a Gram matrix, as in the EKF; what is new is that H, which the EKF forms once per call as C^T C / r,
// is a different matrix per trial, per row and per Newton iteration.
//
//   vjf_laplace_kernel   one workgroup per tile of 16 trials walks the whole record inside the kernel; m (in the x step's s_x) and the
//                    lower triangle of P stay in LDS.  Per row the three predict phases of vjf_ekf_kernel, then n_iter + 1 times
//       E         the decision phi_c <= phi at the candidate x_c = m^- + Lp z_c, taken on the difference formed term by term,
//                 sum_j (lam_j expm1(delta_j) - y_j delta_j) + z . d + |d|^2 / 2 with d = z_c - z and delta = C Lp d (phi itself at the
//                 start only): two decodes as MFMA products with the shared operand C (the trial on the MFMA column, dy walked in
//                 rounds of four tiles of 16 rows, one per wavefront), expf and expm1f, the sum per lane over its rows and then over
//                 the sixteen partials of a trial in a fixed order; the per-trial select z, x <- candidate
//       D         the decode at x again (the same operations: the same lam), and per round v = y - lam and lam of a tile through LDS into
//                   C^T v      the EKF's second product (k split over the wavefronts' tiles, the four sums added in a fixed order)
//                   H          the pair rows C[j][i] C[j][p], p <= i, formed by one multiply, times lam: ntri rows in tiles of 16, the
//                              tiles dealt to the wavefronts round-robin, so a wavefront walks every j ascending for its tiles and no
//                              sum crosses wavefronts; the triangle of H lies where Ls lay
//                 then per trial (sixteen lanes, a lane owning indices l and l + 16): W = H Lp (column p, in K's place), M (row i) and
//                 its factor, grad (row i), and one lane's two triangular solves for dz; where the candidate was accepted dz is the
//                 new direction and alpha = 1, elsewhere dz stays and alpha = alpha / 4
//     then the evidence's sum at the mode (the decode once more, its terms formed per element so that y eta and lgamma(y + 1) cancel
//     before they are added up), Y (column c, in W's place), cov (row i, in H's place) and the evidence.
// A row that is not observed: lam and y - lam are zero by selects, so H = 0, M = I, grad = z = 0, every candidate is 0, P = P^-,
// m = m^-; ll = grad_norm = 0 are selects.  Its y is loaded and never enters arithmetic.
// Every sum is serial in a fixed order, a trial is one MFMA column, and every decision is a select on per-trial values; no trip count
// depends on data.  A trial with a non-finite m, u or observed y, an observed y < 0, a non-finite phi at z = 0, a pivot that is not
// positive and finite or a non-finite ll has NaN written over its carried moments, ll and grad_norm: they stay NaN to the last row,
// and no other trial sees them.  (A y that is negative or NaN makes its term of phi NaN by a select; an infinite y does by arithmetic.)
// Workgroups are independent: no cooperative launch, no hand-off, no scratch, no atomics.  Included by vjf_host_laplace.h.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_trial_algebra.h"       // the lane view and helpers (ta_*); vjf_flow_eval.h: flow_evaluate, the x step's FcTile, fc_stage
#include "vjf_ekf_kernel.h"          // vjf_ekf_ldc, vjf_ekf_ldt: the rows of the decoder's two LDS copies

#define VJF_LAP_MAXDOUT 24           // dout <= 24: at most 19 tiles of pair rows, five per wavefront
#define VJF_LAP_MAXITER 64
#define VJF_LAP_VECTORS 7

namespace {
struct VjfLapArgs {
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
    float* ll; float* gn;                  // (T, B)
    float* cov_last;                       // (B, dout, dout)
    int T, B, n, d, dout, dy;
    int vg;                                // columns of A per pass
    int n_iter;
    float q;
};

// the x step's buffers plus 1 / width^2, seven vectors (g then grad; m^-; C^T (y - lam); z; dz; z_c; x_c), the block (A, K, W, Y in
// turn), the three triangles (P, Ls, H; P^-, Lp; M, Lm), one pass's partial products (y - lam of a round lies there; lam of a round lies
// in the x step's partial products), the sixteen partial sums of phi (and of the evidence), the observed flags and (dec_lds) the decoder
// twice, (cen_lds) w_mean
static inline size_t vjf_lap_lds_floats(int n, int d, int dout, int dy, int vg, bool cen_lds, bool dec_lds) {
    const size_t dyp = ((size_t)dy + 15) / 16 * 16, LD = VJF_LDT;
    return vjf_trial_lds_floats(n, d, dout, vg, cen_lds, VJF_LAP_VECTORS, 3) + 16 * LD + LD +
           (dec_lds ? (size_t)dout * vjf_ekf_ldc(dy) + dyp * vjf_ekf_ldt(dout) : 0);
}

// CL: centroids and w_mean in LDS (else read from global memory when they are used);  NO: output tiles of w_mean^T, dout <= 16 NO --
// and so the indices a lane owns in the per-trial linear algebra and the tiles of pair rows a wavefront owns;  DL: the decoder in
// LDS, else read from global memory (L2) as torch stores it.  All forms issue the same operations on the same operands in the same order.
template <bool CL, int NO, bool DL>
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_laplace_kernel(VjfLapArgs A) {
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_FC_WAVES, NTH = VJF_FC_THREADS;
    constexpr int NPW = NO == 1 ? 3 : 5;         // tiles of pair rows per wavefront: ntri <= 136 (9 tiles) or <= 300 (19)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FcTile S = fc_tile(smem, A.n, A.d, A.dout, A.B);     // s_phi, s_x ([m, u_t]; the accepted x inside a row), s_part, s_w2: the x step's
    const int n = S.n, d = S.d, dout = S.dout, du = S.du, doutp = S.doutp, ntri = dout * (dout + 1) / 2, T = A.T, B = A.B, dy = A.dy;
    const int dyp = (dy + 15) / 16 * 16, ntile = dyp / 16, ldc = (int)vjf_ekf_ldc(dy), ldt = (int)vjf_ekf_ldt(dout);
    const int npt = (ntri + 15) / 16;
    float* s_x = S.s_x;
    float* s_iw2 = S.rest;                        // n            1 / width^2
    float* s_g = s_iw2 + n;                       // dout x LD    g at m; grad, then the solves' vector
    float* s_mp = s_g + dout * LD;                // dout x LD    m^-
    float* s_sv = s_mp + dout * LD;               // dout x LD    s = C^T (y - lam)
    float* s_z = s_sv + dout * LD;                // dout x LD    z
    float* s_dz = s_z + dout * LD;                // dout x LD    dz
    float* s_zc = s_dz + dout * LD;               // dout x LD    z_c = z + alpha dz
    float* s_xc = s_zc + dout * LD;               // dout x LD    x_c = m^- + Lp z_c
    float* s_J = s_xc + dout * LD;                // dout x dout x LD   A[i][j] at [j][i]; K[i][c] at [c][i]; W[a][p] at [a][p]; Y[k][c] at [k][c]
    float* s_P = s_J + dout * dout * LD;          // ntri x LD    lower triangle of P, carried; of Ls up to K; of H inside the iteration
    float* s_Pp = s_P + ntri * LD;                // ntri x LD    lower triangle of P^-, then of its factor Lp
    float* s_M = s_Pp + ntri * LD;                // ntri x LD    lower triangle of M, then of its factor Lm
    float* s_ap = s_M + ntri * LD;                // NW x vg x doutp x LD   the wavefronts' partial products of one pass; y - lam of a round
    float* s_q = s_ap + NW * A.vg * doutp * LD;   // 16 x LD      partial sums of phi; of the evidence's sum behind the iteration
    float* s_obs = s_q + 16 * LD;                 // LD           1 where this row of the trial is observed
    float* s_dec = s_obs + LD;                    // dout x ldc   the decoder, k-major (DL)
    float* s_dect = s_dec + (DL ? dout * ldc : 0);   // dyp x ldt the decoder, j-major (DL)
    S.s_c = s_dect + (DL ? dyp * ldt : 0);        // n x d        centroids (CL): behind this kernel's buffers
    float* s_wm = S.s_c + n * d;                  // n x dout     w_mean (CL)
    float* s_v = s_ap;                            // NW x 16 x LD y - lam of a round's four tiles
    float* s_lam = S.s_part;                      // NW x 16 x LD lam of a round's four tiles
    const int tid = S.tid, wave = S.wave, b0 = S.b0, nb = S.nb, mi = S.mi, kk = S.kk, r4 = S.r4;
    const size_t rowT = (size_t)B * dout;
    const float q = A.q, qnan = __builtin_nanf("");
    const int n_iter = A.n_iter;

    // ---- stage: widths, centroids, [prior mean, u_0], the prior's triangle, the flags of row 0 and the decoder
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
    FlowEval E;
    E.W = CL ? s_wm : A.w; E.c = A.c; E.s_iw2 = s_iw2; E.s_g = s_g; E.s_A = s_J; E.s_ap = s_ap; E.vg = A.vg;

    // the pair rows of this lane: row 16 (wave + 4 m) + mi of the triangle is (pi, pp), pp <= pi; (0, 0) and masked beyond ntri
    int pi[NPW], pp[NPW];
    bool pv[NPW];
#pragma unroll
    for (int m = 0; m < NPW; ++m) {
        const int rr = 16 * (wave + NW * m) + mi;
        pv[m] = rr < ntri;
        int i = 0;
        while (pv[m] && (i + 1) * (i + 2) / 2 <= rr) ++i;
        pi[m] = pv[m] ? i : 0;
        pp[m] = pv[m] ? rr - i * (i + 1) / 2 : 0;
    }

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
        const bool om = s_obs[mi] > 0.f;

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
        // the start z = 0: its candidate is z_c = 0 (flow_evaluate's s_part and s_ap are free from here on)
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i < dout) { s_z[i * LD + b] = 0.f; s_dz[i * LD + b] = 0.f; s_zc[i * LD + b] = 0.f; }
        }
        __syncthreads();

        // ---- mode: the start (it == 0, its candidate accepted by definition) and n_iter steps
        float alpha = 1.f, gnorm = 0.f;
        bool okM = true, phi0 = true;
        for (int it = 0; it <= n_iter; ++it) {
            const bool first = it == 0;
            // x_c = m^- + Lp z_c (row i); the step d = z_c - z in x, Lp d, where s will lie; |z_c|^2 / 2 at the start, else
            // |z_c|^2 / 2 - |z|^2 / 2 = z . d + |d|^2 / 2
            float zz = 0.f;
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int i = l16 + 16 * e;
                if (i < dout) {
                    float s = 0.f, sd = 0.f;
                    for (int p = 0; p <= i; ++p) {
                        const float lp = s_Pp[ta_tri(i, p) * LD + b], zc = s_zc[p * LD + b];
                        s = fmaf(lp, zc, s);
                        sd = fmaf(lp, zc - s_z[p * LD + b], sd);
                    }
                    s_xc[i * LD + b] = s_mp[i * LD + b] + s;
                    s_sv[i * LD + b] = sd;
                    const float zi = s_z[i * LD + b], di = s_zc[i * LD + b] - zi;
                    zz = first ? fmaf(0.5f * di, di, zz) : fmaf(zi, di, fmaf(0.5f * di, di, zz));
                }
            }
            zz = ta_sum16(zz);
            __syncthreads();

            // E, per lane over its tiles, rows ascending.  At the start phi itself at x_c: sum_j (lam_j - y_j eta_j).  Behind it the
            // difference phi_c - phi, whose sign is the decision, term by term: with delta = C Lp d the candidate's eta is eta + delta,
            // so a term is lam_j expm1(delta_j) - y_j delta_j, lam at the accepted x.  (phi_c and phi rounded one by one agree in all
            // their digits long before the steps are small: the difference of the two would be rounding alone.)
            {
                float qs = 0.f;
                for (int y0 = 0; y0 < ntile; y0 += NW) {
                    const int yt = y0 + wave;
                    if (yt < ntile) {
                        const vjf_f32x4 acc = decode(first ? s_xc : s_x, yt);
                        vjf_f32x4 dl = {0.f, 0.f, 0.f, 0.f};
                        if (!first) dl = decode(s_sv, yt);
                        float yv[4];
                        if (y0 == 0) { yv[0] = yr[0]; yv[1] = yr[1]; yv[2] = yr[2]; yv[3] = yr[3]; }
                        else y_load(t, yt, yv);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int j = 16 * yt + r4 + e;
                            const bool live = om && j < dy;
                            const float eta = acc[e] + A.dec_b[j < dy ? j : 0];
                            const float lam = expf(eta);
                            const float term = first ? (yv[e] >= 0.f ? fmaf(-yv[e], eta, lam) : qnan)
                                                     : fmaf(lam, expm1f(dl[e]), -yv[e] * dl[e]);
                            qs += live ? term : 0.f;
                        }
                    }
                }
                s_q[(wave * 4 + kk) * LD + mi] = qs;
            }
            __syncthreads();
            bool accept;
            {
                float s = 0.f;
                for (int p = 0; p < 16; ++p) s += s_q[p * LD + b];
                const float dphi = s + zz;                            // phi at z = 0 at the start, else phi_c - phi
                if (first) phi0 = ta_isfin(dphi);
                accept = first || (dphi <= 0.f && ta_isfin(dphi));
#pragma unroll
                for (int e = 0; e < NO; ++e) {
                    const int i = l16 + 16 * e;
                    if (i < dout && accept) {
                        s_z[i * LD + b] = s_zc[i * LD + b];
                        s_x[i * LD + b] = s_xc[i * LD + b];
                    }
                }
            }
            __syncthreads();

            // D: lam at x again; per round v = y - lam and lam of the wavefronts' tiles through LDS into C^T v and H
            {
                vjf_f32x4 sacc[NO], hacc[NPW];
#pragma unroll
                for (int ot = 0; ot < NO; ++ot) sacc[ot] = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int m = 0; m < NPW; ++m) hacc[m] = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
                for (int y0 = 0; y0 < ntile; y0 += NW) {
                    const int yt = y0 + wave;
                    const bool tv = yt < ntile;                          // (uniform over the wavefront)
                    if (tv) {
                        const vjf_f32x4 acc = decode(s_x, yt);
                        float yv[4];
                        if (y0 == 0) { yv[0] = yr[0]; yv[1] = yr[1]; yv[2] = yr[2]; yv[3] = yr[3]; }
                        else y_load(t, yt, yv);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int j = 16 * yt + r4 + e;
                            const bool live = om && j < dy;
                            const float lam = expf(acc[e] + A.dec_b[j < dy ? j : 0]);
                            s_v[(wave * 16 + r4 + e) * LD + mi] = live ? yv[e] - lam : 0.f;
                            s_lam[(wave * 16 + r4 + e) * LD + mi] = live ? lam : 0.f;
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
                    // H: this wavefront's tiles of pair rows against lam of the round's tiles, j ascending
                    for (int w = 0; w < NW; ++w) {
                        if (y0 + w >= ntile) break;                      // (uniform)
#pragma unroll
                        for (int qq = 0; qq < 4; ++qq) {
                            const int j = 16 * (y0 + w) + 4 * qq + kk;
                            const bool jv = j < dy;
                            const float bv = s_lam[(w * 16 + 4 * qq + kk) * LD + mi];
#pragma unroll
                            for (int m = 0; m < NPW; ++m)
                                if (wave + NW * m < npt) {               // (uniform)
                                    const bool ok = jv && pv[m];
                                    const float ci = DL ? s_dect[j * ldt + pi[m]] : A.dec_W[ok ? (size_t)j * dout + pi[m] : 0];
                                    const float cp = DL ? s_dect[j * ldt + pp[m]] : A.dec_W[ok ? (size_t)j * dout + pp[m] : 0];
                                    hacc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? ci * cp : 0.f, bv, hacc[m], 0, 0, 0);
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
#pragma unroll
                for (int m = 0; m < NPW; ++m)
                    if (wave + NW * m < npt) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int rr = 16 * (wave + NW * m) + r4 + e;
                            if (rr < ntri) s_P[rr * LD + mi] = hacc[m][e];
                        }
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
                    s_sv[i * LD + b] = s;
                }
            }
            // W = H Lp: column p, in K's place (H is symmetric: its lower triangle is read)
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int p = l16 + 16 * e;
                if (p < dout) {
                    for (int a = 0; a < dout; ++a) {
                        float s = 0.f;
                        for (int c = dout - 1; c >= p; --c) s = fmaf(s_P[ta_tri(max(a, c), min(a, c)) * LD + b], s_Pp[ta_tri(c, p) * LD + b], s);
                        s_J[((size_t)a * dout + p) * LD + b] = s;
                    }
                }
            }
            __syncthreads();

            // M = I + Lp^T W: row i; Lm in its place.  grad = z - Lp^T s: row i
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int i = l16 + 16 * e;
                if (i < dout) {
                    for (int p = 0; p <= i; ++p) {
                        float s = p == i ? 1.f : 0.f;
                        for (int a = dout - 1; a >= i; --a) s = fmaf(s_Pp[ta_tri(a, i) * LD + b], s_J[((size_t)a * dout + p) * LD + b], s);
                        s_M[ta_tri(i, p) * LD + b] = s;
                    }
                    float s = 0.f;
                    for (int a = dout - 1; a >= i; --a) s = fmaf(s_Pp[ta_tri(a, i) * LD + b], s_sv[a * LD + b], s);
                    s_g[i * LD + b] = s_z[i * LD + b] - s;
                }
            }
            okM = ta_factor<NO>(b, l16, dout, s_M) && okM;
            __syncthreads();

            // dz = -M^-1 grad: one lane per trial solves Lm a = grad and Lm^T d = a in place; |grad|
            float gn = 0.f;
            if (l16 == 0) {
                float g2 = 0.f;
                for (int k = 0; k < dout; ++k) {
                    float s = s_g[k * LD + b];
                    g2 = fmaf(s, s, g2);
                    for (int p = 0; p < k; ++p) s = fmaf(-s_M[ta_tri(k, p) * LD + b], s_g[p * LD + b], s);
                    s_g[k * LD + b] = s / s_M[ta_tri(k, k) * LD + b];
                }
                for (int k = dout - 1; k >= 0; --k) {
                    float s = s_g[k * LD + b];
                    for (int p = dout - 1; p > k; --p) s = fmaf(-s_M[ta_tri(p, k) * LD + b], s_g[p * LD + b], s);
                    s /= s_M[ta_tri(k, k) * LD + b];
                    s_g[k * LD + b] = s;
                    if (accept) s_dz[k * LD + b] = -s;
                }
                gn = sqrtf(g2);
            }
            gnorm = __shfl(gn, 0, 16);
            alpha = accept ? 1.f : 0.25f * alpha;
            __syncthreads();
            // the next candidate
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int i = l16 + 16 * e;
                if (i < dout) s_zc[i * LD + b] = fmaf(alpha, s_dz[i * LD + b], s_z[i * LD + b]);
            }
            __syncthreads();
        }

        // ---- evidence: sum_j (y_j eta_j - lam_j - lgamma(y_j + 1)) at the mode, per lane over its tiles, rows ascending
        {
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
                        const float eta = acc[e] + A.dec_b[j < dy ? j : 0];
                        const float term = fmaf(yv[e], eta, -expf(eta)) - lgammaf(yv[e] + 1.f);
                        qs += om && j < dy ? term : 0.f;
                    }
                }
            }
            s_q[(wave * 4 + kk) * LD + mi] = qs;
        }

        // ---- posterior: s_x holds m = m^- + Lp z.  Y = Lm^-1 Lp^T: column c by the forward solve, in W's place
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

        // cov: row i of P = Y^T Y, in H's place
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

        // evidence: one lane per trial adds the terms up; then the selects
        float ll = 0.f;
        if (l16 == 0) {
            float ld = 0.f, zz = 0.f, s = 0.f;
            for (int k = 0; k < dout; ++k) {
                ld += logf(s_M[ta_tri(k, k) * LD + b]);
                zz = fmaf(s_z[k * LD + b], s_z[k * LD + b], zz);
            }
            for (int p = 0; p < 16; ++p) s += s_q[p * LD + b];
            ll = fmaf(-0.5f, zz, s) - ld;
        }
        ll = __shfl(ll, 0, 16);
        bad = bad || !okS || !okP || !okM || !phi0 || !ta_isfin(ll);
#pragma unroll
        for (int e = 0; e < NO; ++e) {
            const int i = l16 + 16 * e;
            if (i < dout && bad) {
                s_x[i * LD + b] = qnan;
                for (int p = 0; p <= i; ++p) s_P[ta_tri(i, p) * LD + b] = qnan;
            }
        }
        if (l16 == 0 && b < nb) {
            A.ll[(size_t)t * B + b0 + b] = bad ? qnan : (obs ? ll : 0.f);
            A.gn[(size_t)t * B + b0 + b] = bad ? qnan : (obs ? gnorm : 0.f);
        }
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
