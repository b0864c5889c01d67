// vjf_fixed_point_kernel.h -- fixed points of the mean map of RBFDS.forward(sampling=False):  g(x, u) = Phi([x, u]) w_mean = 0, the
// velocity of f(x, u) = x + g(x, u);  A = dg/dx = -w_mean^T G,  G[k][j] = phi_k (x_j - c_kj) / width_k^2  (J = I + A: vjf_tangent_kernel.h).
//
//   vjf_fixed_point_kernel   one workgroup per tile of 16 trials runs the whole damped Newton (Levenberg-Marquardt) search on |g|^2 of
//                            include/vjf_hip.h inside the kernel, the state in LDS: per candidate the features of [xc, u], g = Phi w_mean
//                            (the x step's product) and the columns of A, then per trial the accept / reject step, M = A^T A, b = A^T g,
//                            the Cholesky factor of M + lam mu I and the two triangular solves.
//
// Column j of A for the tile's 16 trials is one MFMA product: its A operand is w_mean^T (shared by every trial and every j), its B
// operand the n x 16 matrix  phi[k][b] (c[k][j] - x[b][j]) / width_k^2  formed in registers from the features in LDS, so the dout
// columns are dout accumulator tiles, `vg` of them per pass (the partial products of a pass are in LDS together).  K is split over the
// four wavefronts as in the x step (fc_k_range) and the four partial products are added in a fixed order.
// The per-trial linear algebra runs four trials per wavefront, sixteen lanes per trial: lane l of a trial owns rows l and l + 16 of M,
// of the factor L and of every vector, and reads and writes no other row in LDS; what another lane needs comes by a shuffle inside
// the sixteen.  Every sum is taken in a fixed order (serial, or a butterfly over the sixteen lanes), a trial is one MFMA column, and
// every decision is a select on per-trial values: a trial's bits depend on that trial's inputs alone.
// Workgroups are independent: no cooperative launch, no hand-off, no scratch, no atomics.  Included by vjf_host_fixed_point.h.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_trial_algebra.h"       // the lane view, ta_tri, ta_sum16; vjf_flow_eval.h: VJF_FLOW_MV, the x step's FcTile, fc_stage

#define VJF_FP_MV VJF_FLOW_MV       // columns of A whose accumulators a wavefront holds while it walks its share of K
#define VJF_FP_MAXDOUT 32            // dout <= 32: two rows per lane in the per-trial linear algebra, two output tiles of w_mean^T

namespace {
struct VjfFpArgs {
    const float* x0;         // (B, dout)
    const float* u;          // (B, du) or null
    const float* c; const float* logw;     // centroids (n, d), log widths (n)
    const float* w;          // w_mean (n, dout)
    float* x;                // (B, dout)
    float* residual;         // (B)
    int32_t* n_iter;         // (B)
    int32_t* converged;      // (B)
    float* jac;              // (B, dout, dout) or null
    int B, n, d, dout, max_iter;
    int vg;                  // columns of A per pass
    float tol, lam0;
};

// the x step's buffers plus 1 / width^2, the accepted x, g and b, A (the factor L takes its place between two evaluations), the lower
// triangle of M, one pass's partial products and (cen_lds) w_mean
static inline size_t vjf_fixed_point_lds_floats(int n, int d, int dout, int vg, bool cen_lds) {
    return vjf_trial_lds_floats(n, d, dout, vg, cen_lds, 3, 1);
}

// CL: centroids and w_mean in LDS (else read from global memory when they are used);  NO: output tiles of w_mean^T, dout <= 16 NO --
// and so the rows a lane owns in the per-trial linear algebra.
template <bool CL, int NO>
__global__ __launch_bounds__(VJF_FC_THREADS) void vjf_fixed_point_kernel(VjfFpArgs A) {
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_FC_WAVES, NTH = VJF_FC_THREADS, MV = VJF_FP_MV;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    FcTile S = fc_tile(smem, A.n, A.d, A.dout, A.B);     // s_phi, s_x (the candidate [xc, u]), s_part, s_w2: the x step's
    const int n = S.n, d = S.d, dout = S.dout, vg = A.vg, doutp = S.doutp, ntri = dout * (dout + 1) / 2;
    float* s_x = S.s_x;
    float* s_iw2 = S.rest;                        // n            1 / width^2
    float* s_xa = s_iw2 + n;                      // dout x LD    the accepted x
    float* s_g = s_xa + dout * LD;                // dout x LD    g at the candidate
    float* s_b = s_g + dout * LD;                 // dout x LD    A^T g at the accepted x
    float* s_A = s_b + dout * LD;                 // dout x dout x LD   A at the candidate, [j][i][trial]; behind the accept step the
    float* s_L = s_A;                             //              lower triangle of the factor L, [i (i + 1) / 2 + p][trial]
    float* s_M = s_A + dout * dout * LD;          // ntri x LD    lower triangle of A^T A at the accepted x
    float* s_ap = s_M + ntri * LD;                // NW x vg x doutp x LD   the wavefronts' partial products of one pass
    const float* s_c = S.s_c = s_ap + NW * vg * doutp * LD;   // n x d   centroids (CL): behind this kernel's buffers
    float* s_wm = S.s_c + n * d;                  // n x dout     w_mean (CL)
    const int tid = S.tid, wave = S.wave, b0 = S.b0, nb = S.nb, mi = S.mi, kk = S.kk, r4 = S.r4;
    const size_t row0 = (size_t)b0 * dout;

    fc_stage<CL, true>(S, A.logw, A.c, s_iw2, A.x0, nullptr, A.u);
    if (CL) for (int i = tid; i < n * dout; i += NTH) s_wm[i] = A.w[i];
    for (int i = tid; i < (ntri + dout) * LD; i += NTH) (i < ntri * LD ? s_M[i] : s_b[i - ntri * LD]) = 0.f;
    __syncthreads();
    for (int i = tid; i < dout * LD; i += NTH) s_xa[i] = s_x[i];
    const float* W = CL ? s_wm : A.w;

    // g and A at the candidate in s_x: into s_g and s_A.  Barriers inside; s_x is complete before it and s_g, s_A behind it.
    // (flow_evaluate's statements, kept here: with the call in their place this kernel runs 5 % longer, profiles/trial_algebra_ab.txt)
    auto evaluate = [&]() {
        fc_features<CL>(S, A.c);
        __syncthreads();
        fc_product_masked(S, W);                  // Phi w_mean, K split over the four wavefronts as in the roll-out
        for (int v0 = 0; v0 < dout; v0 += vg) {
            const int vn = min(vg, dout - v0);
            for (int g0 = 0; g0 < vn; g0 += MV) {
                vjf_f32x4 acc[MV][NO];
                float xj[MV];
#pragma unroll
                for (int vv = 0; vv < MV; ++vv) {
                    xj[vv] = s_x[(g0 + vv < vn ? v0 + g0 + vv : 0) * LD + mi];
#pragma unroll
                    for (int ot = 0; ot < NO; ++ot) acc[vv][ot] = vjf_f32x4{0.f, 0.f, 0.f, 0.f};
                }
                for (int k0 = S.kb; k0 < S.ke; k0 += 4) {
                    const bool kv = k0 + kk < S.ke;
                    const int k = kv ? k0 + kk : S.kb;
                    const float gr = S.s_phi[k * LD + mi] * s_iw2[k];
                    float aw[NO];
#pragma unroll
                    for (int ot = 0; ot < NO; ++ot) {
                        aw[ot] = 0.f;
                        if (ot * 16 < dout) {                            // (uniform)
                            const bool ok = kv && ot * 16 + mi < dout;
                            const float wv = W[ok ? (size_t)k * dout + ot * 16 + mi : 0];
                            aw[ot] = ok ? wv : 0.f;
                        }
                    }
#pragma unroll
                    for (int vv = 0; vv < MV; ++vv)
                        if (g0 + vv < vn) {                              // (uniform)
                            const int j = v0 + g0 + vv;
                            const float cv = CL ? s_c[k * d + j] : A.c[(size_t)k * d + j];
                            const float bv = kv ? gr * (cv - xj[vv]) : 0.f;
#pragma unroll
                            for (int ot = 0; ot < NO; ++ot)
                                if (ot * 16 < dout) acc[vv][ot] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[ot], bv, acc[vv][ot], 0, 0, 0);
                        }
                }
#pragma unroll
                for (int vv = 0; vv < MV; ++vv)
                    if (g0 + vv < vn) {
#pragma unroll
                        for (int ot = 0; ot < NO; ++ot)
                            if (ot * 16 < dout) {
#pragma unroll
                                for (int r = 0; r < 4; ++r) s_ap[((wave * vg + g0 + vv) * doutp + ot * 16 + r4 + r) * LD + mi] = acc[vv][ot][r];
                            }
                    }
            }
            __syncthreads();
            // the four partials in a fixed order
            if (v0 == 0)
                for (int i = tid; i < dout * TB; i += NTH) {
                    const int b = i & (TB - 1), j = i / TB;
                    float s = S.s_part[j * LD + b];
#pragma unroll
                    for (int w = 1; w < NW; ++w) s += S.s_part[(w * doutp + j) * LD + b];
                    s_g[j * LD + b] = s;
                }
            for (int i = tid; i < vn * dout * TB; i += NTH) {
                const int b = i & (TB - 1), r = i / TB, vl = r / dout, ii = r - vl * dout;
                float s = s_ap[(vl * doutp + ii) * LD + b];
#pragma unroll
                for (int w = 1; w < NW; ++w) s += s_ap[((w * vg + vl) * doutp + ii) * LD + b];
                s_A[((v0 + vl) * dout + ii) * LD + b] = s;
            }
            __syncthreads();
        }
    };

    // the trial of this lane and its rows
    const int b = ta_trial(S), l16 = ta_l16(S);
    const bool bv = b < nb;
    const float tol2 = A.tol * A.tol;
    float r2 = INFINITY, lam = A.lam0;            // (the same in the sixteen lanes of a trial)
    bool done = !bv;                              // rows beyond the batch hold zeros and are never touched
    int nit = 0;
    __syncthreads();

    for (int k = 0;; ++k) {
        evaluate();
        // accept or reject the candidate
        if (!done) {
            float r2c = 0.f;
            for (int i = 0; i < dout; ++i) { const float gi = s_g[i * LD + b]; r2c = fmaf(gi, gi, r2c); }
            if (r2c < r2) {                       // (a NaN compares false)
                r2 = r2c;
                if (k > 0) lam = fmaxf(lam / 10.f, 1e-7f);
#pragma unroll
                for (int e = 0; e < NO; ++e) {
                    const int j = l16 + 16 * e;
                    if (j < dout) {
                        s_xa[j * LD + b] = s_x[j * LD + b];
                        const float* aj = s_A + (size_t)j * dout * LD + b;
                        float bj = 0.f;
                        for (int i = 0; i < dout; ++i) bj = fmaf(aj[i * LD], s_g[i * LD + b], bj);
                        s_b[j * LD + b] = bj;
                        for (int p = 0; p <= j; ++p) {
                            const float* ap = s_A + (size_t)p * dout * LD + b;
                            float m = 0.f;
                            for (int i = 0; i < dout; ++i) m = fmaf(aj[i * LD], ap[i * LD], m);
                            s_M[ta_tri(j, p) * LD + b] = m;
                        }
                    }
                }
            } else {
                lam = fminf(lam * 10.f, 1e7f);
            }
            done = r2 <= tol2;
        }
        if (k == A.max_iter) break;
        if (__syncthreads_and(done)) break;       // (and the barrier between the reads of A and the writes of L in its place)

        // the step from the accepted x: K = M + lam mu I = L L^T, K delta = -b, xc = x + delta
        const bool act = !done;
        if (__ballot(act) != 0) {                 // (uniform over the wavefront: the shuffles below are executed by all of it or none)
            if (act) ++nit;
            float dg = 0.f;
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int i = l16 + 16 * e;
                if (i < dout) dg += s_M[ta_tri(i, i) * LD + b];
            }
            const float shift = lam * (ta_sum16(dg) / (float)dout);
            // (ta_factor's statements with M + shift I read from s_M, kept here: shared, this kernel ran 0.8 % longer, profiles/trial_algebra_ab.txt)
            bool ok = true;
            for (int j = 0; j < dout; ++j) {
                const int own = j & 15, ej = j >> 4;
                const int rj = min(l16 + 16 * ej, dout - 1);              // the row of this lane that lane `own` has as row j
                float a[2] = {0.f, 0.f};
#pragma unroll
                for (int e = 0; e < NO; ++e) {
                    const int i = l16 + 16 * e;
                    a[e] = (i >= j && i < dout) ? s_M[ta_tri(i, j) * LD + b] + (i == j ? shift : 0.f) : 0.f;
                }
                for (int p = 0; p < j; ++p) {
                    const float ljp = __shfl(s_L[ta_tri(rj, min(p, rj)) * LD + b], own, 16);
#pragma unroll
                    for (int e = 0; e < NO; ++e) {
                        const int i = l16 + 16 * e;
                        if (i >= j && i < dout) a[e] = fmaf(-s_L[ta_tri(i, p) * LD + b], ljp, a[e]);
                    }
                }
                const float piv = __shfl(ej ? a[1] : a[0], own, 16);
                ok = ok && piv > 0.f && piv < INFINITY;
                const float dj = sqrtf(piv);
#pragma unroll
                for (int e = 0; e < NO; ++e) {
                    const int i = l16 + 16 * e;
                    if (i >= j && i < dout) s_L[ta_tri(i, j) * LD + b] = i == j ? dj : a[e] / dj;
                }
            }
            // L y = -b, column by column: y_j is final once the columns before it are taken off
            float t[2] = {0.f, 0.f};
#pragma unroll
            for (int e = 0; e < NO; ++e) {
                const int i = l16 + 16 * e;
                t[e] = i < dout ? -s_b[i * LD + b] : 0.f;
            }
            for (int j = 0; j < dout; ++j) {
                const int own = j & 15, ej = j >> 4;
                const int rj = min(l16 + 16 * ej, dout - 1);
                const float yj = __shfl((ej ? t[1] : t[0]) / s_L[ta_tri(rj, min(j, rj)) * LD + b], own, 16);
#pragma unroll
                for (int e = 0; e < NO; ++e) {
                    const int i = l16 + 16 * e;
                    if (i == j) t[e] = yj;
                    else if (i > j && i < dout) t[e] = fmaf(-s_L[ta_tri(i, j) * LD + b], yj, t[e]);
                }
            }
            // L^T delta = y, from the last row up: row j of L^T is column j of L, a row per lane, summed over the sixteen lanes
            for (int j = dout - 1; j >= 0; --j) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < NO; ++e) {
                    const int i = l16 + 16 * e;
                    if (i > j && i < dout) s = fmaf(s_L[ta_tri(i, j) * LD + b], t[e], s);
                }
                s = ta_sum16(s);
#pragma unroll
                for (int e = 0; e < NO; ++e)
                    if (l16 + 16 * e == j) t[e] = (t[e] - s) / s_L[ta_tri(j, j) * LD + b];
            }
            if (act) {
#pragma unroll
                for (int e = 0; e < NO; ++e) {
                    const int i = l16 + 16 * e;
                    if (i < dout) { const float xa = s_xa[i * LD + b]; s_x[i * LD + b] = ok ? xa + t[e] : xa; }
                }
            }
        }
        __syncthreads();
    }

    if (bv && l16 == 0) {
        A.residual[b0 + b] = sqrtf(r2);
        A.n_iter[b0 + b] = nit;
        A.converged[b0 + b] = done ? 1 : 0;
    }
    __syncthreads();
    for (int i = tid; i < nb * dout; i += NTH) {
        const int bb = i / dout, j = i - bb * dout;
        A.x[row0 + i] = s_xa[j * LD + bb];
    }
    if (A.jac) {                                  // one more evaluation, at the returned x: J = I + A
        for (int i = tid; i < dout * LD; i += NTH) s_x[i] = s_xa[i];
        __syncthreads();
        evaluate();
        for (int i = tid; i < nb * dout * dout; i += NTH) {
            const int bb = i / (dout * dout), r = i - bb * dout * dout, ii = r / dout, j = r - ii * dout;
            A.jac[row0 * dout + i] = (ii == j ? 1.f : 0.f) + s_A[(j * dout + ii) * LD + bb];
        }
    }
}
}  // namespace
