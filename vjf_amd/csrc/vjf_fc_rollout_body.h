// vjf_fc_rollout_body.h -- the body of the roll-out of one tile of trials, included inside vjf_fc_rollout_kernel and
// vjf_fe_rollout_kernel (no include guard: it is program text of both, so a member of an ensemble computes the roll-out's bits in every
// form, and the first kernel keeps its instructions).  Expects in scope: `A` (VjfFcArgs), the template parameters NT and CL.
// KEEP IN STEP with vjf_tangent_kernel.h, whose x step restates this body (features, both MFMA loops, the reduction): a change to one belongs in both.
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_FC_WAVES, NTH = VJF_FC_THREADS, KQ = VJF_FC_KQ;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = A.n, d = A.d, dout = A.dout, du = d - dout, doutp = (dout + 15) / 16 * 16;
    float* s_phi = smem;                          // n x LD       features of step t
    float* s_x = s_phi + n * LD;                  // d x LD       [x_t, u_t]
    float* s_part = s_x + d * LD;                 // NW x doutp x LD   the wavefronts' partial products
    float* s_w2 = s_part + NW * doutp * LD;       // n            width^2
    float* s_c = s_w2 + n;                        // n x d        centroids (CL)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b0 = blockIdx.x * TB, nb = min(TB, A.B - b0);
    const size_t row0 = (size_t)b0 * dout;        // the tile's rows in a (B, dout) array are contiguous
    const size_t sx = (size_t)A.B * dout, su = (size_t)A.B * du, sw = (size_t)n * dout;

    for (int k = tid; k < n; k += NTH) { const float w = expf(A.logw[k]); s_w2[k] = w * w; }
    if (CL) for (int i = tid; i < n * d; i += NTH) s_c[i] = A.c[i];
    for (int i = tid; i < TB * dout; i += NTH) {
        const int b = i / dout, j = i - b * dout;
        float v = 0.f;
        if (b < nb) {
            v = A.x_in[row0 + i];
            if (A.x0_out) A.x0_out[row0 + i] = v;
        }
        s_x[j * LD + b] = v;
    }
    for (int i = tid; i < TB * du; i += NTH) {
        const int b = i / du, j = i - b * du;
        s_x[(dout + j) * LD + b] = b < nb ? A.u[(size_t)b0 * du + i] : 0.f;
    }
    const float sigma = A.e ? expf(0.5f * A.tr_logvar[0]) : 0.f;
    int kb, ke;
    fc_k_range(n, wave, kb, ke);
    const int mi = lane & 15, kk = lane >> 4, r4 = 4 * (lane >> 4);
    constexpr int NTR = NT > 0 ? NT : 1;
    float aw[NTR][KQ];                                    // (NT > 0) this lane's A operands of the coming step
    auto fetch_w = [&](const float* Wt) {
#pragma unroll
        for (int t = 0; t < NTR; ++t)
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                const int k = kb + 4 * q + kk, j = t * 16 + mi;
                const bool ok = k < ke && j < dout;       // (masked where the value is used: the loads stay in flight)
                aw[t][q] = Wt[ok ? (size_t)k * dout + j : 0];
            }
    };
    if (NT > 0) fetch_w(A.W);
    __syncthreads();

    for (int t = 0; t < A.Tc; ++t) {
        // this step's noise and the next step's control input: in flight while the features are computed
        float e0 = 0.f, u0 = 0.f;
        if (A.e && tid < nb * dout) e0 = A.e[(size_t)t * sx + row0 + tid];
        if (du > 0 && t + 1 < A.Tc && tid < nb * du) u0 = A.u[(size_t)(t + 1) * su + (size_t)b0 * du + tid];

        // features: exp(-1/2 |xu - c|^2 / width^2), the squared distance as a sum of squared differences
        for (int i = tid; i < TB * n; i += NTH) {
            const int k = i / TB, b = i - k * TB;
            float ph = 0.f;
            if (b < nb) {
                float d2 = 0.f;
                for (int j = 0; j < d; ++j) { const float df = s_x[j * LD + b] - (CL ? s_c[k * d + j] : A.c[(size_t)k * d + j]); d2 = fmaf(df, df, d2); }
                ph = expf(-0.5f * d2 / s_w2[k]);
            }
            s_phi[k * LD + b] = ph;
        }
        __syncthreads();

        // Phi W[t], K split over the four wavefronts: partial(row j, col trial) of features kb .. ke - 1
        const float* Wt = A.W + (size_t)t * sw;
        if (NT > 0) {
#pragma unroll
            for (int tl = 0; tl < NTR; ++tl) {
                vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                const bool rv = tl * 16 + mi < dout;
#pragma unroll
                for (int q = 0; q < KQ; ++q) {
                    const int k0 = kb + 4 * q;
                    if (k0 < ke) {                                       // (uniform over the wavefront)
                        const bool kv = k0 + kk < ke;
                        const float xv = s_phi[(kv ? k0 + kk : kb) * LD + mi];
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((rv && kv) ? aw[tl][q] : 0.f, kv ? xv : 0.f, acc, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) s_part[(wave * doutp + tl * 16 + r4 + r) * LD + mi] = acc[r];
            }
            if (t + 1 < A.Tc) fetch_w(Wt + sw);                          // W[t + 1]: used behind the next step's features
        } else {
            for (int j0 = 0; j0 < dout; j0 += 16) {
                vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                if (kb < ke) mma_tile(acc, Wt + (size_t)kb * dout, dout, dout, j0, s_phi + kb * LD, ke - kb, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) s_part[(wave * doutp + j0 + r4 + r) * LD + mi] = acc[r];
            }
        }
        __syncthreads();

        // x_{t+1} = x_t + (p0 + p1 + p2 + p3) (+ e_t sigma): the four partials in a fixed order, the noise term rounded on its
        // own as the step-by-step path rounds it
        float* xo = A.x_out + (size_t)t * sx + row0;
        for (int i = tid; i < nb * dout; i += NTH) {
            const int b = i / dout, j = i - b * dout;
            float v = s_part[j * LD + b];
#pragma unroll
            for (int w = 1; w < NW; ++w) v += s_part[(w * doutp + j) * LD + b];
            v = s_x[j * LD + b] + v;
            if (A.e) v = __fadd_rn(v, __fmul_rn(i == tid ? e0 : A.e[(size_t)t * sx + row0 + i], sigma));
            s_x[j * LD + b] = v;
            xo[i] = v;
        }
        if (du > 0 && t + 1 < A.Tc)
            for (int i = tid; i < nb * du; i += NTH) {
                const int b = i / du, j = i - b * du;
                s_x[(dout + j) * LD + b] = i == tid ? u0 : A.u[(size_t)(t + 1) * su + (size_t)b0 * du + i];
            }
        __syncthreads();
    }
