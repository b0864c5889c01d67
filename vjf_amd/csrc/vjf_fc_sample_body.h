// vjf_fc_sample_body.h -- the body of one weight sample, included inside vjf_fc_weights_kernel and vjf_fe_weights_kernel (no include
// guard: it is program text of both, so both compute the same bits and the first keeps its instructions).  Expects in scope:
// nz (the sample's noise), Wt (its output), A.w_mean, s_a (w_chol's 16 rows, k-major), m0, col, r4, n, dout, lane.
        for (int j0 = 0; j0 < dout; j0 += 16) {
            vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            mma_tile(acc, nz, dout, dout, j0, s_a, n, lane);
            if (m0 + col < n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = j0 + r4 + r;
                    if (j < dout) Wt[(size_t)(m0 + col) * dout + j] = A.w_mean[(size_t)(m0 + col) * dout + j] + acc[r];
                }
            }
        }
