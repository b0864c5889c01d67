// vjf_recognition_kernel.h -- the stand-alone Recognition.forward kernel (vjf_host_ops.h: recognition_forward), included twice from
// vjf_ops_kernels.h behind mma_tile, VJF_LDT, VJF_K1_THREADS and vjf_act.h:
//   VJF_RECOGNITION_ACT 0: vjf_recognition_kernel (tanh);  1: vjf_recognition_act_kernel (the activation `act`, vjf_act.h).
// (two textual instantiations, as vjf_trial_mfma_body.h: the Tanh kernel's code stays what it was; no include guard but the
//  argument struct's.  Both kernels in an anonymous namespace: their symbols carry it.)
namespace {
#ifndef VJF_REC_ARGS_DEFINED
#define VJF_REC_ARGS_DEFINED
struct VjfRecArgs {
    const float* y; const float* u; const float* mu_s; const float* lv_s;
    const float* W[VJF_MAX_HIDDEN]; const float* b[VJF_MAX_HIDDEN];
    const float* mean_W; const float* lv_W; const float* lv_b;
    float* mu_t; float* lv_t;
    int B, dy, du, dz, L; int h[VJF_MAX_HIDDEN];
};
#endif
#if VJF_RECOGNITION_ACT
__global__ __launch_bounds__(VJF_K1_THREADS) void vjf_recognition_act_kernel(VjfRecArgs A, int hmax, VjfAct act) {
#else
__global__ __launch_bounds__(VJF_K1_THREADS) void vjf_recognition_kernel(VjfRecArgs A, int hmax) {
#endif
    constexpr int TB = 16, LD = VJF_LDT, NW = VJF_K1_THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int din = A.dy + A.du + 2 * A.dz;
    float* s_in = smem;                  // din x LD
    float* s_a = s_in + din * LD;        // hmax x LD
    float* s_b = s_a + hmax * LD;        // hmax x LD
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b0 = blockIdx.x * TB, nb = min(TB, A.B - b0);
    for (int i = tid; i < TB * din; i += VJF_K1_THREADS) {
        const int b = i / din, c = i - b * din;
        float v = 0.f;
        if (b < nb) {
            const size_t g = (size_t)(b0 + b);
            if (c < A.dy) v = A.y[g * A.dy + c];
            else if (c < A.dy + A.du) v = A.u[g * A.du + c - A.dy];
            else if (c < A.dy + A.du + A.dz) v = A.mu_s[g * A.dz + c - A.dy - A.du];
            else v = A.lv_s[g * A.dz + c - A.dy - A.du - A.dz];
        }
        s_in[c * LD + b] = v;
    }
    __syncthreads();
    const int col = lane & 15, r4 = 4 * (lane >> 4);     // accumulator: row = r4 + r (output unit), column = trial
    const float* xin = s_in; int kin = din;
    float* cur = s_a; float* nxt = s_b;
    for (int l = 0; l < A.L; ++l) {
        const int hl = A.h[l];
        const float* bias = A.b[l];
        for (int t = wave; t * 16 < hl; t += NW) {
            vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            mma_tile<true>(acc, A.W[l], kin, hl, t * 16, xin, kin, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = t * 16 + r4 + r;
#if VJF_RECOGNITION_ACT
                if (f < hl) cur[f * LD + col] = vjf_act_fwd(act, acc[r] + bias[f]);
#else
                if (f < hl) cur[f * LD + col] = tanhf(acc[r] + bias[f]);
#endif
            }
        }
        __syncthreads();
        xin = cur; kin = hl;
        float* t = cur; cur = nxt; nxt = t;
    }
    const int nt = (A.dz + 15) / 16;                         // tiles per head; the wavefronts take mean tiles, then log-variance tiles
    for (int t = wave; t < 2 * nt; t += NW) {
        const bool lvh = t >= nt;
        const int f0 = (lvh ? t - nt : t) * 16;
        vjf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        mma_tile<true>(acc, lvh ? A.lv_W : A.mean_W, kin, A.dz, f0, xin, kin, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = f0 + r4 + r;
            if (f < A.dz && col < nb) {
                if (lvh) A.lv_t[(size_t)(b0 + col) * A.dz + f] = acc[r] + A.lv_b[f];
                else A.mu_t[(size_t)(b0 + col) * A.dz + f] = acc[r];
            }
        }
    }
}
}  // namespace
