// vjf_host_ops.h -- host side of the stand-alone operators (the kernels: vjf_ops_kernels.h): what each entry point of vjf_abi.hip
// calls behind its argument checks.  Included by vjf_abi.hip only, behind vjf_host_launch.h (launch_wide_gemm).
#pragma once

namespace {

// slot of the loss kernels' partial-sum table for this call (handed out in turn: VJF_LOSS_SLOTS calls may be in flight)
inline int loss_slot() { static std::atomic<unsigned> next{0}; return (int)(next.fetch_add(1u, std::memory_order_relaxed) % VJF_LOSS_SLOTS); }

int launch_rbf(const float* x, const float* centroid, const float* logwidth, float* out, int B, int n, int d, hipStream_t s) {
    const size_t lds = (size_t)16 * d * 4;
    if (lds > kMaxLds - 1024) return fail(-11, "vjf_rbf_forward: d=%d too large", d);
    allow_lds(vjf_rbf_kernel, lds);
    hipLaunchKernelGGL(vjf_rbf_kernel, dim3((n + 255) / 256, (B + 15) / 16), dim3(256), lds, s, x, centroid, logwidth, out, B, n, d);
    VJF_HIP(hipGetLastError());
    return 0;
}
// the three scalar losses (vjf_loss_kernel's `mode`; operands a mode does not read are null)
int launch_loss(int mode, const float* m1, const float* lv1, const float* m2, const float* lv2, const float* logvar, float* out, int B,
                int d, hipStream_t s) {
    hipLaunchKernelGGL(vjf_loss_kernel, dim3(VJF_LOSS_BLOCKS), dim3(256), 0, s, mode, m1, lv1, m2, lv2, logvar, out, B, d, loss_slot());
    VJF_HIP(hipGetLastError());
    return 0;
}
// Phi W (a.mean) and the row norm of Phi w_chol (a.logvar, or null) of vjf_blr_predict / vjf_blr_sample
int launch_predict(const char* who, const VjfPredArgs& a, hipStream_t s) {
    const size_t lds = ((size_t)a.n * VJF_LDT + 64) * 4;
    if (lds > kMaxLds - 1024) return fail(-11, "%s: n=%d too large", who, a.n);
    allow_lds(vjf_blr_predict_kernel, lds);
    hipLaunchKernelGGL(vjf_blr_predict_kernel, dim3((a.B + 15) / 16), dim3(VJF_K1_THREADS), lds, s, a);
    VJF_HIP(hipGetLastError());
    return 0;
}
// ---- the stand-alone RLS / Kalman updates
// plan for the stand-alone RLS (only the fields the Gram kernels read for kind-0 jobs)
void rls_plan(int n, int dout, VjfPlan* P) {
    memset(P, 0, sizeof *P);
    P->n = n; P->dz = dout;
    P->ldE = (int)vjf_align(n + dout, VJF_TILE);
    P->red_SCA = 0; P->red_G = 0; P->red_FDX = n * n; P->red_SC = (int)vjf_align((int64_t)n * n + (int64_t)n * dout, 4);
    P->red_len = P->red_SC + RS_N;
}
struct RlsCarve { size_t E, slabs, red, work, jobs, partial, total; int njobs, nsplit; };
RlsCarve rls_carve(int B, int n, int dout, std::vector<VjfJob>* jobs_out) {
    VjfPlan P; rls_plan(n, dout, &P);
    std::vector<VjfJob> jobs; build_jobs(P, jobs);
    // build_jobs also emits gradient jobs from the (zeroed) plan: keep kind 0 only
    std::vector<VjfJob> k0;
    for (auto& j : jobs) if (j.kind == 0) k0.push_back(j);
    RlsCarve c{};
    c.njobs = (int)k0.size(); c.nsplit = split_for(B);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = (o + bytes + 255) / 256 * 256; return at; };
    c.E = take((size_t)B * P.ldE * 4);
    c.slabs = take((size_t)c.njobs * c.nsplit * 1024 * 4);
    c.red = take((size_t)P.red_len * 4);
    VjfPlan Q = P;
    c.work = take(vjf_serial_work_floats(Q) * 4);
    c.jobs = take(k0.size() * sizeof(VjfJob));
    c.partial = take(RS_N * 4);
    c.total = o;
    if (jobs_out) *jobs_out = k0;
    return c;
}
// the statistics of the stand-alone RLS / Kalman updates: rows [Phi | target] -> Gram tiles -> their reduction; G and Phi^T target are
// then in the scratch's reduce buffer (*red_out), laid out as `P` (rls_plan) says
int rls_statistics(const VjfPlan& P, void* scratch, const float* x, const float* centroid, const float* logwidth, const float* target,
                   int B, int n, int d, int dout, hipStream_t s, RlsCarve* carve, float** red_out) {
    std::vector<VjfJob> jobs;
    const RlsCarve c = rls_carve(B, n, dout, &jobs);
    char* ws = (char*)scratch;
    VJF_HIP(hipMemcpyAsync(ws + c.jobs, jobs.data(), jobs.size() * sizeof(VjfJob), hipMemcpyHostToDevice, s));
    VJF_HIP(hipStreamSynchronize(s));     // host vector goes out of scope
    VJF_HIP(hipMemsetAsync(ws + c.partial, 0, RS_N * 4, s));
    float* E = (float*)(ws + c.E);
    hipLaunchKernelGGL(vjf_rls_rows_kernel, dim3((unsigned)(((size_t)B * P.ldE + 255) / 256)), dim3(256), 0, s, x, centroid, logwidth, target, E, B, n, d, dout, P.ldE);
    VJF_HIP(hipGetLastError());
    VjfGramArgs g{};
    g.jobs = (const VjfJob*)(ws + c.jobs); g.E = E; g.ACT = E; g.DEL = E; g.slabs = (float*)(ws + c.slabs);
    g.B = B; g.nsplit = c.nsplit; g.rows_per_split = ((B + c.nsplit - 1) / c.nsplit + 7) / 8 * 8;
    hipLaunchKernelGGL(vjf_gram_kernel, dim3(c.njobs * c.nsplit), dim3(VJF_GRAM_THREADS), 0, s, P, g);
    VJF_HIP(hipGetLastError());
    VjfReduceArgs r{};
    r.jobs = g.jobs; r.slabs = g.slabs; r.partial = (const float*)(ws + c.partial); r.red = (float*)(ws + c.red);
    r.njobs = c.njobs; r.nsplit = c.nsplit; r.nblocks_k1 = 1;
    hipLaunchKernelGGL(vjf_gram_reduce_kernel, dim3(c.njobs), dim3(VJF_REDUCE_THREADS), 0, s, P, r);   // sc_mask = 0: no loss sums here
    VJF_HIP(hipGetLastError());
    *carve = c; *red_out = r.red;
    return 0;
}
// vjf_blr_rls / vjf_blr_kalman behind their argument checks: the plan, the refusal of an n beyond the single-workgroup kernel's LDS
// (`words`: the caller's name for that kernel), the statistics, then the caller's `fill(a, st)` of the kernel's arguments and the launch
struct RlsStats { VjfPlan P; RlsCarve c; float* red; char* ws; };
// bytes of one of the Kalman update's six temporaries, which lie behind the RLS carve in its scratch
size_t kalman_stride(int n, int dout) { return ((size_t)n * (n > dout ? n : dout) * 4 + 255) / 256 * 256; }
template <class Args, class Fill>
int rls_update(const char* who, const char* words, void (*kernel)(Args), void* scratch, const float* x, const float* target,
               const float* centroid, const float* logwidth, int B, int n, int d, int dout, void* stream, Fill&& fill) {
    hipStream_t s = (hipStream_t)stream;
    RlsStats st{};
    rls_plan(n, dout, &st.P);
    const size_t lds = vjf_serial_lds_floats(st.P) * 4;
    if (lds > kMaxLds - 1024) return fail(-11, "%s: n=%d too large for the single-workgroup %s", who, n, words);
    if (int rc = rls_statistics(st.P, scratch, x, centroid, logwidth, target, B, n, d, dout, s, &st.c, &st.red)) return rc;
    st.ws = (char*)scratch;
    allow_lds(kernel, lds);
    Args a{};
    fill(a, st);
    hipLaunchKernelGGL(kernel, dim3(1), dim3(VJF_K2_THREADS), lds, s, a);
    VJF_HIP(hipGetLastError());
    return 0;
}
// vjf_recognition_forward(_act): act null or Tanh -> the Tanh kernel
int recognition_forward(const char* who, const float* y, const float* u, const float* mu_s, const float* lv_s, const float* const* rec_W,
                        const float* const* rec_b, const float* mean_W, const float* lv_W, const float* lv_b, float* mu_t,
                        float* lv_t, int32_t B, int32_t ydim, int32_t udim, int32_t xdim, int32_t n_hidden,
                        const int32_t* hidden, const VjfAct* act, void* stream) {
    if (!y || !mu_s || !lv_s || !rec_W || !rec_b || !mean_W || !lv_W || !lv_b || !mu_t || !lv_t || !hidden)
        return fail(-1, "%s: null tensor", who);
    if (udim > 0 && !u) return fail(-21, "%s: u is required when udim > 0", who);
    if (n_hidden < 1 || n_hidden > VJF_MAX_HIDDEN) return fail(-3, "%s: n_hidden=%d", who, n_hidden);
    if (B < 1) return fail(-20, "%s: bad shape", who);
    VjfRecArgs a{};
    a.y = y; a.u = u; a.mu_s = mu_s; a.lv_s = lv_s; a.mean_W = mean_W; a.lv_W = lv_W; a.lv_b = lv_b; a.mu_t = mu_t; a.lv_t = lv_t;
    a.B = B; a.dy = ydim; a.du = udim; a.dz = xdim; a.L = n_hidden;
    int hmax = 0;
    for (int l = 0; l < n_hidden; ++l) { a.W[l] = rec_W[l]; a.b[l] = rec_b[l]; a.h[l] = hidden[l]; if (hidden[l] > hmax) hmax = hidden[l]; }
    const size_t lds = (size_t)VJF_LDT * (ydim + udim + 2 * xdim + 2 * hmax) * 4;
    if (lds > kMaxLds - 1024) return fail(-10, "%s: layer widths do not fit LDS", who);
    with_act_kernel(act ? *act : VjfAct{VJF_ACT_TANH, 0.f, 0.f}, vjf_recognition_kernel, vjf_recognition_act_kernel, [&](auto kernel, auto... tail) {
        allow_lds(kernel, lds);
        hipLaunchKernelGGL(kernel, dim3((B + 15) / 16), dim3(VJF_K1_THREADS), lds, (hipStream_t)stream, a, hmax, tail...);
    });
    VJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace
