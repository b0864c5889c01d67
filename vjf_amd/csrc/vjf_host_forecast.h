// vjf_host_forecast.h -- host side of vjf_forecast_seq / vjf_forecast_ens: the overrides the tests set, the chunk planners (pure
// arithmetic on the shapes and those overrides), the forms of the roll-out kernels, one dispatch on them, and the one chunk loop.
// Included by vjf_abi.hip only, behind vjf_host_ctx.h (fail, allow_lds, kMaxLds).
#pragma once
#include "vjf_forecast_kernel.h"        // the sampled roll-out: vjf_fc_weights_kernel, vjf_fc_rollout_kernel
#include "vjf_forecast_ens_kernel.h"    // the ensemble of roll-outs: vjf_fe_weights_kernel, vjf_fe_rollout_kernel, vjf_fe_moments_kernel

namespace {

// ---- overrides (tests), read by the entry points on every call: VJF_FC_CENTROID_LDS=0 / VJF_FC_LOOKAHEAD=0 switch a form off,
//      VJF_FC_CHUNK / VJF_FE_MEMBERS ask for fewer steps / members per chunk (0: not set)
bool fc_env_on(const char* name) { const char* v = getenv(name); return !(v && atoi(v) == 0 && v[0] == '0'); }
int fc_env_int(const char* name) { const char* v = getenv(name); return v ? atoi(v) : 0; }

// ---- planners
// Steps per chunk of vjf_forecast_seq: the weight samples of a chunk (n dout floats per step) take at most kFcScratchBytes, and a
// chunk is at most kFcMaxChunk steps (a roll-out launch stays on the device for milliseconds, not seconds); `chunk` (VJF_FC_CHUNK)
// asks for shorter chunks.
constexpr size_t kFcScratchBytes = (size_t)8 << 20;
constexpr int kFcMaxChunk = 4096;
int fc_chunk_bound(int n, int dout) {
    const size_t per = (size_t)n * dout * 4;
    const size_t c = kFcScratchBytes / per;
    return c < 1 ? 1 : (c > (size_t)kFcMaxChunk ? kFcMaxChunk : (int)c);
}
int fc_chunk(int n, int dout, int chunk) {
    const int bound = fc_chunk_bound(n, dout);
    return chunk >= 1 && chunk < bound ? chunk : bound;
}
// (four rows of padding behind the last W[t]: a wavefront whose share of K is shorter than 4 features -- n = 37: 12, 12, 12, 1 --
//  hands mma_tile a K < 4, whose lanes kk >= K read row kb + kk, up to n + 2, from a valid address and mask the value)
size_t fc_scratch_bytes(int T, int n, int dout) {
    const int bound = fc_chunk_bound(n, dout);
    return ((size_t)(T < bound ? T : bound) * n * dout * 4 + (size_t)4 * dout * 4 + 255) / 256 * 256;
}

// Chunks of vjf_forecast_ens: Sc members x Tc steps whose weight samples take at most kFcScratchBytes and whose states (Tc + 1 rows
// of B dout floats per member) at most kFeStateBytes; where one member-step is more than a cap, the chunk is that one member-step.
// As many members side by side as the caps allow while a chunk keeps kFeMinChunk steps (a launch per chunk of steps is worth that
// many), the member chunks levelled; `members` / `chunk` (VJF_FE_MEMBERS / VJF_FC_CHUNK) ask for fewer members / steps per chunk.
constexpr size_t kFeStateBytes = (size_t)32 << 20;
constexpr int kFeMaxMembers = 4096, kFeMinChunk = 16;
struct FeChunks { int Sc, Tc; };
FeChunks fe_chunks(int T, int S, int B, int n, int dout, int members, int chunk) {
    const size_t wstep = (size_t)n * dout * 4, xstep = (size_t)B * dout * 4;
    // steps per chunk that `sc` members leave room for: sc tc samples within kFcScratchBytes and sc (tc + 1) rows within
    // kFeStateBytes; 0 where not even one step of `sc` members fits
    auto steps = [&](int sc) {
        const size_t w = kFcScratchBytes / wstep / sc, rows = kFeStateBytes / xstep / sc, x = rows > 1 ? rows - 1 : 0;
        size_t t = w < x ? w : x;
        t = t > (size_t)kFcMaxChunk ? (size_t)kFcMaxChunk : t;
        return (int)(t > (size_t)T ? (size_t)T : t);
    };
    // members that `tc` steps leave room for (0: not one)
    auto room = [&](int tc) {
        const size_t w = kFcScratchBytes / wstep / tc, x = kFeStateBytes / xstep / ((size_t)tc + 1);
        return w < x ? w : x;
    };
    const int want = T < kFeMinChunk ? T : kFeMinChunk;
    int sc = S < kFeMaxMembers ? S : kFeMaxMembers;
    if (steps(sc) < want) {                              // fewer members, so that a chunk keeps `want` steps; else as many as one step allows
        size_t m = room(want);
        if (m < 1) m = room(1);
        sc = m < 1 ? 1 : (m < (size_t)sc ? (int)m : sc);
    }
    const int nch = (S + sc - 1) / sc;
    sc = (S + nch - 1) / nch;
    if (members >= 1 && members < sc) sc = members;
    int tc = steps(sc);
    if (tc < 1) tc = 1;                                  // (sc = 1 here: one member-step, more than a cap)
    if (chunk >= 1 && chunk < tc) tc = chunk;
    return FeChunks{sc, tc};
}
// min(a b per, cap), at least `least`, without overflow
size_t fe_capped(int a, int64_t b, size_t per, size_t cap, size_t least) {
    const size_t room = cap / per;
    const size_t v = (size_t)a * (size_t)b <= room ? (size_t)a * (size_t)b * per : cap;
    return v < least ? least : v;
}
// [weight samples of a chunk + four rows of padding (fc_scratch_bytes)] [states of a chunk]: whatever chunking the call takes
size_t fe_w_bytes(int T, int S, int n, int dout) {
    const size_t wstep = (size_t)n * dout * 4;
    return (fe_capped(S, T, wstep, kFcScratchBytes, wstep) + (size_t)4 * dout * 4 + 255) / 256 * 256;
}
size_t fe_x_bytes(int T, int S, int B, int dout) {
    const size_t xstep = (size_t)B * dout * 4;
    return (fe_capped(S, (int64_t)T + 1, xstep, kFeStateBytes, 2 * xstep) + 255) / 256 * 256;
}

// ---- the forms of the kernels, chosen once per call for both entry points.  VJF_FC_CENTROID_LDS=0 / VJF_FC_LOOKAHEAD=0 (tests):
//      the forms for shapes beyond the LDS / register budgets, at any shape
struct FcForms { bool fits, cl, la; size_t lds, lds_w; };   // fits LDS at all (else the entry point refuses); centroids in LDS; look-ahead; dynamic LDS: roll-out, weights
FcForms fc_forms(int n, int d, int dout) {
    const bool cl = vjf_fc_lds_floats(n, d, dout, true) * 4 <= kMaxLds - 1024 && fc_env_on("VJF_FC_CENTROID_LDS");
    const bool la = cl && vjf_fc_reg_form(n, dout) && fc_env_on("VJF_FC_LOOKAHEAD");
    return FcForms{vjf_fc_lds_floats(n, d, dout, false) * 4 <= kMaxLds - 1024, cl, la, vjf_fc_lds_floats(n, d, dout, cl) * 4, (size_t)n * VJF_LDT * 4};
}
// the moments kernel: the same two switches also take the decoder out of LDS and the batched staging out of the kernel
struct FeMomForms { int mb; bool dl; size_t lds; };      // members staged per barrier; decoder rows in LDS; dynamic LDS
FeMomForms fe_mom_forms(int dout, int dy) {
    const int mb = vjf_fe_lds_floats(dout, VJF_FE_BATCH, false) * 4 <= kMaxLds / 4 && fc_env_on("VJF_FC_LOOKAHEAD") ? VJF_FE_BATCH : 1;
    const bool dl = dy > 0 && vjf_fe_lds_floats(dout, mb, true) * 4 <= kMaxLds / 2 && fc_env_on("VJF_FC_CENTROID_LDS");
    return FeMomForms{mb, dl, vjf_fe_lds_floats(dout, mb, dl) * 4};
}
// f(NT, CL) with the x step's template arguments as std::integral_constant / std::bool_constant values: the one dispatch on the two
// switches (la implies cl), for the roll-out kernels and the tangent kernel
template <class F> void with_fc_form(bool la, bool cl, int dout, F&& f) {
    if (la && dout <= 16) f(std::integral_constant<int, 1>{}, std::true_type{});
    else if (la) f(std::integral_constant<int, 2>{}, std::true_type{});
    else if (cl) f(std::integral_constant<int, 0>{}, std::true_type{});
    else f(std::integral_constant<int, 0>{}, std::false_type{});
}
template <class F> void with_fe_mom_form(const FeMomForms& fm, F&& f) { if (fm.dl) f(std::true_type{}); else f(std::false_type{}); }
// grid rows of a weights kernel: a wavefront per sample, at most 2048 workgroups in all
unsigned fc_weights_rows(int mt, int64_t samples) {
    const int64_t cap = 2048 / mt, gy = (samples + VJF_FC_WAVES - 1) / VJF_FC_WAVES, g = gy > cap ? cap : gy;
    return (unsigned)(g < 1 ? 1 : g);
}
// ---- one chunk's roll-out arguments from `a`, what the call's chunks share (u, c, logw, tr_logvar and the sizes, filled by the entry
//      point): steps t0 .. t0 + Tc - 1 from the row `x_in` (x[t0]) to rows x[t0 + 1 ..] at `x_out`; `e`: the roll-out's state noise
//      (T, B, dout) or null.  REQUIRED of x_out: the row in front of it belongs to the chunk too (the first chunk copies its start, x[0],
//      there).  For an ensemble these are member 0 of the chunk; the member strides are the loop's.
VjfFcArgs fc_chunk_args(VjfFcArgs a, const float* W, const float* e, int t0, int Tc, const float* x_in, float* x_out) {
    const size_t xstep = (size_t)a.B * a.dout;
    a.x_in = x_in; a.W = W; a.Tc = Tc; a.x_out = x_out; a.x0_out = t0 == 0 ? x_out - xstep : nullptr;
    if (a.u) a.u += (size_t)t0 * a.B * (a.d - a.dout);
    a.e = e ? e + (size_t)t0 * xstep : nullptr;
    return a;
}

// ---- both forecasts behind their argument checks.  ens == null, vjf_forecast_seq: one member whose states go into `x`, chunks of steps,
//      vjf_fc_* kernels, no moments.  Else vjf_forecast_ens: `x` is x_members or null, chunks of members x steps, vjf_fe_* kernels, every
//      chunk folded into the running moments (`mom`: the decoder, the outputs, S, dy and mb, filled by the entry point).
struct FeEns { VjfFeMomArgs mom; FeMomForms mf; int64_t x0_ms; int members; };
int forecast_run(const VjfFcArgs& base, const float* w_mean, const float* w_chol, const float* x0, const float* w_noise, const float* s_noise,
                 float* x, void* scratch, int T, const FcForms& fm, int chunk_override, const FeEns* ens, hipStream_t s) {
    const int B = base.B, n = base.n, dout = base.dout, S = ens ? ens->mom.S : 1, dy = ens ? ens->mom.dy : 0;
    const size_t wstep = (size_t)n * dout, xstep = (size_t)B * dout, ystep = (size_t)B * dy, x0_ms = ens ? (size_t)ens->x0_ms : 0;
    const int tiles = (B + 15) / 16, mt = (n + 15) / 16, zg = ((dout + 15) / 16 + (dy + 15) / 16 + VJF_FE_GROUP - 1) / VJF_FE_GROUP;
    // rows r0 .. r0 + rows - 1 of the outputs from `rows` rows of states of members ms0 .. ms0 + Sc - 1
    auto moments = [&](const float* xs, size_t xs_ms, int r0, int rows, int ms0, int Sc) {
        VjfFeMomArgs m = ens->mom;
        m.xs = xs; m.xs_ms = xs_ms; m.x_mean += (size_t)r0 * xstep; m.x_var += (size_t)r0 * xstep;
        if (dy) { m.y_mean += (size_t)r0 * ystep; m.y_var += (size_t)r0 * ystep; }
        m.Sc = Sc; m.ms0 = ms0; m.last = ms0 + Sc == S;
        with_fe_mom_form(ens->mf, [&](auto dl) {
            auto kernel = vjf_fe_moments_kernel<decltype(dl)::value>;
            allow_lds(kernel, ens->mf.lds);
            hipLaunchKernelGGL(kernel, dim3(tiles, rows, zg), dim3(VJF_FE_THREADS), ens->mf.lds, s, m);
        });
    };
    if (T == 0) {                                        // (ensemble only) nothing to roll out: the moments of the starts, x_members is not written
        moments(x0, x0_ms, 0, 1, 0, S);
        VJF_HIP(hipGetLastError());
        return 0;
    }
    const FeChunks ch = ens ? fe_chunks(T, S, B, n, dout, ens->members, chunk_override) : FeChunks{1, fc_chunk(n, dout, chunk_override)};
    if (ens && ((size_t)ch.Sc * ch.Tc * wstep * 4 + (size_t)4 * dout * 4 > fe_w_bytes(T, S, n, dout) ||
                (size_t)ch.Sc * (ch.Tc + 1) * xstep * 4 > fe_x_bytes(T, S, B, dout)))
        return fail(-11, "vjf_forecast_ens: a chunk of %d members x %d steps is beyond the scratch", ch.Sc, ch.Tc);
    float* W = (float*)scratch;
    float* X = ens ? (float*)((char*)scratch + fe_w_bytes(T, S, n, dout)) : nullptr;
    // the members' states of a chunk: in `x` where they are kept, else in the scratch, (ch.Tc + 1) rows per member
    const size_t xs_ms = x ? (size_t)(T + 1) * xstep : (size_t)(ch.Tc + 1) * xstep;
    if (ens) allow_lds(vjf_fe_weights_kernel, fm.lds_w);
    else allow_lds(vjf_fc_weights_kernel, fm.lds_w);
    for (int32_t ms0 = 0; ms0 < S; ms0 += ch.Sc) {
        const int Sc = S - ms0 < ch.Sc ? S - ms0 : ch.Sc;
        int Tp = 0;                                      // steps of the previous chunk
        for (int32_t t0 = 0; t0 < T; t0 += ch.Tc) {
            const int Tc = T - t0 < ch.Tc ? T - t0 : ch.Tc;
            const float* wn = w_noise + ((size_t)ms0 * T + t0) * wstep;
            if (ens) {
                VjfFeWeightArgs wa{w_mean, w_chol, wn, W, (size_t)T * wstep, Sc, Tc, n, dout};
                hipLaunchKernelGGL(vjf_fe_weights_kernel, dim3(mt, fc_weights_rows(mt, (int64_t)Sc * Tc)), dim3(VJF_FC_THREADS), fm.lds_w, s, wa);
            } else {
                VjfFcWeightArgs wa{w_mean, w_chol, wn, W, Tc, n, dout};
                hipLaunchKernelGGL(vjf_fc_weights_kernel, dim3(mt, fc_weights_rows(mt, Tc)), dim3(VJF_FC_THREADS), fm.lds_w, s, wa);
            }
            VJF_HIP(hipGetLastError());
            // row 0 of the chunk's states is x[t0] (the start, or the previous chunk's last row), rows 1 .. Tc are x[t0 + 1 ..]
            float* rows = x ? x + (size_t)ms0 * xs_ms + (size_t)t0 * xstep : X;
            const float* x_in = t0 == 0 ? x0 + (size_t)ms0 * x0_ms : (x ? rows : X + (size_t)Tp * xstep);
            VjfFeArgs e{};
            e.a = fc_chunk_args(base, W, s_noise ? s_noise + (size_t)ms0 * T * xstep : nullptr, t0, Tc, x_in, rows + xstep);
            e.x_in_ms = t0 == 0 ? x0_ms : xs_ms; e.e_ms = (size_t)T * xstep; e.W_ms = (size_t)Tc * wstep;
            e.x0_out_ms = t0 == 0 ? xs_ms : 0; e.x_out_ms = xs_ms;
            with_fc_form(fm.la, fm.cl, dout, [&](auto nt, auto cl) {
                constexpr int NT = decltype(nt)::value;
                constexpr bool CL = decltype(cl)::value;
                if (ens) {
                    allow_lds(vjf_fe_rollout_kernel<NT, CL>, fm.lds);
                    hipLaunchKernelGGL((vjf_fe_rollout_kernel<NT, CL>), dim3(tiles, Sc), dim3(VJF_FC_THREADS), fm.lds, s, e);
                } else {
                    allow_lds(vjf_fc_rollout_kernel<NT, CL>, fm.lds);
                    hipLaunchKernelGGL((vjf_fc_rollout_kernel<NT, CL>), dim3(tiles), dim3(VJF_FC_THREADS), fm.lds, s, e.a);
                }
            });
            VJF_HIP(hipGetLastError());
            if (ens && t0 == 0) moments(rows, xs_ms, 0, Tc + 1, ms0, Sc);
            else if (ens) moments(rows + xstep, xs_ms, t0 + 1, Tc, ms0, Sc);
            VJF_HIP(hipGetLastError());
            Tp = Tc;
        }
    }
    return 0;
}

}  // namespace
