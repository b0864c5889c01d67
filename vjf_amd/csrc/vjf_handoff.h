// vjf_handoff.h -- the hand-off protocol between workgroups that run beside each other (other streams, other roles of one launch),
// device code only: the bounded poll of a count or flag word, the waits and signals of a whole workgroup built on it, the verdict
// that ends every other wait once one has been given up, and the sc1 loads / write-through stores of the handed-off bytes.
//
// Producer, whole workgroup: write-through stores (vjf_st_wt, vjf_st4_wt), every storing wavefront drains its vmcnt, the workgroup
// barrier, one lane adds to the count (vjf_wg_signal_wt).  Consumer, whole workgroup: one lane polls (vjf_poll_count /
// vjf_poll_flag: relaxed, bounded, a look at the status word every 256 polls), the workgroup barrier, and then sc1 loads ONLY
// (vjf_ld_sc1, vjf_ld4_sc1) -- no acquire (MI355X guide, "sc1 loads in place of the acquire").  One plain load of a handed-off byte
// reads stale data whenever the line sits in this CU's L1: tools/audit_plain_loads.py lists every plain load of the resident kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "vjf_plan.h"

// Bound of every wait of one kernel for another (polls; ~2 us each with the sleep between them, VJF_POLL_SLEEP: ~4 s).  Long enough for a
// host that is late with its launches, or a peer rank that is late with its half of a collective; short enough that a sequence
// that really is stuck (a launch held behind a resident kernel's hardware queue) is given up quickly.
#define VJF_WAIT_SPINS (1u << 21)
// s_sleep argument (units of 64 cycles) between two polls of a hand-off word in memory.  The polls of a launch -- 256 workgroups, most
// of them waiting most of the time -- all go to the few memory-side lines of the counter block, and they delay each other AND the
// write-through traffic of the step: with back-to-back polls (1) config B ran 56.3 us a step, with 12: 55.1, 24: 53.4-53.8,
// 40: 52.3-52.8, 64: 53.2 (same box, two runs each; a poll every ~1 us costs less in detection latency than the contention of
// faster ones; four out-of-phase pollers per workgroup: 60.4).  Spreading the counters over 4-KB pages of their own changed nothing.
// (Config C, whose trial role takes its operands from L2, would like 64 better: 74.8 against 76.5 us a step; config B 53.2 against 52.5.)
#ifndef VJF_POLL_SLEEP_LITE
#define VJF_POLL_SLEEP_LITE 16
#endif
#ifndef VJF_POLL_SLEEP
#define VJF_POLL_SLEEP 40
#endif
// -DVJF_CHAOS (diagnostic builds only, tools/chaos_handoffs.sh): one workgroup in eight is held for up to 200 us in front of a wait or
// a signal, so that an access which is ordered by the usual timing of the roles and not by a hand-off shows as a wrong result.
#ifdef VJF_CHAOS
__device__ int vjf_chaos_range[6] = {0, 1 << 30, -1, 0, 20000, 7};          // workgroups [lo, hi) are held (VJF_CHAOS_LO / _HI) at count word [2] (-1: any; VJF_CHAOS_SITE), kind [3] (0 any, 1 waits, 2 signals),
                                                                            // for up to [4] ticks of 10 ns (VJF_CHAOS_TICKS), one time in [5] + 1 (a mask; VJF_CHAOS_MASK)
__device__ const unsigned* vjf_chaos_base = nullptr;
#endif
__device__ __forceinline__ void vjf_chaos(int tid, const unsigned* count, int kind) {
#ifdef VJF_CHAOS
    if (tid == 0 && (int)blockIdx.x >= vjf_chaos_range[0] && (int)blockIdx.x < vjf_chaos_range[1] &&
        (vjf_chaos_range[2] < 0 || count - vjf_chaos_base == vjf_chaos_range[2]) && (vjf_chaos_range[3] == 0 || vjf_chaos_range[3] == kind)) {
        const unsigned long long t0 = wall_clock64();                       // 100 MHz
        unsigned h = ((unsigned)t0 * 2654435761u) ^ (blockIdx.x * 40503u);
        h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
        const unsigned d = (h & (unsigned)vjf_chaos_range[5]) == 0u ? (h >> 8) % (unsigned)vjf_chaos_range[4] : 0u;
        while (wall_clock64() - t0 < d) __builtin_amdgcn_s_sleep(8);
    }
#endif
}
// A wait that ran out somewhere in the sequence (status detail bits 0x1ff00, include/vjf_hip.h) ends every other wait at once:
// the sequence is lost anyway (the host re-runs it), and nothing should sit through its own bound step after step.
__device__ __forceinline__ bool vjf_abort_seen(const float* status) {
    if (!status) return false;
    const float f = __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return ((unsigned)f & VJF_STATUS_WAIT_MASK) != 0u;
}
// The same verdict for a whole workgroup: the lane that polled in the wait just before (vjf_wg_wait / vjf_wg_wait_sc1, given a status
// word) read the status word once more behind its poll and left what it saw in this LDS word in front of the wait's barrier --
// every thread of the workgroup takes the SAME decision to leave (a thread-by-thread read could split a workgroup around its later
// barriers when the bits are raised between two threads' loads).  4 bytes of static LDS in the kernels that wait.
__shared__ int vjf_s_abort_word;
__device__ __forceinline__ bool vjf_abort_wg() { return vjf_s_abort_word != 0; }
// THE poll of a count word, by one lane: until the count has reached `target` (wrap-around compare), at most SPINS polls, SLEEP
// (units of 64 cycles, see VJF_POLL_SLEEP) between two of them, and every 256 polls a look at the status word (null: none) for a
// wait given up elsewhere.  False: not there -- the caller raises its own status bit.  How a wait is paced and how it gives up is
// decided here and nowhere else.
template <int SLEEP, unsigned SPINS = VJF_WAIT_SPINS>
__device__ __forceinline__ bool vjf_poll_count(const unsigned* w, unsigned target, const float* status) {
    bool there = false;
    for (unsigned spins = 0; spins < SPINS; ++spins) {
        if ((int)(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) >= 0) { there = true; break; }
        if ((spins & 255u) == 255u && vjf_abort_seen(status)) break;
        __builtin_amdgcn_s_sleep(SLEEP);
    }
    return there;
}
// The same for a flag word (epoch << 1) | failed: 0 = there, 1 = there and failed, 2 = timed out (or a wait given up elsewhere).
template <int SLEEP>
__device__ __forceinline__ int vjf_poll_flag(const unsigned* w, unsigned epoch, const float* status) {
    int st = 2;
    for (unsigned spins = 0; spins < VJF_WAIT_SPINS; ++spins) {
        const unsigned v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((v >> 1) == epoch) { st = (int)(v & 1u); break; }
        if ((spins & 255u) == 255u && vjf_abort_seen(status)) break;
        __builtin_amdgcn_s_sleep(SLEEP);
    }
    return st;
}
// The signal of a workgroup whose outputs went out as write-through stores (in memory once vmcnt has drained): no L2 write-back
// (an agent-scope release by every workgroup of a kernel that runs beside the trial kernel costs that kernel microseconds).
__device__ __forceinline__ void vjf_wg_signal_wt(unsigned* count, int tid) {
    vjf_chaos(tid, count, 2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The wait without the acquire: for consumers that read EVERY handed-off byte with sc1 loads (which bypass this CU's vector L1;
// the producer stored write-through and drained before it signalled) -- MI355X guide, "sc1 loads in place of the acquire".  One
// lane polls, the workgroup barrier, then the sc1 loads.
// `fence` = true adds the acquire (VJF_HANDOFF_ACQUIRE=1; the default of the one-launch route is the sc1 loads alone).
#define VJF_FLAG_HANDOFF_ACQUIRE 0x40000000u      /* internal flag bit of the kernels' `flags` words */
// (SLEEP: the pause between two polls, in units of 64 cycles -- the training launch has ~250 workgroups polling one 1-KB block and
//  wants them a microsecond apart, VJF_POLL_SLEEP; the launches without an RLS update have a third of the pollers and take 16)
template <int SLEEP = VJF_POLL_SLEEP>
__device__ __forceinline__ bool vjf_wg_wait_sc1(const unsigned* count, unsigned target, int tid, const float* status = nullptr, bool fence = false) {
    bool there = true;
    vjf_chaos(tid, count, 1);
    if (tid == 0) {
        there = vjf_poll_count<SLEEP>(count, target, status);
        if (fence) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        vjf_s_abort_word = (!there || vjf_abort_seen(status)) ? 1 : 0;
    }
    __syncthreads();
    return there;
}
// The wait WITH the acquire, for consumers that go on with plain loads (the producer's stores were written back by a kernel's end or
// an agent-scope release in front of its count, vjf_count_kernel): one lane polls, acquires at agent scope, its vmcnt drained, the
// workgroup barrier, and only then the plain loads (MI355X guide, visibility across XCDs, valid forms).
// Both waits return false (lane 0 only; the others get true) when the count did not arrive within the bound.
__device__ __forceinline__ bool vjf_wg_wait(const unsigned* count, unsigned target, int tid, const float* status = nullptr) {
    bool there = true;
    vjf_chaos(tid, count, 1);
    if (tid == 0) {
        there = vjf_poll_count<VJF_POLL_SLEEP>(count, target, status);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        vjf_s_abort_word = (!there || vjf_abort_seen(status)) ? 1 : 0;
    }
    __syncthreads();
    return there;
}
// OR status bits into the status scalar (a float holding a small integer).  Kernels of one step may run on two
// streams (vjf_filter_seq), so the read-modify-write is a compare-and-swap loop.
__device__ __forceinline__ void vjf_status_or(float* p, unsigned bits) {
    unsigned* u = reinterpret_cast<unsigned*>(p);
    unsigned old = *u, assumed;
    do {
        assumed = old;
        const float nv = (float)((unsigned)__uint_as_float(assumed) | bits);
        old = atomicCAS(u, assumed, __float_as_uint(nv));
    } while (old != assumed);
}

// ---- the handed-off bytes.  4-byte agent-scope atomics: the load bypasses this CU's vector L1 (sc1), the store is write-through.
__device__ __forceinline__ float vjf_ld_sc1(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void vjf_st_wt(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void vjf_st_wt(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// 16-byte sc1 loads (buffer_load_dwordx4 ... sc1): what another workgroup stored write-through, read past this CU's vector L1.
// The descriptor's base must be workgroup-uniform (it lives in scalar registers; word 3 = 0x00020000: raw 32-bit data format); the
// per-lane part is the 32-bit float index.  With `nfloats` the descriptor is bounded: a load past the end returns zeros.
typedef unsigned vjf_u4 __attribute__((ext_vector_type(4)));
typedef float vjf_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t vjf_rsrc(const float* uniform_base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(uniform_base), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t vjf_rsrc(const float* uniform_base, size_t nfloats) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(uniform_base), 0, (int)(nfloats * 4), 0x00020000);
}
// the same as a PLAIN load (through this CU's L1): only for bytes that are constants of the launch by the time they are first read
__device__ __forceinline__ float4 vjf_ld4_plain(__amdgpu_buffer_rsrc_t r, int float_index) {
    const vjf_u4 v = __builtin_amdgcn_raw_buffer_load_b128(r, float_index * 4, 0, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}
__device__ __forceinline__ float4 vjf_ld4_sc1(__amdgpu_buffer_rsrc_t r, int float_index) {
    const vjf_u4 v = __builtin_amdgcn_raw_buffer_load_b128(r, float_index * 4, 0, 16);               // aux 16 = sc1
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}
// 16-byte write-through store.  The asm store is not counted by the compiler: every hand-off that follows drains vmcnt by hand
// before it signals (vjf_wg_signal_wt does; a wavefront that publishes on its own writes the s_waitcnt itself).
__device__ __forceinline__ void vjf_st4_wt(float* p, vjf_f32x4 o) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(o) : "memory");
}
__device__ __forceinline__ void vjf_st4_wt(float* p, float x, float y, float z, float w) { vjf_st4_wt(p, vjf_f32x4{x, y, z, w}); }
