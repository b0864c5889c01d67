// vjf_host_routes.h -- host side of vjf_abi.hip: the route decision and the routes of a sequence (one-launch, three-stream,
// packed, two-stream) with the serial half of the per-step route.  Included by vjf_abi.hip behind vjf_host_launch.h.
#pragma once

namespace {
// the serial half of a step; `ta`: the trial-parallel half's arguments when this rank holds ALL trials (then a step with a non-finite
// loss component is replayed as the reference defines it), else null
int filter_global_impl(vjf_ctx* c, int32_t B_total, float* loss4, uint32_t flags, const VjfTrialArgs* ta) {
    const bool replay = ta && (flags & VJF_FLAG_SGD) && (c->fast_chol || c->plan.n > 32 * VJF_CHOL_MAXBLK);
    const float* red = c->red();
    const PrepOpts first_pass = PrepOpts().loss(loss4).pass(replay ? kReplayFollows : kNoReplay);
    if (c->fast_chol || c->plan.n > 32 * VJF_CHOL_MAXBLK) {
        // (feature counts beyond one CU's LDS: clip + SGD and scalars in the prep kernel, then the RLS update as a sequence of
        //  chip-wide launches on the matrix in global memory, vjf_rlsb_kernels.h)
        int rc = launch_prep(c, B_total, flags, red, c->fast_chol ? kPrepAll : kPrepSgd, c->stream, first_pass);
        if (rc) return rc;
        if (replay && (rc = launch_replay(c, *ta, B_total, flags, c->stream))) return rc;
        if (c->fast_chol) return launch_rls(c, B_total, flags, red, c->stream, kRlsSeparate, ta);
        return (flags & VJF_FLAG_UPDATE) ? launch_rlsb(c, B_total, flags, red, c->stream, RlsbOpts().all_trials(ta)) : 0;
    }
    VjfSerialArgs s{};
    s.state = c->state; s.red = red; s.work = c->work();
    s.loss4 = loss4; s.B_total = B_total; s.flags = flags;
    s.E = (ta && ta->B == B_total && B_total < c->plan.n) ? ta->E : nullptr;
    hipLaunchKernelGGL(vjf_serial_kernel, dim3(1), dim3(VJF_K2_THREADS), c->lds_k2, c->stream, c->plan, s);
    VJF_HIP(hipGetLastError());
    return 0;
}
// ---- the same sums as ONE collective per step ("one ncclAllReduce(sum, fp32) per step between K1 and K2 on the packed
//      buffer"): the trial-parallel half of step t, one all-reduce of the whole reduce buffer [grad | loss sums | G | Phi^T dx | sums],
//      the serial half -- on the caller's stream, in the one-stream order.  Fewer collectives (one latency of the ring per step
//      instead of two on two chains), no overlap of the RLS chain with the trial chain: which of the two wins at 8 ranks is for the
//      first 8-GPU run to say (bench.py --collectives 1|2).  Same kernels and sums as vjf_filter_local / vjf_filter_global around
//      a caller's all-reduce, bit for bit.
// `packed` false: the per-step route of a single rank -- the two halves of every step on the caller's stream, nothing between them.
int filter_seq_steps(vjf_ctx* c, int32_t T, const SeqView& s, uint32_t flags, bool packed) {
    if (packed) c->on_mega = false;
    for (int t = 0; t < T; ++t) {
        // the prep kernel keeps the transposed weight copies current inside a sequence; the generic
        // serial kernel does not, so that path refreshes them every step
        const bool fresh = t > 0 && c->fast_chol;
        int rc = launch_local(c, s.step(t), flags, fresh);
        if (rc) return rc;
        if (packed && (rc = all_reduce_sum(c, c->red(), (size_t)c->plan.red_len, c->comm_a, c->stream))) return rc;
        const VjfTrialArgs ta = trial_args(c, s.step(t), flags);           // (packed: the ranks hold shards, the serial half gets no rows)
        rc = filter_global_impl(c, packed ? s.B * c->world * c->fake_world : s.B, s.loss_at(t), flags, packed ? nullptr : &ta);
        if (rc) return rc;
    }
    return 0;
}

// ---- the one-launch route (kRouteMega): one launch of vjf_mega_kernel or vjf_mega_lite_kernel -- a grid that is resident as a
//      whole -- per chunk of steps
int filter_seq_mega(vjf_ctx* c, int32_t T, const SeqView& s, uint32_t flags) {
    const VjfPlan& P = c->plan;
    const int32_t B = s.B;
    int rc = check_step_args(c, s.step(0));
    if (rc) return rc;
    MegaShape m{};
    if (!mega_shape(P, B, c->ncu, flags, &m)) return fail(-26, "vjf_filter_seq: %d compute units are too few for the one-launch route", c->ncu);
    // (parameters that fit the trial role's LDS: it reads the image the SGD role builds at the start of the launch; else the state
    //  and its transposed copies, refreshed here)
    if (!vjf_mega_trial_lds(P, (int)(kMegaLds / 4) - 8).theta) { rc = refresh_aux(c); if (rc) return rc; }
    // every counter and flag of the launch starts at 0: the launch before it zeroed this block as its first act (the context's first
    // launch finds both blocks zeroed by vjf_ctx_create) -- no memset in front of the launch, no dispatch gap behind it
    unsigned* cnt = c->mega_counters(c->mega_launches);
    const int nbl = (P.n + 31) / 32;
    const unsigned npost = (unsigned)(2 * nbl + 1);
    float* rede[2] = {c->red_rls(0), c->red_rls(1)};
    float* stw = c->status_word();
    VjfMegaArgs A{};
    A.T = T; A.B = B; A.ntiles = m.ntiles;
    A.n_rls = m.n_rls; A.n_trial = m.n_trial; A.n_gram = m.n_gram; A.n_prep = m.n_prep; A.n_sgd = m.n_sgd;
    A.n_sgd_live = (flags & VJF_FLAG_SGD) ? m.n_sgd : 1;
    A.n_mom = m.n_mom; A.mom = c->mg_mom();
    A.y = s.y; A.u = s.u; A.eps = s.eps; A.mu0 = s.mu0; A.lv0 = s.lv0; A.mu = s.mu; A.lv = s.lv; A.loss = s.loss;
    A.state = c->state; A.aux = c->aux(); A.img = c->mg_img(); A.pmsave = c->mg_pmsave();
    A.slab_early = c->mg_early(); A.slab_late = c->mg_late(); A.gslab = c->mg_gslab();
    A.red0 = rede[0]; A.red1 = rede[1]; A.gbuf = c->work(); A.xt = c->mg_xt();
    A.cnt = cnt; A.cnt_next = c->mega_counters(c->mega_launches + 1u); A.flags = flags;
    const bool acq = c->handoff_acquire;                                   // (VJF_HANDOFF_ACQUIRE, read when the context is created)
    if (acq) A.flags |= VJF_FLAG_HANDOFF_ACQUIRE;
    A.slab_len = vjf_mega_slab_layout(P).len;
    A.early_len = ((P.n + 3) & ~3) * 16 + 8; A.late_len = A.slab_len + 8 * VJF_MG_RING;
    A.gram_rows = m.gram_rows;
    A.lds_floats = (int)(kMegaLds / 4) - 8;               // (a few static words beside the dynamic region)
    A.sl_pidx = c->mg_pidx(); A.sl_cidx = c->mg_cidx(); A.sl_grp = c->mg_grp();
    A.stamps = c->stamps ? c->mega_stamps() : nullptr;
    VjfCholArgs C{};
    C.state = c->state; C.red = rede[0]; C.red2 = rede[1]; C.gbuf = A.gbuf; C.B_total = B; C.flags = flags | (acq ? VJF_FLAG_HANDOFF_ACQUIRE : 0u);
    C.stamps = c->stamps ? c->step_stamps() : nullptr;
    C.post = 1; C.dinv_out = c->dinv(); C.ok_out = c->ok_flag();
    C.lscr = c->lscr(); C.flags_out = cnt + MG_C_COLFLAGS; C.epoch = 1; C.no_triclean = 1;
    C.pscr = c->pscr(); C.self_prep = 1; C.src_state = 1;
    C.wait_count = cnt + MG_C_PDONE; C.wait_target = 0; C.wait_stride = npost;
    C.stat_count = cnt + MG_C_STAT; C.stat_target = (unsigned)m.n_gram; C.stat_stride = (unsigned)m.n_gram;
    C.nsteps = T; C.step0 = 0;
    C.sig_word = (const unsigned long long*)(cnt + MG_C_SIGW);
    { const char* ie = getenv("VJF_DEBUG_INJECT"); C.inject_epoch = ie ? (unsigned)atoi(ie) : 0u; }   // (test hook: a hand-off of step k - 1 reports a time-out)
    VjfPostArgs Q{};
    Q.state = c->state; Q.dinv = C.dinv_out; Q.gbuf = A.gbuf; Q.lscr = C.lscr; Q.flags = cnt + MG_C_COLFLAGS; Q.epoch = 1; Q.status = stw;
    Q.k1_done = cnt + MG_C_K1; Q.k1_target = (unsigned)m.n_trial; Q.k1_stride = (unsigned)m.n_trial;
    Q.done = cnt + MG_C_PDONE; Q.started = cnt + MG_C_STARTED;
    Q.red = rede[0]; Q.red2 = rede[1]; Q.B_total = B; Q.fold_sigma = 1; Q.stamps = C.stamps; Q.undo_P = 1;
    Q.sig_word = (unsigned long long*)(cnt + MG_C_SIGW); Q.acquire = acq ? 1 : 0;
    Q.prep_count = cnt + MG_C_PREP; Q.prep_target = (unsigned)m.n_prep; Q.prep_stride = (unsigned)m.n_prep;
    Q.nsteps = T; Q.step0 = 0; Q.role = 2;
    Q.xt = c->mg_xt(); Q.xt_count = cnt + MG_C_XT;
    const bool ungated = !(flags & (VJF_FLAG_SGD | VJF_FLAG_UPDATE));       // (lite kernel: builders and moments workgroups are the same ones)
    const int grid = m.n_rls + m.n_trial + m.n_gram + m.n_prep + (ungated ? (m.n_mom > m.n_sgd ? m.n_mom : m.n_sgd) : m.n_sgd + m.n_mom);
#ifdef VJF_CHAOS
    {
        static bool told = false;
        if (!told) fprintf(stderr, "vjf chaos build: roles rls %d trial %d gram %d operand %d sgd %d\n", m.n_rls, m.n_trial, m.n_gram, m.n_prep, m.n_sgd);
        told = true;
    }
#endif
    // One resident grid: every wait in it is for a workgroup of the SAME launch, so the whole grid must be on the device at once.
    // The check is the one hipLaunchCooperativeKernel makes -- workgroups per compute unit (occupancy query, made once when the
    // context is created) x compute units >= grid -- and the launch itself is a plain one: identical residency (MI355X guide,
    // "Residency and cooperative launch"), and no cooperative queue.  That queue is why the API is avoided: a process that has
    // made ONE cooperative launch faults in the HIP runtime's exit handler when it runs under rocprofv3 (hsa queue teardown behind
    // the profiler's finalisation; tools/coop_exit_repro.hip shows it with 20 lines and no other library) -- every profile of
    // round 2 ended in SIGSEGV for this reason.  When the grid does not fit -- compute units masked off, a smaller part -- the
    // context leaves this route for good and the caller's entry point goes on with the per-step kernels (nothing of the state
    // has been touched yet).
    const char* refuse = getenv("VJF_DEBUG_REFUSE_COOP");                  // (test hook)
    const bool full = m.n_rls > 0;                                         // (else: trial and SGD roles only, vjf_mega_lite_kernel)
    const int per_cu = full ? c->mega_wg_per_cu : c->lite_wg_per_cu;
    if ((refuse && atoi(refuse)) || per_cu < 1 || grid > per_cu * c->ncu) {
        c->mega_ok = false;
        return kMegaRefused;
    }
    { const char* ab = getenv("VJF_DEBUG_ABSENT"); A.alive_extra = ab ? atoi(ab) : 0; }   // (test hook: the grid waits for workgroups that never come)
    DevShared* d = dev_shared(c->cfg.device);
    if (d) A.host_word = d->mirror_d ? d->mirror_d + VJF_MIRROR_SLOT(stw) : nullptr;
    // the chain of resident grids of this process and device (DevShared): behind the previous one's completion, whichever context's
    std::unique_lock<std::mutex> chain;
    hipEvent_t done = nullptr;
    if (d && d->chained) {
        chain = std::unique_lock<std::mutex>(d->mu);
        if (d->last_valid && d->last_stream != c->stream) VJF_HIP(hipStreamWaitEvent(c->stream, d->last, 0));
        done = d->last;
    }
    if (full) with_mega_kernel(c->act, [&](auto kernel, auto... tail) {
        VJF_LAUNCH(kernel, dim3(grid), dim3(VJF_MG_THREADS), kMegaLds, c->stream, done, P, A, C, Q, tail...);
    });
    else with_lite_kernel(c->act, [&](auto kernel, auto... tail) {
        VJF_LAUNCH(kernel, dim3(grid), dim3(VJF_MG_THREADS), kMegaLds, c->stream, done, P, A, tail...);
    });
    const hipError_t le = hipGetLastError();
    if (done && le == hipSuccess) { d->last_stream = c->stream; d->last_valid = true; }
    c->on_mega = true;
    if (le == hipErrorLaunchOutOfResources) {
        c->mega_ok = false;
        return kMegaRefused;
    }
    if (le == hipSuccess) ++c->mega_launches;
    VJF_HIP(le);
    return 0;
}

// ---- the three-stream route (trials sharded over ranks, RCCL communicators in the context).  Step t's work splits into
//   chain A (caller's stream): K1 backward half(t) -> gradient Gram -> [all-reduce] -> clip + SGD -> K1 forward half(t+1)
//   chain B (second stream):   [gate: forward half(t)] E^T E Gram(t) -> [all-reduce] -> [gate: RLS(t-1)] P += G/v, g -> the RLS
//                              update of step t as ONE launch (Cholesky workgroup, y / W workgroup, inverse workgroups)
// K1's backward half(t+1) needs W, w_chol, sigma of step t, nothing else on chain A does; chain B(t+1) needs only the forward
// half's rows.  So a step costs max(A, B) instead of A + B.  Every kernel that waits in-kernel (the gates, the backward half,
// the y / W and inverse workgroups) waits for work that the host enqueued BEFORE it: whatever hardware queues the streams share,
// the producers are dispatched first and run to completion.  Results are those of the one-stream order bit for bit (same
// kernels, same sums).  RLS statistics alternate between two reduce buffers.
int filter_seq_streams(vjf_ctx* c, int32_t T, const SeqView& s, uint32_t flags) {
    int rc = ensure_stream2(c);
    if (rc) return rc;
    c->on_mega = false;
    const VjfPlan& P = c->plan;
    const int32_t B = s.B;
    hipStream_t sa = c->stream, sb = c->stream2, sc = c->stream3;
    float* redg = c->red();                             // gradients + loss sums (chain A)
    float* rede[2] = {c->red_rls(0), c->red_rls(1)};   // RLS statistics of even / odd steps (chain B)
    const int Bt = B * c->world * c->fake_world;                           // trials of all ranks
    const bool exact = (flags & VJF_FLAG_EXACT_NONFINITE) && (flags & VJF_FLAG_SGD) && c->comm_a != nullptr;
    auto args = [&](int t) { return trial_args(c, s.step(t), flags, t & 1); };
    rc = check_step_args(c, s.step(0));
    if (rc) return rc;
    if (c->comm_a) {
        // The ranks enter the sequence together: kernels of this route wait in-kernel (bounded, seconds) for kernels that sit behind
        // an all-reduce, and an all-reduce waits for the slowest rank -- one that is late with this CALL by more than the bound
        // (data loading, a first call) must not run its peers' waits out.  One tiny all-reduce and a host synchronisation per
        // call; inside the sequence the per-step collectives keep the ranks in step.
        // (Both communicators: the first collective on one sets its channels up, which can take longer than the bound.)
        float* tok = (float*)c->flag_words() + kRankTokenWord;
        VJF_HIP(hipMemsetAsync(tok, 0, 8, sa));
        VJF_NCCL(nccl().all_reduce(tok, tok, 1, kNcclFloat, kNcclSum, c->comm_a, sa));
        VJF_HIP(hipStreamSynchronize(sa));
        if (c->comm_b) {
            VJF_NCCL(nccl().all_reduce(tok + 1, tok + 1, 1, kNcclFloat, kNcclSum, c->comm_b, sc));   // (comm_b lives on sc)
            VJF_HIP(hipStreamSynchronize(sc));
        }
    }
    rc = refresh_aux(c);
    if (rc) return rc;
    unsigned* fl = c->flag_words();
    float* stw = c->status_word();
    if ((rc = launch_trial(c, args(0), kForwardHalf, sa, TrialOpts().counted()))) return rc;   // prologue: forward half of step 0
    for (int t = 0; t < T; ++t) {
        // sb: RLS statistics of step t as soon as its forward half is done (a one-wavefront gate on the workgroup count: no
        //     cross-stream event inside the loop), then -- behind W, sigma of t-1 -- P += G/v, g, and the RLS update
        // sc: the statistics have a stream of their own -- they need the forward half of step t only, and sb is still inside the
        //     update of step t-1 when that is done (behind it they cost the chain sb a sixth of its step: 15 of 96 us)
        hipLaunchKernelGGL(vjf_gate_kernel, dim3(1), dim3(64), 0, sc, (const unsigned*)(fl + kFwdDoneWord), c->fwd_count, stw);
        // (the operand kernel of sb waits in-kernel for the statistics -- a cross-stream event costs 6-13 us on this stack: for the
        //  reduction's own workgroups on a single rank, for one more launch behind the sum over ranks otherwise)
        if ((rc = launch_gram(c, B, kGramStats, kScRls, rede[t & 1], sc, GramOpts().rows(t & 1).count_into(c->comm_b ? nullptr : fl + kStatsWord)))) return rc;
        if (c->comm_b) {
            if ((rc = all_reduce_sum(c, rede[t & 1] + P.red_G, (size_t)(P.red_len - P.red_G), c->comm_b, sc))) return rc;   // [G | FDX | sums]
            hipLaunchKernelGGL(vjf_count_kernel, dim3(1), dim3(64), 0, sc, fl + kStatsWord);
            ++c->stats_count;
        } else c->stats_count += (unsigned)(c->n_ejobs + 1);
        // sa: backward half(t) waits in-kernel for the RLS update of step t-1, behind the reloads of its forward half's rows
        if ((rc = launch_trial(c, args(t), kBackwardHalf, sa, TrialOpts().after_rls(t > 0 ? fl + kPostDoneWord : nullptr, c->post_count)))) return rc;
        if (t == 0) {
            // the inverse workgroups write only the block-upper half of w_chol (block-lower of w_pchol): the other halves are
            // cleared once per blob (VJF_SC_TRI_CLEAN), here behind the backward half that may still read a full w_chol
            hipLaunchKernelGGL(vjf_triclean_kernel, dim3(64), dim3(256), 0, sa, P, c->state);
            hipLaunchKernelGGL(vjf_triclean_done_kernel, dim3(1), dim3(1), 0, sa, P, c->state);
            VJF_HIP(hipGetLastError());
        }
        // (P += G/v and g behind W, sigma of step t-1: the update of t-1 precedes them in sb)
        if ((rc = launch_prep(c, Bt, flags, rede[t & 1], kPrepOperands, sb, PrepOpts().after(fl + kStatsWord, c->stats_count)))) return rc;
        if (exact) c->k1_count += (unsigned)trial_blocks(c, B);           // (the replayed backward half of this step reads W, w_chol, sigma too)
        if ((rc = launch_rls(c, Bt, flags, rede[t & 1], sb, kRlsOneGrid))) return rc;
        if ((rc = launch_gram(c, B, kGramGrads, kScAll & ~kScRls, redg, sa, GramOpts().rows(t & 1)))) return rc;
        // sum the gradients and the loss sums over ranks -- [grad | loss sums]: ONE collective
        if ((rc = all_reduce_sum(c, redg, (size_t)P.red_SCA + 4, c->comm_a, sa))) return rc;
        // (the scalar workgroup ends once the RLS workgroups of step t are resident: the next backward half spins on their results
        //  and must not take the CUs they need before they are placed)
        rc = launch_prep(c, Bt, flags, redg, kPrepSgd, sa, PrepOpts().loss(s.loss_at(t)).pass(exact ? kReplayFollows : kNoReplay)
                             .end_when_rls_resident(fl + kCholRunWord, c->epoch, fl + kPostStartedWord, c->start_count));
        if (rc) return rc;
        if (exact) {
            // VJF_FLAG_EXACT_NONFINITE: the verdict on the step's loss (the same on every rank: it is taken on the summed loss terms) is
            // in the flag block now.  The backward half again with the dropped components' seeds at zero, its gradient sums, their sum
            // over ranks, the SGD pass from them -- every launch returns at once on an ordinary step; the collective runs regardless.
            const VjfTrialArgs ar = replay_args(c, args(t));
            if ((rc = launch_trial(c, ar, kBackwardHalf, sa, TrialOpts().counted()))) return rc;
            if ((rc = launch_gram(c, B, kGramGrads, kScNone, redg, sa, GramOpts().rows(t & 1).only_if(ar.replay_mask)))) return rc;
            if ((rc = all_reduce_sum(c, redg, (size_t)P.red_SCA, c->comm_a, sa))) return rc;
            if ((rc = launch_prep(c, Bt, flags, redg, kPrepSgd, sa, PrepOpts().pass(kReplayedPass)))) return rc;
        }
        if (t + 1 < T && (rc = launch_trial(c, args(t + 1), kForwardHalf, sa, TrialOpts().counted()))) return rc;
    }
    VJF_HIP(hipEventRecord(c->ev_c, sb));
    VJF_HIP(hipStreamWaitEvent(sa, c->ev_c, 0));                           // join: the caller's stream sees the final state
    return 0;
}

// Plans whose RLS update is a sequence of launches (n_rbf beyond one compute unit's LDS: BASELINE config E has 1000 features, 33
// column launches a step), single rank, T > 1: the update of step t on a stream of its own beside the trial chain.  Nothing in it
// reads what the backward half of step t or the forward half of step t + 1 writes, and those read none of its results:
//   sa (the caller's stream):  [W, w_chol, sigma of t-1 there] predictive moments, losses, backward half(t) -> gradient sums ->
//                              clip + SGD (+ the replay of a step with a non-finite loss component) -> forward half(t+1)
//   sc:                        [forward half(t) there] G, Phi^T dx
//   sb:                        [G, Phi^T dx there; the update of t-1 done: stream order] P W, P + G/v -> the column launches -> y,
//                              [backward half(t) done: it read the previous W, w_chol, sigma] W, w_chol, w_pchol, P, state-noise update
// Cross-stream order through events only (recorded before the wait that names them, in host order); the rows of E alternate
// between two buffers (the update's residual Phi W reads step t's rows while step t + 1 writes its own), the statistics of the
// two chains have buffers of their own, Phi W of the residual too.  Same kernels, same arithmetic as the one-stream order.
int filter_seq_two(vjf_ctx* c, int32_t T, const SeqView& s, uint32_t flags) {
    int rc = ensure_stream2(c);
    if (rc) return rc;
    const int32_t B = s.B;
    hipStream_t sa = c->stream, sb = c->stream2;
    float* redg = c->red();
    float* rede[2] = {c->red_rls(0), c->red_rls(1)};
    auto args = [&](int t) { return trial_args(c, s.step(t), flags, t & 1); };
    rc = check_step_args(c, s.step(0));
    if (rc) return rc;
    const bool replay = (flags & VJF_FLAG_SGD) != 0;
    VJF_HIP(hipEventRecord(c->ev_s, sa));                                  // (sb: behind whatever the caller's stream holds already)
    VJF_HIP(hipStreamWaitEvent(sb, c->ev_s, 0));
    hipStream_t sc = c->stream3;                                            // (its first launch waits for an event of sa behind this point)
    if ((rc = refresh_aux(c, sa))) return rc;
    if ((rc = launch_trial(c, args(0), kForwardHalf, sa))) return rc;
    VJF_HIP(hipEventRecord(c->ev_f[0], sa));
    // VJF_DEBUG_TWO_TIMELINE=1 (diagnostic): timing events around the phases of every step, printed to stderr behind a synchronisation
    const bool tl = getenv("VJF_DEBUG_TWO_TIMELINE") != nullptr;
    enum { TL_A0, TL_A1, TL_A2, TL_A3, TL_G0, TL_G1, TL_R0, TL_R2, TL_N };
    std::vector<hipEvent_t> tle;
    auto mark = [&](int t, int k, hipStream_t st) -> int {
        if (!tl) return 0;
        VJF_HIP(hipEventRecord(tle[(size_t)t * TL_N + k], st));
        return 0;
    };
    if (tl) {
        tle.resize((size_t)T * TL_N + 1);
        for (auto& e : tle) VJF_HIP(hipEventCreate(&e));
        VJF_HIP(hipEventRecord(tle[(size_t)T * TL_N], sa));
    }
    for (int t = 0; t < T; ++t) {
        const int g = t & 1;
        const VjfTrialArgs ta = args(t);
        // (the statistics on a stream of their own: they need the forward half only, not the previous update, which sb may still be in)
        VJF_HIP(hipStreamWaitEvent(sc, c->ev_f[g], 0));
        if ((rc = mark(t, TL_G0, sc))) return rc;
        if ((rc = launch_gram(c, B, kGramStats, kScNone, rede[g], sc, GramOpts().rows(g)))) return rc;
        if ((rc = mark(t, TL_G1, sc))) return rc;
        VJF_HIP(hipEventRecord(c->ev_g[g], sc));
        VJF_HIP(hipStreamWaitEvent(sb, c->ev_g[g], 0));
        if (t > 0) VJF_HIP(hipStreamWaitEvent(sa, c->ev_r[g ^ 1], 0));
        if ((rc = mark(t, TL_A0, sa))) return rc;
        if ((rc = launch_trial(c, ta, kBackwardHalf, sa))) return rc;
        if ((rc = mark(t, TL_A1, sa))) return rc;
        if ((rc = launch_gram(c, B, kGramGrads, kScAll, redg, sa, GramOpts().rows(g)))) return rc;
        if ((rc = launch_prep(c, B, flags, redg, kPrepSgd, sa, PrepOpts().loss(s.loss_at(t)).pass(replay ? kReplayFollows : kNoReplay)))) return rc;
        if (replay && (rc = launch_replay(c, ta, B, flags, sa, g))) return rc;
        VJF_HIP(hipEventRecord(c->ev_b[g], sa));
        if ((rc = mark(t, TL_A2, sa))) return rc;
        if (t + 1 < T) {                                                   // (enqueued before the update's ~40 launches: the host must not
            if (c->mfma_trial && (rc = refresh_aux(c, sa))) return rc;    //  hold the trial chain back; this route's SGD pass does not keep
            if ((rc = launch_trial(c, args(t + 1), kForwardHalf, sa))) return rc;    //  the transposed copies)
            VJF_HIP(hipEventRecord(c->ev_f[g ^ 1], sa));
        }
        if ((rc = mark(t, TL_A3, sa))) return rc;
        if ((rc = mark(t, TL_R0, sb))) return rc;
        if ((rc = launch_rlsb(c, B, flags, rede[g], sb, RlsbOpts().all_trials(&ta).beside_trial_chain(c->ev_b[g], c->resid())))) return rc;
        if ((rc = mark(t, TL_R2, sb))) return rc;
        VJF_HIP(hipEventRecord(c->ev_r[g], sb));
    }
    VJF_HIP(hipEventRecord(c->ev_c, sb));
    VJF_HIP(hipStreamWaitEvent(sa, c->ev_c, 0));                           // join: the caller's stream sees the final state
    if (tl) {
        VJF_HIP(hipStreamSynchronize(sa));
        static const char* nm[TL_N] = {"sa part2 starts", "sa part2 done", "sa sgd(+replay) done", "sa part1(t+1) done", "sc stats start", "sc stats done",
                                       "sb update starts", "sb update done"};
        for (int t = 0; t < T; ++t)
            for (int k = 0; k < TL_N; ++k) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, tle[(size_t)T * TL_N], tle[(size_t)t * TL_N + k]) == hipSuccess)
                    fprintf(stderr, "two-timeline %10.1f us  [%d] %s\n", ms * 1e3, t, nm[k]);
            }
        for (auto& e : tle) (void)hipEventDestroy(e);
    }
    return 0;
}

// ---- the route of a call.  One decision for vjf_route (what it reports), vjf_filter_seq and vjf_filter_step (what runs); the
//      values are those of vjf_route (include/vjf_hip.h).  In this order, the first row that holds:
//   kRoutePacked   communicators and collectives == 1: any flags, any T (ONE sum over ranks per step)
//   kRouteMega     single rank, overlap, no forced streams, the plan and the device fit the one-launch grid (mega_ok), stamps off (or
//                  kept beside the overlap), any T.  Flags: sgd + update is the training step (model.py:206-216); warm-up and
//                  update=False drop the RLS, Gram and operand roles (vjf_mega_lite_kernel, when it can be resident); sgd=False the
//                  backward pass and the gradient steps; update without sgd and without warm-up is NOT served.  A grid that turns out
//                  not to be resident makes the context leave the route for good (kMegaRefused): the rest runs per step
//   kRouteStreams  T > 1, communicators or forced streams, overlap, update without warm-up, fast Cholesky + post kernels +
//                  matrix-core trial kernel, stamps off (or kept beside the overlap)
//   kRouteTwo      T > 1, single rank, overlap, update without warm-up, stamps off, the multi-launch RLS plans (n_rbf beyond one
//                  compute unit's LDS): their update on a second stream beside the trial chain (filter_seq_two)
//   kRoutePerStep  everything else; with ranks (world > 1) vjf_filter_seq has no such route and fails with -24
// vjf_route has no T: it reports the route of a sequence (T > 1).  vjf_filter_step asks with T = 1: kRouteMega, or the step per step.
enum Route { kRoutePerStep = 0, kRouteMega = 1, kRouteTwo = 2, kRouteStreams = 3, kRoutePacked = 4 };
constexpr int kRouteOfASequence = 2;                       // the T vjf_route asks with

Route pick_route(const vjf_ctx* c, uint32_t flags, int T) {
    const bool rls = (flags & (VJF_FLAG_UPDATE | VJF_FLAG_WARM_UP)) == VJF_FLAG_UPDATE;
    const bool stamps_allow = !c->stamps || c->stamps_keep_overlap;
    if (c->comm_a && c->collectives == 1) return kRoutePacked;
    if (c->mega_ok && c->overlap && !c->comm_a && !c->force_streams && stamps_allow && (rls ? (flags & VJF_FLAG_SGD) != 0 : c->lite_wg_per_cu >= 1))
        return kRouteMega;
    const bool streams = (c->comm_a || c->force_streams) && c->overlap && (flags & VJF_FLAG_UPDATE) && !(flags & VJF_FLAG_WARM_UP) &&
                         c->fast_chol && c->post_kernels && c->mfma_trial && stamps_allow;
    if (streams && T > 1) return kRouteStreams;
    const bool two = c->overlap && !c->comm_a && c->world == 1 && !c->fast_chol && c->plan.n > 32 * VJF_CHOL_MAXBLK && !c->stamps && rls;
    return two && T > 1 ? kRouteTwo : kRoutePerStep;
}
int seq_chunk() {
    // Long sequences go in chunks: the workgroups of one launch stay resident for its whole length, and a compute kernel that
    // stays on the device for a minute is what drivers' lockup timers are for (16384 steps ~ 1 s at config B).
    const char* ce = getenv("VJF_SEQ_CHUNK");                              // (tests)
    return ce && atoi(ce) >= 1 ? atoi(ce) : 16384;
}
}  // namespace
