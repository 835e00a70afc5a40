// mlt_guards.cpp -- the parity guards of the host runtime (include/mltcnn.h: flat guard, decision guard, magnitude guard).
#include "mlt_runtime.h"

// ---- parity guards ---------------------------------
// A guarded pass: [flat_stat_kernel] -> fast network, whose heads kernel ends with the selection (an unordered list of the flagged CUs + their count) -> 4-byte D2H
// of the count.  Which CUs are flagged is decided by ONE device function (mlt_tail_kernels.inc: guard_rule) under the size's GuardRule (guard_thresholds).  The
// pass itself has three forms: run_selecting -- batches (run_fast_async) and QP sweeps (run_checked_sweep) on their slot's counter pair; mlt_predict's one CU, whose
// result copy carries the count (g.single); and MLT_GUARD_SELECT_KERNEL, the selection as guard_select_kernel, a launch of its own (ascending list) -- the A/B
// form.  Once the host knows the count k (check_flagged_count) it enqueues, for k > 0: gather of the flagged CUs' planes (gather_flagged) -> exact network on k
// CUs -> scatter of their results over the fast ones (sweeps: the exact pass's heads step writes them in place).

int guard_slot(mlt_ctx *ctx, int which, int n, int nl, GuardSlot *g) {
  Lay::GuardLay &lay = ctx->guard_lay;
  if ((size_t)n > lay.n || (size_t)nl > lay.nl) lay = Lay::GuardLay(std::max((size_t)n, lay.n), std::max((size_t)nl, lay.nl));
  int rc;
  if ((rc = ctx->guard_dev.reserve(ctx, 2 * lay.bytes(), "guard slots", true))) return rc;   // (the selection's counters must start at zero)
  if (!ctx->guard_host) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->guard_host, 64, hipHostMallocDefault));
  *g = GuardSlot{lay.at(ctx->guard_dev.p + (size_t)which * lay.bytes()), &ctx->guard_phase[which], ctx->guard_host + which};
  return MLT_OK;
}

namespace {

// the thresholds of the size's guards: what the selection compares against
GuardRule guard_thresholds(const mlt_ctx *ctx, const SizeState &st) {
  const int quads = st.size * st.size / 4;
  GuardRule r{};
  r.flat_thr = quads / st.flat_div;  // >= 1/8 (tiers behind the magnitude guard, exact-lite tier: 1/16) of the quads exactly flat (constant / exactly linear in both planes)
  r.near_thr = quads / 2;            // or >= 1/2 of them near-flat (mlt_kernels.h: MLT_FLAT_RANGE)
  r.margin = st.margin_guard ? st.guard_margin : 0.f;
  r.mag_thr = st.mag_thr;
  r.conf_band = st.conf_band(ctx->tolerance);
  r.cand_band = st.cand_band(ctx->tolerance);
  return r;
}

// The size's main arithmetic on n CUs with the selection as the tail of its heads kernel, on the slot's counter pair: an unordered list of the flagged CUs through
// an atomic append on a counter that is zero on entry; the launch zeroes the slot's OTHER counter for the next one (whose predecessor's count has left the device
// by then: same stream).  Then the 4-byte copy of the count to g.h_count.  (A first version counted finished workgroups to let the last one publish and re-arm a
// single counter: 4096 same-address atomics and release fences made the heads launch 0.123 ms instead of 0.030 -- more than the selection launch it saved.)
int run_selecting(mlt_ctx *ctx, SizeState &st, int n, const PassIO &io, const GuardSlot &g) {
  const GuardTail tail{guard_thresholds(ctx, st), g.d.count + *g.phase, g.d.idx, st.flat_guard ? g.d.flat : nullptr, g.d.count + (*g.phase ^ 1)};
  GuardOut go;
  go.d_flat = tail.flat; go.tail = &tail;
  if (const int rc = run_network(ctx, st, st.main_cfg(), n, io, go)) {
    // a pass that failed (e.g. no memory for the workspace of an oversized batch -- the caller may come back with a smaller one) may or may not have run its heads
    // kernel: both counters back to zero, the phase stays -- whichever counter the next launch counts on is zero on entry
    (void)hipMemsetAsync(g.d.count, 0, 8, ctx->stream);
    return rc;
  }
  *g.phase ^= 1;
  HIP_TRY(ctx, hipMemcpyAsync(g.h_count, tail.count, 4, hipMemcpyDeviceToHost, ctx->stream));
  return MLT_OK;
}

// The k flagged CUs idx[0 .. k) of a pass, out of its planes into the dense staging set gs, their poc and qp beside them.
int gather_flagged(mlt_ctx *ctx, int S, const Planes &pl, const int32_t *poc, const int32_t *qp, const int32_t *idx, int k, const StageSet::Ptrs &gs) {
  GuardGatherArgs ga{};
  pl.fill(ga);
  ga.poc = poc; ga.qp = qp; ga.idx = idx; ga.k = k; ga.s_l = ilog2(S);
  ga.g_org = gs.d_org; ga.g_pred = gs.d_pred; ga.g_poc = gs.d_poc; ga.g_qp = gs.d_qp;
  HIP_TRY(ctx, mlt_launch_guard_gather(ga, ctx->stream));
  return MLT_OK;
}

}  // namespace

// The size's main arithmetic on n CUs with whatever guards the size has, everything asynchronous on ctx->stream.  With guards (g: the batch's slot, unused
// without) the selection of the flagged CUs runs too and their count lands in g.h_count (pinned) -- valid after the stream has been synchronised; the
// caller then re-evaluates them with guard_fixup_async.  io.logits may be NULL.
int run_fast_async(mlt_ctx *ctx, SizeState &st, int n, const PassIO &io, const GuardSlot &g) {
  if (!st.guards()) return run_network(ctx, st, st.main_cfg(), n, io);
  int rc;
  PassIO fast = io;
  if (!fast.logits && st.margin_guard) fast.logits = g.d.lg;
  GuardOut go;
  go.d_flat = st.flat_guard ? g.d.flat : nullptr;
  if (g.single && n == 1) {
    // one CU (mlt_predict's captured graph): the selection is a tail of the heads kernel -- no guard_select launch, no memset of the
    // statistic (the tail clears it for the next call; it is only consumed when the first kernel is the one that produces it: aligned planes,
    // S >= 64 -- else flat_stat_kernel overwrites it), no separate copy of the count (the caller's result copy carries it)
    const GuardTail tail{guard_thresholds(ctx, st), g.d.count, g.d.idx, go.d_flat, nullptr};
    go.tail = &tail; go.flat_is_clear = true;
    return run_network(ctx, st, st.main_cfg(), 1, fast, go);
  }
  if (!ctx->guard_select_kernel && g.phase) return run_selecting(ctx, st, n, fast, g);   // (one launch and one launch gap less per step than a selection launch)
  go.d_mag = st.mag_thr > 0.f ? g.d.mag : nullptr;
  if ((rc = run_network(ctx, st, st.main_cfg(), n, fast, go))) return rc;
  GuardSelectArgs sa{};
  sa.rule = guard_thresholds(ctx, st);
  sa.mag = go.d_mag;
  sa.flat = go.d_flat;
  sa.logits = st.margin_guard ? fast.logits : nullptr;
  sa.idx = g.d.idx; sa.count = g.d.count; sa.n = n; sa.n_logits = st.model.n_logits;
  sa.head_off = st.head_off(); sa.head_classes = st.head_classes();
  sa.min_conf = st.min_conf; sa.cand_cov = st.cand_cov; sa.cand_max = st.cand_max;
  Launch L{ctx};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if ((rc = L.prof_begin("guard_select", 0.0, 0.0, e0, e1))) return rc;
  LAUNCH_TRY(ctx, mlt_launch_guard_select(sa, ctx->stream));
  if ((rc = L.prof_end(e1))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(g.h_count, g.d.count, 4, hipMemcpyDeviceToHost, ctx->stream));
  return MLT_OK;
}

// k > 0 flagged CUs (g.d.idx) of a batch whose fast results are in io.split / io.logits / io.dec / io.cand: exact re-evaluation, asynchronous.
int guard_fixup_async(mlt_ctx *ctx, SizeState &st, int k, const PassIO &io, const GuardSlot &g) {
  const int S = st.size, nl = st.model.n_logits;
  const StageSet lay(S, k, nl, io.dec != nullptr, io.cand != nullptr);
  int rc = ctx->gstage.reserve(ctx, lay.bytes(), "guard staging");
  if (rc) return rc;
  const StageSet::Ptrs gs = lay.at(ctx->gstage.p);
  if ((rc = gather_flagged(ctx, S, io.pl, io.poc, io.qp, g.d.idx, k, gs))) return rc;
  // (the re-run's heads kernel applies the size's confidence gate to the gathered split modes and fills the flagged CUs' records -- decision and candidate -- from the exact logits)
  rc = run_network(ctx, st, st.exact_cfg(), k, PassIO{Planes::dense(gs.d_org, gs.d_pred, S), gs.d_poc, gs.d_qp, gs.d_split, gs.d_lg, gs.d_dec, gs.d_cand});
  if (rc) return rc;
  GuardScatterArgs sc{};
  sc.g_dec = gs.d_dec; sc.dec = io.dec;
  sc.g_cand = gs.d_cand; sc.cand = io.cand;
  sc.idx = g.d.idx; sc.g_split = gs.d_split; sc.g_logits = gs.d_lg; sc.split = io.split; sc.logits = io.logits; sc.k = k; sc.n_logits = nl;
  HIP_TRY(ctx, mlt_launch_guard_scatter(sc, ctx->stream));
  st.reruns += (uint64_t)k;
  return MLT_OK;
}

namespace {

// Blocks until the 4-byte count of a guarded pass on n CUs, whose copy is the last thing enqueued on ctx->stream, has landed (run_checked, run_checked_sweep).
int wait_count(mlt_ctx *ctx, SizeState &st, int n) {
  // Wait for the 4-byte count.  Default: SLEEP for most of the time the batch is expected to take (a running estimate per CU of this
  // size, learnt from the previous calls), then poll the event for the rest: the host core is idle for all but the last ~0.2 ms of a
  // 5 ms batch -- in the encoder host cores are the scarce resource -- and the caller's next batch is still enqueued the moment this one
  // is through (a plain blocking wait wakes up on an interrupt and left the GPU idle for ~0.14 ms per 4096-CU step, 2.8 %).
  // MLT_GUARD_SPIN_WAIT=1: poll from the start (one busy core); MLT_GUARD_BLOCKING_WAIT=1: hipEventSynchronize on a blocking-sync event.
  const int wait_mode = tuning().guard_wait_mode;
  if (!ctx->ev_guard) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_guard, hipEventDisableTiming | hipEventBlockingSync));
  HIP_TRY(ctx, hipEventRecord(ctx->ev_guard, ctx->stream));
  if (wait_mode == 2) HIP_TRY(ctx, hipEventSynchronize(ctx->ev_guard));
  else {
    const auto t0 = std::chrono::steady_clock::now();
    // Only chunks of >= 512 CUs are worth sleeping for (shorter ones are through in well under a millisecond: poll), and only on an
    // estimate measured on a chunk of the same power-of-two bucket, scaled by the ratio of the sizes.
    int b = 0;
    while (b < 15 && (2 << b) <= n) ++b;
    const double expect_us = (n >= 512 && st.guard_n[b] > 0) ? st.guard_us[b] * (double)n / (double)st.guard_n[b] : 0.0;
    const bool slept = wait_mode == 0 && expect_us > 400.0;
    if (slept) std::this_thread::sleep_for(std::chrono::microseconds((long)(expect_us - 250.0)));
    hipError_t e = hipEventQuery(ctx->ev_guard);
    const bool overslept = slept && e != hipErrorNotReady;  // through already on waking up: the true duration is unknown, only "shorter"
    while (e == hipErrorNotReady) {
#if defined(__x86_64__)
      for (int i = 0; i < 32; ++i) __builtin_ia32_pause();
#endif
      e = hipEventQuery(ctx->ev_guard);
    }
    HIP_TRY(ctx, e);
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    // The estimate must never stay above the truth (oversleeping costs GPU time, polling only host time): a wake-up that found the batch
    // finished FORGETS the bucket's estimate -- the next chunk of that size is polled from the start and measured exactly -- and a
    // measured duration (we polled, so `us` is exact) replaces the estimate at once when it is shorter, half-way when it is longer.
    if (overslept) { st.guard_n[b] = 0; st.guard_us[b] = 0.0; }
    else if (n >= 512) {
      const double scaled = st.guard_n[b] > 0 ? st.guard_us[b] * (double)n / (double)st.guard_n[b] : 0.0;
      st.guard_us[b] = (st.guard_n[b] == 0 || us < scaled) ? us : 0.5 * (scaled + us);
      st.guard_n[b] = n;
    }
  }
  return MLT_OK;
}

}  // namespace

// network for n CUs with whatever guards the size has; synchronises once when guards are on (see mlt_predict_batch_device).
int run_checked(mlt_ctx *ctx, SizeState &st, int n, const PassIO &io) {
  const bool guards = st.guards();
  GuardSlot g;
  int rc;
  if (guards && (rc = guard_slot(ctx, 0, n, st.model.n_logits, &g))) return rc;
  if ((rc = run_fast_async(ctx, st, n, io, g)) || !guards) return rc;
  if ((rc = wait_count(ctx, st, n))) return rc;
  const int k = *g.h_count;
  if ((rc = check_flagged_count(ctx, k, n))) return rc;
  return k ? guard_fixup_async(ctx, st, k, io, g) : MLT_OK;
}


// QP sweep (io.sweep: qps, n_qps, slab): ONE pass of the size's main arithmetic whose heads step evaluates every point, the selection as that kernel's tail (per CU
// a mask of the points it is flagged under; MLT_GUARD_SELECT_KERNEL does not apply), the 4-byte count of the CUs flagged under ANY point, then -- for k > 0 -- the
// gather of that union and ONE exact pass on its k CUs, whose heads step writes each CU's exact results into the slabs of its mask only: no scatter launch.
// Sizes without guards run the sweep heads and nothing else.  guard_reruns counts the union: what ran.
int run_checked_sweep(mlt_ctx *ctx, SizeState &st, int n, const PassIO &io) {
  if (!st.guards()) return run_network(ctx, st, st.main_cfg(), n, io);
  Lay::SweepGuardLay &lay = ctx->sweep_guard_lay;
  if ((size_t)n > lay.n) lay = Lay::SweepGuardLay((size_t)n);
  int rc;
  if ((rc = ctx->sweep_guard_dev.reserve(ctx, lay.bytes(), "sweep guard slot", true))) return rc;   // (the counters must start at zero)
  if (!ctx->guard_host) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->guard_host, 64, hipHostMallocDefault));
  const GuardSlot g{lay.at(ctx->sweep_guard_dev.p), &ctx->sweep_phase, ctx->guard_host + 2};   // the sweep's one slot ...
  uint32_t *d_mask = lay.mask.in<uint32_t>(ctx->sweep_guard_dev.p);                             // ... and, beside it, the CUs' masks
  PassIO fast = io;
  fast.sweep.idx = nullptr; fast.sweep.mask = d_mask;
  if ((rc = run_selecting(ctx, st, n, fast, g)) || (rc = wait_count(ctx, st, n))) return rc;
  const int k = *g.h_count;
  if ((rc = check_flagged_count(ctx, k, n)) || !k) return rc;
  const int S = st.size;
  const StageSet gl(S, k, st.model.n_logits, false, false);
  if ((rc = ctx->gstage.reserve(ctx, gl.bytes(), "guard staging"))) return rc;
  const StageSet::Ptrs gs = gl.at(ctx->gstage.p);
  // (the CUs' qp offsets follow them into the re-run; without offsets the column is a copy of poc and is not read)
  if ((rc = gather_flagged(ctx, S, io.pl, io.poc, io.qp ? io.qp : io.poc, g.d.idx, k, gs))) return rc;
  PassIO exact = io;   // the caller's outputs: the heads step writes row idx[j] of the slabs in mask[idx[j]]
  exact.pl = Planes::dense(gs.d_org, gs.d_pred, S); exact.poc = gs.d_poc; exact.qp = io.qp ? gs.d_qp : nullptr;
  exact.sweep.idx = g.d.idx; exact.sweep.mask = d_mask;
  if ((rc = run_network(ctx, st, st.exact_cfg(), k, exact))) return rc;
  st.reruns += (uint64_t)k;
  return MLT_OK;
}
