// mlt_runtime.h -- internal declarations of the host runtime, shared by its translation units (include/mltcnn.h is the ABI; nothing here is exported):
//   mlt_dispatch.cpp   tuning switches, workspace, the run_* launch wrappers, plan_network / run_network, mlt_plan_describe
//   mlt_guards.cpp     the parity guards: selection slots, the fast pass with the size's guards, the exact re-run of flagged CUs
//   mlt_calibrate.cpp  model upload, calibration sets and session, the loader, mlt_load_weights / mlt_calibrate / mlt_arithmetic
//   mlt_api.cpp        init / shutdown / stream, the predict entry points, deferred prediction, confidence gate, profile
//   mlt_pictures.cpp   device-resident pictures: create / upload / wrap / destroy, mlt_predict_at, mlt_grid_positions
//   mlt_tree.cpp       partition trees of a picture: mlt_predict_tree, mlt_predict_trees, mlt_predict_tree_sweep, mlt_predict_trees_sweep, mlt_tree_roots, mlt_tree_max_nodes
//   mlt_motion.cpp     prediction pictures: mlt_motion_blocks, mlt_picture_download, mlt_picture_compensate, mlt_picture_predict and their _refs forms
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mltcnn.h"
#include "mlt_kernels.h"
#include "mlt_layout.h"
#include "mlt_model.h"
#include "mlt_tier_search.h"

// Every environment switch of the library except MLT_CALIB_VERBOSE is a tuning / test knob (A/B runs, sweeps, fallback paths): they are
// honoured only when MLT_TUNING=1 is set as well, so that an encoder process cannot change kernel selection, chunking or wait modes by
// an accident of its environment.
const char *tuning_env(const char *name);

// Every tuning switch of the dispatcher and of the load path, parsed ONCE on first use (round 6, VERDICT r5 item 7: round 5 read them through some thirty
// function-local statics scattered over the run_* functions).  All of them need MLT_TUNING=1 (tuning_env).
struct Tuning {
  const char *debug_dump_dir;      // MLT_DEBUG_DUMP_DIR: after every kernel, synchronise and write its output tensor there (bring-up only)
  int xl_kill, xl_kill_layer;      // MLT_XL_KILL / MLT_XL_KILL_LAYER: exact-lite bring-up, silence a K block (of one layer: cin * 1000 + cout)
  long lat_pixels;                 // MLT_LAT_PIXELS: launches of at most this many output pixels take the latency variants / per-conv forms (16384; 0 disables)
  bool no_exact_lat;               // MLT_NO_EXACT_LAT
  bool exact_patch_big;            // (MLT_EXACT_PATCH_64K clears it) the exact arithmetic's patch planes may use what the weight ring leaves of the LDS
  int wg_cap, wg_cap0, wg_cap1, wg_cap2;   // MLT_WG_CAP / _CAP0 / _CAP1 / _CAP2: persistent workgroups per launch (256 = one per CU)
  bool l0_mfma32, l1_mfma32;       // MLT_L0_MFMA32: layer0_stream_kernel on round 5's 32x32x16 MFMAs; layer1_stream_kernel runs them unless MLT_L1_MFMA16 (same bits either way)
  bool no_chain, no_chain_s2, no_c16, chain64, no_block_fusion, no_l0_s5;   // MLT_NO_CHAIN, _CHAIN_S2, _C16, _CHAIN64, _BLOCK_FUSION, _L0_S5: knock-outs of the fused forms
  bool no_xs_handoff;              // MLT_NO_XS_HANDOFF (also set by MLT_DEBUG_DUMP_DIR): the streaming pair hands over layer1's shortcut (sc) instead of its input (xs); A/B, same bits
  bool no_stage256_wide;           // MLT_NO_STAGE256_WIDE: the whole 256-channel stage runs chain_kernel (one cout pass at a time) instead of stage256_wide_kernel; A/B, same bits
  int l0_stream_min, l1_stream_min;        // MLT_L0_STREAM_MIN / MLT_L1_STREAM_MIN (128; MLT_NO_L0_STREAM / MLT_NO_L1_STREAM: 0 = never)
  int guard_wait_mode;             // 0 sleep-then-poll, 1 MLT_GUARD_SPIN_WAIT, 2 MLT_GUARD_BLOCKING_WAIT
  bool no_small_mix, no_mag_guard, no_graph;   // MLT_NO_SMALL_MIX, MLT_NO_MAG_GUARD, MLT_NO_GRAPH (also set by MLT_DEBUG_DUMP_DIR)
};
const Tuning &tuning();

inline int size_index(int size) {
  switch (size) {
    case 128: return 0;
    case 64: return 1;
    case 32: return 2;
    case 16: return 3;
    default: return -1;
  }
}
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// ---- launch plans (round 6) ----
// WHAT a batch launches is decided once per (size, tier, batch class, alignment) -- plan_network, a pure function of the models' packing, the tier's
// launch-unit masks and a handful of booleans derived from n and the planes' alignment -- and cached in the size's state; the hot path (run_network)
// binds the workspace and walks the list.  mlt_plan_describe shows the walk on the CPU (tests/test_launch_plan_cpu.py, scripts/plan_matrix.py).
struct NetCfg {   // the arithmetic of a pass: every launch unit takes its weights from one of up to three models
  int S = 0;
  mlt::Model *m = nullptr, *mback = nullptr, *mx = nullptr;   // main | hi+lo weights for the units of back_mask | exact for the units of x_units
  unsigned back_mask = 0, x_units = 0;
  mlt::Model &model_of(int s, int u) const { return ((x_units >> (2 * s + u)) & 1u) ? *mx : (mback && ((back_mask >> (2 * s + u)) & 1u)) ? *mback : *m; }
  int h_in(int s) const { int h = S; for (int i = 0; i < s; ++i) h = h / 2 > 0 ? h / 2 : 1; return h; }   // map side at the input of stage s
};

// One launch of a size's plan (built by plan_network, walked by run_network: mlt_dispatch.cpp): the kind says which buffers it reads and writes.
struct PlanStep {
  enum Kind : uint8_t {
    FLAT_STAT,      // the flat-content statistic as a launch of its own (the first kernel does not read the raw planes as aligned quads)
    LAYER0_STREAM,  // all of layer0 (front: + layer1.0.conv1 + shortcut) from the raw planes          -> out[0] | t = pool0, sc = pool1 (chunk-major; xs: its input)
    STEM_BLOCK,     // layer0.0 from the raw planes                                                      -> b0 = pool2
    STEM5,          // composed first layer: t, sc of layer0.0                                           -> pool0, pool1
    CONV_S2,        // stride-2 conv + shortcut that open stage s: stage input                           -> t = pool0, sc = pool1
    CHAIN,          // rest of stage s (inside_s2: all of it, from the stage input) in one launch        -> out[s] (+ GAP)
    LAYER1_STREAM,  // the three stride-1 convs of the 64-channel stage, streaming form                   -> out[1] (+ GAP)
    CONV_B0C2,      // block 0, conv2 + shortcut + ReLU: pool0, pool1                                     -> b0 = pool2
    BLOCK32,        // layer0.1 in one kernel: pool2                                                      -> out[0]
    CONV_B1C1,      // block 1, conv1: pool2                                                              -> pool3
    CONV_B1C2,      // block 1, conv2 + b0 + ReLU: pool3, pool2                                           -> out[s] (+ GAP)
    HEADS
  } kind;
  int8_t s = 0;             // stage
  bool front = false;       // LAYER0_STREAM: layer1.0.conv1 + shortcut ride along
  bool xs = false;          // LAYER0_STREAM (front) + the LAYER1_STREAM behind it: pool1 carries the shortcut's INPUT (xs), layer1's launch computes the shortcut
  bool inside_s2 = false;   // CHAIN: the stage's stride-2 conv + shortcut run inside the launch
  bool wide = false;        // CHAIN (inside_s2, 256 channels): stage256_wide_kernel -- both cout passes per wave, every input patch staged once
  bool x_c16 = false;       // CHAIN (inside_s2): the stage input is chunk-major
  bool sc_c16 = false;      // CONV_S2 writes / CHAIN, LAYER1_STREAM read the shortcut chunk-major
  bool y_c16 = false;       // the stage's output is written chunk-major (its consumer is a whole-stage launch)
};
using NetPlan = std::vector<PlanStep>;
using PlanKey = std::tuple<const void *, const void *, const void *, unsigned, unsigned, unsigned>;   // models (main, hi+lo weights, exact), their unit masks, batch class

struct SizeState {
  bool enabled = false, loaded = false;
  std::map<PlanKey, NetPlan> plans;   // launch plans of the loaded tier, by batch class (filled on first use; cleared by every (re)load)
  bool exact = false;          // arithmetic `model` runs (after calibration)
  bool w2 = false;             // middle tier: the main path runs `model_w2` (hi+lo weights on single fp16 activations, fused kernels); guards as for fast
  unsigned w2_mask = 0;        // ... in the stages whose bit is set (bit s = layer s; all four: the whole network); the other stages stay on the
                               // single-pass kernels of `model` ("mixed" tiers: the calibration picks the CHEAPEST set of stages that meets the contract)
  unsigned w2_units = 0;       // ... at the granularity the kernels allow: bit 2 s = the first launch unit of layer s (layer0.0 / the stride-2 conv + shortcut),
                               // bit 2 s + 1 = the second (layer0.1 / the three stride-1 convs); w2_mask = the stages with at least one unit set
  unsigned x_mask = 0;         // round 4, the tier below exact: the stages of this mask run the EXACT arithmetic (model_exact's per-conv kernels, a lo
                               // plane behind their activations), the other stages hi+lo weights (w2_mask = the complement) -- for weight sets whose
                               // ACTIVATION rounding, spread evenly over all 18 rounding sites, misses the contract by a few per cent
  unsigned x_units = 0;        // ... at launch-unit granularity (bit 2 s + u as in w2_units); x_mask = the stages with at least one exact unit
  bool lite = false;           // round 5: the calibration found no fp16 tier within the contract but the exact-lite arithmetic is: `model` is the exact-lite
                               // model (two activation planes, FP8 cross terms; mlt_model.h: xl), the flat guard is off (its error is 1/20 of the single
                               // pass's), the decision guard -- if configured -- still re-evaluates near-ties with `model_exact`
  bool cfg_flat_guard = false; // flat guard as configured (flags); flat_guard is what the loaded tier uses
  int flat_div = 8;            // the flat guard re-evaluates a CU when >= 1 / flat_div of its quads are EXACTLY flat.  8 for the fp16 tiers admitted by the plain rule; 16
                               // for a tier behind the magnitude guard (CalibSession::price_guarded) and for the exact-lite
                               // tier (round 6: its FP8 cross terms quantise a constant area's activations coherently -- 3-bit mantissas -- and a weight set with
                               // large logits turns a 10-12 % constant band into |dlogit| 1.0-1.5e-3: 4 of 331,776 probed logits of the second trained family,
                               // profiles/r06b_tail_probe_trained.txt; round 5 had switched the guard OFF for this tier on the strength of the seeded sets)
  float guard_margin = 3e-3f;  // decision guard's threshold for THIS size's tier: the context's (3 x tolerance, or as configured) -- except the exact-lite tier, whose
                               // largest calibration error is ~ 1/6 of the tolerance: 3 x 1.7 x calib_max there (1.7: the tail probes' largest error over the
                               // calibration set's), at least 1e-4, at most the context's
  bool want_exact = false;     // configured arithmetic (flags)
  bool flat_guard = false, margin_guard = false, calibrate = false;
  bool small_mix = false;      // 64 / 32 / 16 (round 4): configured exact, but the load-time calibration may keep the first stages -- the large maps, where the
                               // time is -- on the single-pass kernels (x_mask = the remaining stages); exact when no prefix meets the contract
  bool calibrated = false;
  // Round 6, the MAGNITUDE guard.  The fp16 pipeline's error is RELATIVE: it scales with the size of the feature-driven part of the logits,
  // M = max over logits of sum_k |w_ck gap_k| (heads_kernel).  A trained-like weight set amplifies what it was trained to see: on content far
  // outside its training range (a residual plane of hundreds of ten-bit steps: the synthetic calibration classes "uniform", "constant org /
  // pred", the bands) M is 20-80 x what texture or natural scenes give (tools/attribute_error.py, profiles/r06_attribution_*.txt) and so is
  // the absolute error -- the heavy tail that kept every fp16 tier of that family out.  mag_thr > 0: CUs whose M exceeds it
  // are re-evaluated with the exact arithmetic like the flat-content guard's; the threshold is where the tier's worst relative error
  // measured at load time (calib_rel, over EVERY calibration CU) reaches max_frac x tolerance.  0: off (every seeded weight set: their
  // error does not follow M, they are admitted -- or not -- by the plain rule as before).
  float mag_thr = 0.f, calib_rel = 0.f, mag_flag = 0.f;
  int mag_kind = 0;            // 0: no magnitude guard; 2: the tier was ADMITTED behind it (threshold from the admission rule, above); 1: RANGE guard -- a tier the plain rule
                               // admitted is still only validated on the magnitudes its calibration CUs had, and its error grows linearly with M: CUs beyond
                               // kMagRange x the largest calibrated magnitude are re-evaluated exactly (1.5 x the 0.65-of-tolerance the largest calibration error
                               // may reach = the tolerance).  Costs nothing on content inside the calibrated range; it is what stands between a tier and
                               // content it has never been priced on (scripts/r06_lite_range_probe.py: the exact-lite arithmetic forced onto activations
                               // beyond its e4m3 range is off by 2e-2)
  bool cfg_mag_guard = true;   // (MLT_FLAG_NO_MAGNITUDE_GUARD clears it)
  float calib_rms = 0.f, calib_max = 0.f;
  int calib_cus = 0, calib_caller_cus = 0;   // CUs the last calibration priced (after dropping those the flat guard re-evaluates anyway) / of them the caller's (mlt_calibrate)
  std::vector<char> blob;      // host copy of the MLTW blob the size was loaded from (mlt_calibrate re-packs from it)
  uint64_t reruns = 0;         // CUs re-evaluated by the guards
  // run_checked's sleep: measured duration (enqueue -> flagged-CU count on the host) of a guarded chunk, per power-of-two bucket of the chunk
  // size (a 4-CU tail costs ~50 us per CU, a 4096-CU chunk ~1.2: ONE per-CU figure for all sizes made a tail's measurement inflate the
  // next full chunk's sleep 20-fold); guard_n[b] = the chunk size guard_us[b] was measured on; 0: unknown -> poll
  double guard_us[16] = {0};
  int guard_n[16] = {0};
  int size = 0, head_index = 0;
  // the decision head inside a CU's logits: first logit, class count
  int head_off() const { int off = 0; for (int h = 0; h < head_index; ++h) off += model.heads[h].classes; return off; }
  int head_classes() const { return model.heads[head_index].classes; }
  float min_conf = 0.f;        // confidence gate (mlt_set_confidence_gate): split = -1 unless the decision head's softmax probability reaches it.  0: off.  Not a
                               // property of the weights: (re)loads and calibrations keep it
  // the gate guard's band (mlt_kernels.h: MLT_CONF_BAND_FRAC x the tolerance the tier was calibrated against); 0 unless gate and decision guard are both on
  float conf_band(float tolerance) const { return (min_conf > 0.f && margin_guard) ? MLT_CONF_BAND_FRAC * tolerance : 0.f; }
  // candidate policy (mlt_set_candidate_policy): the candidate record keeps the shortest rank prefix of the decision head that carries cand_cov of the softmax
  // probability, every class when that takes more than cand_max > 0.  (0, 0): the default -- the argmax alone.  Like min_conf it survives (re)loads and calibrations.
  float cand_cov = 0.f;
  int cand_max = 0;
  bool cand_used = false;      // a policy was set or a candidate call made on this size: deferred batches carry candidate records from then on
  bool cand_policy() const { return cand_cov > 0.f || cand_max > 0; }
  // the candidate guard's band (same width as the gate guard's); 0 unless a policy is set and the decision guard is on
  float cand_band(float tolerance) const { return (cand_policy() && margin_guard) ? MLT_CONF_BAND_FRAC * tolerance : 0.f; }
  mlt::Model model;
  mlt::Model model_exact;      // fast sizes: exact-arithmetic copy the guards re-evaluate flagged CUs with
  mlt::Model model_w2;         // hi+lo-weights copy on the fast tiling (MLT_MODEL_W2); built only when the single-pass calibration fails
  mlt::Model model_xl;         // exact-lite copy (MLT_MODEL_XLITE): exists only while the calibration prices it; the tier's model moves into `model`
  bool guards() const { return !exact && (flat_guard || margin_guard || mag_thr > 0.f) && model_exact.on_device; }
  // the size's main arithmetic: `model` (fast, or exact when that is the configured / calibrated arithmetic) -- with, for the hi+lo-weights tiers, `model_w2` in the
  // launch units of w2_units and, for the tiers below exact, `model_exact` in those of x_units (no model, no mask)
  NetCfg main_cfg() {
    NetCfg c;
    c.S = size; c.m = &model;
    if (w2) { c.mback = &model_w2; c.back_mask = w2_units; }
    if (x_units) { c.mx = &model_exact; c.x_units = x_units; }
    return c;
  }
  // the exact copy the guards re-evaluate flagged CUs with (and the calibration measures against)
  NetCfg exact_cfg() { NetCfg c; c.S = size; c.m = &model_exact; return c; }
};

// guard state of one in-flight pass -- a batch, a QP sweep, mlt_predict's one CU: any layout's guard fields on the device, {fields.at(base), phase, h_count[, single]}
struct GuardSlot {
  Lay::GuardFields::Ptrs d{};
  int *phase = nullptr;        // passes with the selection as the heads kernel's tail on a counter pair: d.count[*phase] is the launch's running count (zero on entry),
                               // d.count[*phase ^ 1] the one it zeroes for the NEXT launch of the slot; toggled per launch (mlt_guards.cpp: run_selecting).  NULL: no such pair
  int32_t *h_count = nullptr;  // pinned: where the count comes back
  bool single = false;         // mlt_predict's slot: one CU, d.flat zero on entry and cleared by the heads kernel (consume-and-clear), the
                               // selection rides on the heads kernel, and the caller's own result copy brings the count back
};
// the selection as the tail of a pass's heads kernel: the size's rule (mlt_kernels.h: GuardRule) and where the tail counts, lists and reads the flat statistic
// (HeadArgs.rule, g_count, g_idx, g_flat, g_next; next != NULL: a counter pair -- batches and sweeps)
struct GuardTail { GuardRule rule; int32_t *count, *idx, *flat, *next; };

using Lay::StageSet;

// A grow-only buffer of a context, device memory or (pinned) page-locked host memory: reserve() keeps the allocation when it is large enough, else synchronises
// the context's stream, frees and allocates anew (zero: cleared).  hipErrorOutOfMemory -> MLT_ERR_NOMEM; `what` opens the message.
struct GrowBuf {
  bool pinned = false;
  char *p = nullptr;
  size_t bytes = 0;
  int reserve(mlt_ctx *ctx, size_t want, const char *what, bool zero = false);
  void release() { if (p) (void)(pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; bytes = 0; }
};

// mlt_predict (one CU per call, the encoder's use): pinned host staging, one H2D, the kernel chain replayed from a
// hipGraph captured once per CU size and call kind, one D2H.
struct SingleCu {
  char *h_stage = nullptr, *d_stage = nullptr;  // Lay::SingleLay, twice: planes, poc, qp | split, flagged count, logits, record, candidate record | the guards' scratch
  Lay::SingleLay lay;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  uint64_t ws_gen_at_capture = 0;       // the graph bakes in workspace pointers: valid only for the workspace allocation it was captured on
  hipStream_t stream_at_capture = nullptr;
};

// mlt_submit / mlt_flush / mlt_wait: two generations of up to MLT_DEFER_CAP CUs per size (one accumulating, one in
// flight or finished).  Generation g uses buffer set g & 1; ticket = g * MLT_DEFER_CAP + slot.
struct Deferred {
  char *h_in = nullptr, *d_in = nullptr;    // [2 sets] of Lay::DeferIn: org planes, pred planes, poc, qp
  char *h_out = nullptr, *d_out = nullptr;  // [2 sets] of Lay::DeferOut: split, logits, flagged count, records, candidate records | the guards' scratch
  Lay::DeferIn in;
  Lay::DeferOut out;
  uint64_t gen = 0;                         // generation being filled
  int n = 0;                                // CUs submitted into it
  int n_launched[2] = {0, 0};               // CUs of the generation occupying each set (0: never launched)
  uint64_t gen_of_set[2] = {~0ull, ~0ull};
  hipEvent_t done[2] = {nullptr, nullptr};
  bool has_cand[2] = {false, false};        // the set's batch was launched with a candidate area (SizeState.cand_used at that time)
  bool guard_pending[2] = {false, false};   // set's batch ran with guards and its flagged CUs have not been re-evaluated yet
  int phase[2] = {0, 0};                    // which of the set's two selection counters (count[0 .. 1]) its next launch counts on (GuardSlot.phase)
};

// A device-resident picture (include/mltcnn.h: mlt_picture): one int16 luma plane per device of the context that owns it.  Library-owned planes are pitched to
// a multiple of 64 elements (rows start on 128-byte lines; any multiple of 8 would do for the gather's argument) and allocated as height x pitch elements, so the
// extent starts and ends on 16-byte boundaries and picture_gather_kernel may fetch 16-byte windows (mlt_picture_kernels.inc); a wrapped plane is the caller's
// memory -- base, stride and the extent (height - 1) x stride + width as declared -- and takes the vector paths only when that extent happens to start and end so.
struct mlt_picture {
  mlt_ctx *owner = nullptr;
  int width = 0, height = 0;
  long pitch = 0;                  // elements
  bool owned = false;              // allocated by mlt_picture_create (freed by mlt_picture_destroy / mlt_shutdown); false: mlt_picture_wrap_device
  bool vec = false;                // extent starts and ends 16-byte aligned
  std::vector<int16_t *> plane;    // [device index of the owner]: sample (0, 0)
};

struct ProfAcc { uint32_t launches = 0; double flops = 0, bytes = 0; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; };

struct mlt_ctx {
  // multi-device context (mlt_config.n_devices > 1): this object is the context of devices[0]; peers[i] is the full context of
  // devices[i + 1].  Host-pointer entry points shard over all of them (contiguous ranges, one host thread per peer), mlt_submit deals
  // CUs round-robin (the ticket's top byte is the device index); device-pointer calls, streams and profiles address ONE device
  // (mlt_device_ctx).  A peer never has peers of its own.
  std::vector<mlt_ctx *> peers;
  unsigned rr = 0;  // next device of mlt_submit
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  SizeState sz[4];
  float guard_margin = 3e-3f;  // decision guard: 3 x tolerance unless configured (mlt_init)
  bool guard_margin_configured = false;  // mlt_config.guard_margin > 0: used as is for every tier
  int max_batch = 4096, chunk = 4096;  // CUs per pass; MLT_CHUNK overrides (workspace ~1.5 MiB per CU at S = 128)
  char *ws = nullptr;
  size_t ws_bytes = 0;
  uint64_t ws_gen = 1;  // bumped by every (re)allocation / release of ws: a captured graph is replayed only on the generation it was captured on
                        // (an equal ADDRESS proves nothing once the workspace can shrink: a later, smaller allocation may land on it)
  char *zero_page = nullptr;  // 64 KiB of zeros: padding source of the LDS-DMA patch staging
  // mlt_predict_batch: second stream + events for the H2D / compute overlap, CUs per staged sub-chunk (MLT_STAGE_CHUNK)
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
  int stage_chunk = 512;  // measured on 4096 x 128x128 from pinned memory: 512 -> 526 k, 1024 -> 498 k, 2048 -> 426 k CU/s
  GrowBuf h_res{true};  // pinned result staging for the two sets (Lay::ResultSet: split, logits, records, candidate records)
  SingleCu single[12];  // [4 + si]: the calls that want the decision record (their graph bakes the record pointer into the heads kernel's arguments); [8 + si]: the
                        // calls that want the candidate record (and the decision record with it)
  Deferred deferred[4];
  // staging for the host-pointer entry points
  GrowBuf stage;
  // parity guards: selection buffers for two in-flight batches, gather staging for the flagged CUs
  float tolerance = 1e-3f;
  bool xlite = false;  // MLT_FLAG_EXACT_LITE: sizes configured exact run the exact-lite arithmetic (FP8 cross terms, mlt_model.h: xl)
  GrowBuf guard_dev;              // two slots of guard_lay, zero when allocated
  Lay::GuardLay guard_lay;        // (sized for the largest batch and logit count seen: a slot's counters stay where they are while the buffer does)
  int32_t *guard_host = nullptr;  // pinned: two counters
  int guard_phase[2] = {0, 0};    // which counter of a slot's pair the next batch launch counts on (GuardSlot.phase)
  hipEvent_t ev_guard = nullptr;  // "count of flagged CUs has landed" (device-pointer entry)
  GrowBuf gstage;
  GrowBuf sweep_guard_dev;              // QP sweeps: one slot of sweep_guard_lay (zero when allocated), its counter phase (GuardSlot.phase); the count lands in guard_host[2]
  Lay::SweepGuardLay sweep_guard_lay;
  int sweep_phase = 0;
  // mlt_predict_tree's / mlt_predict_trees' device arena (Lay::TreeArena) or mlt_predict_tree_sweep's / mlt_predict_trees_sweep's (Lay::TreeSweepArena), and the pinned count
  GrowBuf tree_dev;
  int32_t *tree_host = nullptr;
  GrowBuf motion_dev;   // mlt_picture_predict / mlt_picture_compensate and their _refs forms (mlt_motion.cpp: FieldBuf, RefsFieldBuf): this device's motion field(s)
  std::vector<mlt_picture *> pictures;  // every picture created on / wrapped for this context (mlt_pictures.cpp); what is left is released by mlt_shutdown
  std::string err;
  bool profile = false;
  bool guard_select_kernel = false;  // MLT_GUARD_SELECT_KERNEL (read at mlt_init, like MLT_CHUNK): the guards' selection of a BATCH as a launch of its own (round 5's form,
                                     // ascending list) instead of a tail of the heads kernel -- kept for the A/B and the bit-identity test
  bool lds_oob_zero = false;  // DS reads beyond the LDS allocation return zeros on this device (probed at init): chain kernels without zero masks
  std::map<std::string, ProfAcc> prof;
  std::vector<std::string> prof_order;
  // Round 6: != NULL = PLAN mode -- the dispatcher (run_network and the run_* functions under it) runs its decisions as usual but
  // RECORDS every launch (name + variant) here instead of enqueuing it, touches no device and allocates nothing: what a batch of n CUs of a tier
  // would launch, observable and unit-tested on the CPU (mlt_plan_describe, tests/test_launch_plan_cpu.py).
  std::vector<std::string> *plan = nullptr;
  bool plan_detail = false;   // ... with the buffers of every launch (offsets into the workspace, which plan mode carves from address 0): the hand-offs between launches
};

// the device-side record (mlt_kernels.h) is the C ABI's mlt_decision, field for field
static_assert(sizeof(mlt_decision) == 48 && sizeof(DecisionRec) == sizeof(mlt_decision), "mlt_decision is 48 bytes");
static_assert(offsetof(mlt_decision, confidence) == offsetof(DecisionRec, confidence) && offsetof(mlt_decision, level_mode) == offsetof(DecisionRec, level_mode) &&
              offsetof(mlt_decision, level_conf) == offsetof(DecisionRec, level_conf) && offsetof(mlt_decision, level_conf) == 32, "mlt_decision layout");

static_assert(sizeof(mlt_tree_node) == 32 && sizeof(TreeNodeRec) == 32 && offsetof(mlt_tree_node, size) == offsetof(TreeNodeRec, size) && offsetof(mlt_tree_node, parent) == 12 &&
              offsetof(TreeNodeRec, parent) == 12 && offsetof(mlt_tree_node, cand_mask) == offsetof(TreeNodeRec, cand_mask) && offsetof(mlt_tree_node, cand_mask) == 28, "mlt_tree_node layout");
static_assert(sizeof(mlt_tree_config) == 40, "mlt_tree_config is 40 bytes");
static_assert(sizeof(mlt_tree_picture) == 24 && MLT_TREES_ROW == MLT_MAX_LOGITS && MLT_TREES_LEVELS == Lay::TreeArena::kLevels && sizeof(TreesEntry) == 48, "mlt_predict_trees layouts");

static_assert(MLT_MOTION_MAX_REFS == MLT_MOTION_MAX_REFS_K && sizeof(mlt_motion_refs_config) == 24, "the motion kernels' reference arrays hold the ABI's maximum");
static_assert(MLT_SWEEP_MAX_QPS == MLT_SWEEP_MAX_QPS_K, "the sweep kernel's point array holds the ABI's maximum");
static_assert(sizeof(mlt_candidates) == 40 && sizeof(CandRec) == sizeof(mlt_candidates) && offsetof(mlt_candidates, order) == offsetof(CandRec, order) &&
              offsetof(mlt_candidates, prob) == offsetof(CandRec, prob) && offsetof(mlt_candidates, prob) == 16, "mlt_candidates layout");

#define HIP_TRY(ctx, expr)                                                                             \
  do {                                                                                                 \
    hipError_t e__ = (expr);                                                                           \
    if (e__ != hipSuccess) {                                                                           \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                                 \
      return MLT_ERR_HIP;                                                                              \
    }                                                                                                  \
  } while (0)

// a kernel launch of the dispatcher: skipped in plan mode (the launch was recorded by Launch::prof_begin)
#define LAUNCH_TRY(ctx, expr) do { if (!(ctx)->plan) HIP_TRY(ctx, expr); } while (0)

inline int check_size(mlt_ctx *ctx, int size, SizeState **out) {
  const int si = size_index(size);
  if (si < 0) { ctx->err = "unsupported CU size"; return MLT_ERR_ARG; }
  SizeState &st = ctx->sz[si];
  if (!st.enabled || !st.loaded) { ctx->err = "CU size not enabled or weights not loaded"; return MLT_ERR_SIZE_DISABLED; }
  *out = &st;
  return MLT_OK;
}
// a flagged-CU count that came back from a guarded pass on n CUs
inline int check_flagged_count(mlt_ctx *ctx, int k, int n) {
  if (k < 0 || k > n) { ctx->err = "guard: bad flagged-CU count"; return MLT_ERR_HIP; }
  return MLT_OK;
}

// the two Pel planes of a batch in device memory (element strides)
struct Planes {
  const int16_t *org, *pred;
  long org_rs, org_cs, pred_rs, pred_cs;
  static Planes dense(const int16_t *org, const int16_t *pred, int S) { return Planes{org, pred, S, (long)S * S, S, (long)S * S}; }
  // stem_block_kernel / layer0_stream_kernel fetch 4-pixel quads with 8-byte loads: planes 8-byte aligned, strides multiples of 4 elements
  bool aligned8() const { return (((uintptr_t)org | (uintptr_t)pred) & 7) == 0 && ((org_rs | org_cs | pred_rs | pred_cs) & 3) == 0; }
  // the six plane fields every launch struct that reads the raw planes carries (mlt_kernels.h)
  template <class Args> void fill(Args &a) const {
    a.org = org; a.pred = pred; a.org_row_stride = org_rs; a.org_cu_stride = org_cs; a.pred_row_stride = pred_rs; a.pred_cu_stride = pred_cs;
  }
};

// QP sweep part of a pass (off unless n_qps > 0): the heads step evaluates every CU under qps[0 .. n_qps) -- sweep_heads_kernel instead of the heads kernel --
// and output (q, i) of split / logits / dec / cand lies `slab` CUs x q behind output (0, i); PassIO.qp is NULL or the CUs' OFFSETS to every point (CU i under point q: qps[q] + qp[i]; tree sweeps over several entries).  idx + mask: the pass is the exact re-run of
// a sweep's flagged CUs -- CU j writes row idx[j] of the points in mask[idx[j]]; mask alone (with the guards' tail): where the fast pass leaves the CUs' masks.
struct SweepPart {
  int n_qps = 0;
  int32_t qps[MLT_SWEEP_MAX_QPS] = {0};
  long slab = 0;
  const int32_t *idx = nullptr;
  uint32_t *mask = nullptr;
  const uint32_t *active = nullptr;   // per CU, the points it takes part in: a CU is flagged only under those (tree sweeps); NULL: all points
};

// what a pass reads and writes per CU (device memory; any of the outputs may be NULL)
struct PassIO {
  Planes pl;
  const int32_t *poc, *qp;
  int32_t *split;
  float *logits;
  DecisionRec *dec;
  CandRec *cand = nullptr;
  SweepPart sweep;
};

// what a pass produces for the guards besides (all unset: a plain pass)
struct GuardOut {
  int32_t *d_flat = nullptr;        // the flat-content guard's per-CU statistic (fused into the first kernel where that kernel reads the raw planes as
                                    // aligned quads, else by flat_stat_kernel)
  const GuardTail *tail = nullptr;  // the selection as a tail of the heads kernel
  bool flat_is_clear = false;       // d_flat is zero on entry (the consumer of the previous call cleared it): no memset
  float *d_mag = nullptr;           // per-CU logit magnitude (HeadArgs.mag)
};

// profile / plan bookkeeping around one kernel launch (mlt_dispatch.cpp)
struct Launch {
  mlt_ctx *ctx;
  int prof_begin(const std::string &name, double flops, double bytes, hipEvent_t &e0, hipEvent_t &e1, const char *variant = nullptr);
  int prof_end(hipEvent_t e1);
};

// One launch with its profile row (plan mode: its record): prof_begin, the launch, prof_end; leaves the calling function with the code of whichever fails.
// PROF_HIP_TRY enqueues in plan mode as well (HIP_TRY), PROF_LAUNCH_TRY does not (LAUNCH_TRY); `expr` is the launch, a hipError_t.
#define PROF_TRY_(TRY, ctx, name, flops, bytes, expr)                                                  \
  do {                                                                                                 \
    Launch l__{ctx};                                                                                   \
    hipEvent_t e0__ = nullptr, e1__ = nullptr;                                                         \
    int rc__;                                                                                          \
    if ((rc__ = l__.prof_begin(name, flops, bytes, e0__, e1__))) return rc__;                          \
    TRY(ctx, expr);                                                                                    \
    if ((rc__ = l__.prof_end(e1__))) return rc__;                                                      \
  } while (0)
#define PROF_HIP_TRY(ctx, name, flops, bytes, expr) PROF_TRY_(HIP_TRY, ctx, name, flops, bytes, expr)
#define PROF_LAUNCH_TRY(ctx, name, flops, bytes, expr) PROF_TRY_(LAUNCH_TRY, ctx, name, flops, bytes, expr)

// contiguous shard of n items for device g of G (fastintercu-vvc_amd/shard.py: shard_bounds)
inline int shard_lo(int n, int g, int G) { return (int)(((long long)n * g) / G); }
inline mlt_ctx *device_of(mlt_ctx *ctx, int i) { return i == 0 ? ctx : ctx->peers[(size_t)i - 1]; }
// A call on n items of a multi-device context: per_device(g, lo, hi) on device g's shard, one host thread per further device, no exchange between them (every
// device runs the single-device path, so the results are those of one device).  The first failing device's code; a peer's message is prefixed "device N: ".
template <class F> int run_sharded(mlt_ctx *ctx, int n, F per_device) {
  const int G = 1 + (int)ctx->peers.size();
  std::vector<int> rcs((size_t)G, MLT_OK);
  auto run = [&](int g) { const int lo = shard_lo(n, g, G), hi = shard_lo(n, g + 1, G); if (hi > lo) rcs[(size_t)g] = per_device(g, lo, hi); };
  std::vector<std::thread> th;
  for (int g = 1; g < G; ++g) th.emplace_back(run, g);
  run(0);
  for (std::thread &t : th) t.join();
  for (int g = 0; g < G; ++g)
    if (rcs[(size_t)g]) { if (g) ctx->err = "device " + std::to_string(device_of(ctx, g)->device) + ": " + device_of(ctx, g)->err; return rcs[(size_t)g]; }
  return MLT_OK;
}

// ---- functions that cross translation units ----
// mlt_pictures.cpp
void free_pictures(mlt_ctx *ctx);               // mlt_shutdown: before the peers go
bool owns_picture(const mlt_ctx *ctx, const mlt_picture *pic);
const int kPictureMinDim = 16, kPictureMaxDim = 16384;   // a picture's width and height (mlt_picture_create)
// the picture pair of a one-pair call: both of this context, one geometry (`who` opens the message)
int check_at_pair(mlt_ctx *ctx, const char *who, const mlt_picture *org, const mlt_picture *pred);
// the picture pair as one device sees it | the CUs of a call: a host list with poc / qp per CU, a DEVICE list of positions that all take one (poc, qp) pair, or a
// device list over the entries of a device table (mlt_predict_trees: AtPlanes is not read) |
// where the results go (host arrays for a host list, device arrays for a device list; any may be NULL)
struct AtPlanes {
  const int16_t *org; long org_pitch; bool org_vec;
  const int16_t *pred; long pred_pitch; bool pred_vec;
  static AtPlanes of(const mlt_picture *o, const mlt_picture *p, int g) { return AtPlanes{o->plane[(size_t)g], o->pitch, o->vec, p->plane[(size_t)g], p->pitch, p->vec}; }
};
struct AtList {
  const int32_t *xy, *poc, *qp;
  bool device; int32_t poc_all, qp_all;
  const int32_t *pic = nullptr; const TreesEntry *entries = nullptr; int n_entries = 0;   // device lists of SEVERAL pairs: CU i is of entry pic[i] (planes, poc, qp from the table)
  static AtList host(const int32_t *xy, const int32_t *poc, const int32_t *qp) { return AtList{xy, poc, qp, false, 0, 0}; }
  static AtList on_device(const int32_t *d_xy, int32_t poc, int32_t qp) { return AtList{d_xy, nullptr, nullptr, true, poc, qp}; }
  static AtList of_entries(const int32_t *d_xy, const int32_t *d_pic, const TreesEntry *d_entries, int n) { return AtList{d_xy, nullptr, nullptr, true, 0, 0, d_pic, d_entries, n}; }
};
struct AtOut { int32_t *split; float *logits; mlt_decision *dec; mlt_candidates *cand; };
int predict_at_chunks(mlt_ctx *dev, SizeState *st, const AtPlanes &pl, int n, const AtList &at, const AtOut &out);
// One chunk's gather, enqueued on dev's stream: the c CUs of size x size at d_xy (device) out of the pair's planes into the dense staging planes g_org / g_pred --
// or, with d_pic, CU i out of the planes of entry d_pic[i] of the device table `entries`, its poc and qp into g_poc / g_qp besides (pl is not read).
struct GatherSrc { AtPlanes pl; const TreesEntry *entries; int n_entries; };
int enqueue_gather(mlt_ctx *dev, const GatherSrc &src, const int32_t *d_xy, const int32_t *d_pic, int16_t *g_org, int16_t *g_pred, int32_t *g_poc, int32_t *g_qp, int c,
                   int size);
// mlt_dispatch.cpp
void release_ws(mlt_ctx *ctx);
int run_network(mlt_ctx *ctx, SizeState &st, const NetCfg &c, int n, const PassIO &io, const GuardOut &go = GuardOut());
// mlt_guards.cpp
int guard_slot(mlt_ctx *ctx, int which, int n, int nl, GuardSlot *g);
int run_fast_async(mlt_ctx *ctx, SizeState &st, int n, const PassIO &io, const GuardSlot &g);
int guard_fixup_async(mlt_ctx *ctx, SizeState &st, int k, const PassIO &io, const GuardSlot &g);
int run_checked(mlt_ctx *ctx, SizeState &st, int n, const PassIO &io);
int run_checked_sweep(mlt_ctx *ctx, SizeState &st, int n, const PassIO &io);   // io.sweep: qps, n_qps, slab
// mlt_calibrate.cpp
void free_model(mlt::Model &m);
void drop_graphs(mlt_ctx *ctx, int si);
