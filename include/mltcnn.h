/*
 * mltcnn.h -- C ABI of the MI355X-native MLT-CNN inter-CU split predictor.
 *
 * Drop-in boundary for the inline CNN block of the reference encoder
 *   /root/reference/vtm-mlt-cpp/source/Lib/EncoderLib/EncCu.cpp:799-930
 * (the reference has no plugin API; this header IS the interface a maintainer binds, see
 * INTEGRATION.md).  Plain C types only, no C++ exceptions cross it, no torch / OpenCV.
 *
 * Error contract (mirrors the reference's swallow-and-continue, EncCu.cpp:902-905,923-926):
 * every call returns MLT_OK (0) or a non-zero code and NEVER aborts; on failure the caller
 * leaves predictedSplitMode = -1, for which EncModeCtrl::setNewModeList is a no-op
 * (EncModeCtrl.cpp:147-148) and the encoder falls back to exhaustive RDO.
 */
#ifndef MLTCNN_H
#define MLTCNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLT_ABI_VERSION 4

enum {
  MLT_OK = 0,
  MLT_ERR_ARG = 1,        /* bad pointer / size / batch */
  MLT_ERR_NO_DEVICE = 2,  /* HIP device missing or unusable */
  MLT_ERR_WEIGHTS = 3,    /* weight file / blob missing or malformed */
  MLT_ERR_SIZE_DISABLED = 4, /* CU size not enabled in size_mask or no weights loaded for it */
  MLT_ERR_HIP = 5,        /* a HIP runtime call failed (see mlt_last_error) */
  MLT_ERR_NOMEM = 6
};

/* CU sizes the two reference models cover (EncCu.cpp:754 gate; only 128 is active upstream). */
#define MLT_SIZE_128 0x1u
#define MLT_SIZE_64 0x2u
#define MLT_SIZE_32 0x4u
#define MLT_SIZE_16 0x8u

#define MLT_MAX_LOGITS 15 /* CU model: 2+3+4+6; CTU (128) model: 2+3+4 = 9 */

/* mlt_config.flags -- arithmetic of the conv stack (DESIGN.md "Numerics").
 * fast : fp16 operands on the MFMA units, fp32 accumulate.  Its logit error depends on the weight set (rms 1.4e-4 ... 5.5e-4
 *        over seeded weight sets, tails ~4.5x rms) and on the content (exactly-constant areas carry coherent rounding errors).
 * exact: every weight / activation is an fp16 (hi, lo) pair, 3 MFMA passes, ~fp32 accuracy (|dlogit| ~ 1e-5).
 * Defaults: 128x128 -> fast WHEN the load-time calibration says the weight set meets mlt_config.tolerance with it (else a middle
 * tier or exact, see mlt_load_weights); 64/32/16 -> CONFIGURED exact (few pixels per map, so fp16 rounding is not averaged away by the
 * global pooling, and these models are 5-65x cheaper), but the same calibration may keep layer0 -- or one of its two launch units --
 * on the single-pass or hi+lo-weights kernels when the contract still holds with it (mlt_arith_info.exact == 4, .x_units = what
 * stays exact; admission as for the 128 model but with the largest error held to 0.5 x tolerance instead of 0.65 x: their tails are
 * heavier).  Sizes with ANY non-exact unit are protected by two device-side guards (and keep a second, exact copy of the weights
 * resident), applied on EVERY entry point (single, batch, device-pointer, deferred):
 *   flat guard (default on): CUs in which >= 1/8 of the aligned 4-pixel quads are EXACTLY FLAT (org and |org - pred| each constant or
 *                            exactly linear over the quad) or >= 1/2 are NEAR-FLAT (each spans <= 8 ten-bit steps or is linear to
 *                            within one step: +-1 LSB dither, low-contrast texture, ramps) are re-evaluated with the exact
 *                            arithmetic (their fp16 rounding errors are coherent, the global pooling does not average them away);
 *   decision guard (default on since ABI 4 -- split modes are what the encoder consumes, EncCu.cpp:921 -> EncModeCtrl.cpp:110-149;
 *                            MLT_FLAG_NO_DECISION_GUARD turns it off): CUs whose decision-head top-2 margin is below guard_margin
 *                            (default 3 x tolerance) are re-evaluated too, so the split mode handed to
 *                            EncModeCtrl::setNewModeList is the one ~fp32 arithmetic gives.  A CU with a NaN logit on the
 *                            decision head is re-evaluated as well, whatever its other classes' margin.
 * Both cost a second (exact) copy of the weights on the device (11 MB). */
#define MLT_FLAG_EXACT_128 0x1u
#define MLT_FLAG_FAST_SMALL 0x2u       /* single-pass fp16 for 64/32/16 (measurement only: NO seeded weight set meets 1e-3 with it --
                                          2e-3 ... 6e-3 measured -- and it is neither calibrated nor guarded) */
#define MLT_FLAG_DECISION_GUARD 0x4u    /* ABI <= 3: opt-in to the decision guard.  Since ABI 4 the guard is the default: accepted, no effect */
#define MLT_FLAG_NO_FLAT_GUARD 0x8u    /* fast arithmetic without the flat-content guard (measurement only) */
#define MLT_FLAG_NO_CALIBRATION 0x10u  /* keep the fast arithmetic whatever the weight set (measurement only) */
#define MLT_FLAG_EXACT_LITE 0x40u      /* ABI 4 (round 5, measurement): sizes configured exact (MLT_FLAG_EXACT_128; 64/32/16 with MLT_FLAG_NO_CALIBRATION) run the
                                          "exact-lite" arithmetic: Wh*Xh in fp16, the two cross terms Wl*Xh + Wh*Xl as ONE scaled FP8 MFMA per tap and 32 channels
                                          (2 fp16-equivalent MFMAs per product instead of 3; |dlogit| ~ 1/20 of the single pass's) */
#define MLT_FLAG_NO_MAGNITUDE_GUARD 0x80u /* round 6 (measurement only): never admit a tier behind the magnitude guard (mlt_arith_info.mag_guard_thr): the round-5 search */
#define MLT_FLAG_NO_DECISION_GUARD 0x20u /* ABI 4: fast arithmetic without the decision guard (measurement only: a split whose reference margin is
                                          below ~2 x tolerance may then differ from the reference's) */

typedef struct mlt_ctx mlt_ctx;

typedef struct mlt_config {
  uint32_t struct_size;   /* = sizeof(mlt_config) */
  int32_t device;         /* HIP device ordinal (reference: at::kCUDA hard-coded, EncCu.cpp:804) */
  const char *weights_dir;/* directory holding MLTORPQ_splitMode_<S>.mltw, the blob counterpart of the
                             reference's hard-coded ".../torch_model/MLTORPQ_splitMode_<S>.pt"
                             (EncCu.cpp:897-899).  NULL: load later with mlt_load_weights(). */
  uint32_t size_mask;     /* MLT_SIZE_* bits to enable; 0 => MLT_SIZE_128 (reference default, :754) */
  int32_t head_index[4];  /* decision head per size {128,64,32,16}; -1 => reference default:
                             element [2] for 128, [0] otherwise (EncCu.cpp:913-919) */
  int32_t max_batch;      /* largest n passed to mlt_predict_batch*; 0 => 4096 */
  uint32_t flags;         /* MLT_FLAG_* bits, 0 = defaults */
  float guard_margin;     /* decision-guard threshold on (top1 - top2) of the decision head; <= 0 => 3 x tolerance.  Two logits that are each
                             within `tolerance` of the reference move their difference by at most 2 x tolerance; the admission of the fast
                             arithmetic is CALIBRATED (statistical), not proven, and its tail probes saw single logits at up to ~1.1 x tolerance,
                             hence 3 x rather than 2 x: everything below the threshold is re-evaluated exactly */
  float tolerance;        /* |dlogit| contract the fast arithmetic is calibrated against at load time; <= 0 => 1e-3
                             (BASELINE.json north_star) */
  uint32_t reserved;      /* 0 */
  /* ---- since ABI 3.  ABI 4 is a hard break: struct_size must equal sizeof(mlt_config) (the 56-byte ABI-2 struct is rejected with
     MLT_ERR_ARG -- an ABI-2 binary would also hand mlt_arithmetic a 32-byte mlt_arith_info) ---- */
  int32_t n_devices;      /* 0: the single `device` above.  k >= 1: devices[0..k-1] -- ONE context serving k GPUs of the node (SURVEY.md 8e
                             "CTUs within a frame shard across the GPUs"; the encoder is one process): weights are uploaded (and
                             calibrated) once per device from the one host blob, mlt_predict_batch shards its batch contiguously over the
                             devices (one host thread each, no exchange between them), mlt_submit deals CUs round-robin and mlt_flush /
                             mlt_wait / mlt_synchronize / mlt_load_weights / mlt_shutdown address all of them; mlt_predict, the
                             device-pointer entry, mlt_set_stream and the profile calls address devices[0] (use mlt_device_ctx for the
                             others).  Results are bit-identical to a one-device context.  An ordinal may be listed more than once
                             (several contexts on one GPU: how a 1-GPU box exercises this path). */
  int32_t devices[8];
} mlt_config;
#define MLT_MAX_DEVICES 8

/* Create a context: selects the device, allocates workspaces, loads + folds + packs weights
 * ONCE (the reference re-reads the .pt on every CU, EncCu.cpp:894-900).  Natural home:
 * EncCu::init (EncCu.cpp:233-259).  Thread-compatible: one ctx per EncCu / encoder thread. */
int mlt_init(const mlt_config *cfg, mlt_ctx **out);

/* Multi-device contexts: number of devices served (1 for a plain context) and the context of devices[index] -- a full single-device
 * context owned by `ctx` (never shut it down itself), for the calls that address one device (mlt_predict_batch_device with buffers on
 * that GPU, mlt_set_stream, mlt_profile_*, mlt_arithmetic).  index 0 returns ctx. */
int mlt_num_devices(const mlt_ctx *ctx);
mlt_ctx *mlt_device_ctx(mlt_ctx *ctx, int index);

/* Load weights for one CU size from an in-memory MLTW blob (format: weights.py).  Used when the
 * blob arrives over RCCL broadcast instead of from weights_dir.  A size configured for the fast arithmetic is
 * CALIBRATED here: 560 seeded synthetic CUs in six content classes the flat guard does not catch (texture, i.i.d. uniform,
 * constant org / textured pred, textured org / constant pred, a constant band and a near-flat band just under the guard's two thresholds) run
 * through the fast and the exact arithmetic on the device; the fast arithmetic is kept only if
 * 5.5 x (the worst rms|dlogit| pooled per content class and per head) <= tolerance and max|dlogit| (over 5040 logits) <=
 * 0.65 x tolerance (the largest of 295 k probed logits measured up to 1.7 x the largest of these 5040) -- for a set whose largest
 * error exceeds 5 x its overall rms (heavy tail) the 5.5 grows with that ratio, up to 6.5;
 * first with the default realisation of the weights' tap-diffused rounding, then with five others (mlt_arith_info.rounding);
 * otherwise the 128 model tries the middle tiers the same way -- (hi, lo) pairs for the WEIGHTS only (hi fp16; lo fp16, or e4m3 with a
 * per-layer power-of-two scale where the layer has >= 128 input channels: the lo term carries < 2^-11 of the product), on the W2 forms
 * of the fused kernels, in a SUBSET of the four stages: the 15 subsets are priced in the order of
 * their measured cost and the cheapest one that meets the contract is kept (mlt_arith_info.w2_stages); failing those, the tiers that
 * put one to three stages into the exact arithmetic and the others into (hi, lo) weights (.x_stages), cheapest first -- and a size that
 * meets the contract with none of them is priced in the exact-lite arithmetic (mlt_arith_info.exact == 5; what a TRAINED-like weight set lands
 * on: profiles/r05d_trained_family.txt) and runs exact only if that fails too (mlt_arithmetic reports the outcome).  The
 * admission is STATISTICAL (synthetic content, Gaussian-tail factor), not a bound: "within 1e-3" is calibrated, not proven. */
int mlt_load_weights(mlt_ctx *ctx, int size, const void *blob, size_t bytes);

/* Arithmetic a size runs after loading + what the calibration measured.  The caller sets struct_size = sizeof(mlt_arith_info) BEFORE the
 * call (ABI 4); the library writes only the fields that fit into struct_size bytes and fails with MLT_ERR_ARG when struct_size does not
 * even cover the ABI-4 fields below, so a later, longer struct never overruns an older caller's storage. */
typedef struct mlt_arith_info {
  uint32_t struct_size;   /* in: sizeof(mlt_arith_info) of the caller */
  int32_t exact;          /* 0: fast; 1: exact ((hi, lo) pairs for weights and activations); 2: (hi, lo) weights on fp16 activations in
                             every stage; 3: (hi, lo) weights in SOME stages (w2_stages), single pass in the others; 4: the exact arithmetic in the
                             stages of x_stages, (hi, lo) weights in the others (w2_stages); 5 (round 5): exact-lite in every stage -- (hi, lo) pairs
                             with Wh*Xh in fp16 and both cross terms Wl*Xh + Wh*Xl in ONE scaled FP8 MFMA per tap and 32 channels: 2 fp16-equivalent
                             MFMAs per product instead of 3, |dlogit| ~ 1/20 of the single pass's (1e-5 rms); tried after every fp16 tier, before exact */
  int32_t calibrated;     /* 1: the calibration ran for this size */
  float calib_rms, calib_max; /* |dlogit| of the chosen non-exact tier (or of the fast one if exact was chosen) vs exact over the calibration CUs:
                                 worst rms pooled per content class / per head, and the overall maximum */
  int32_t flat_guard, decision_guard;
  uint64_t guard_reruns;  /* CUs re-evaluated by the guards since init */
  int32_t w2_stages;      /* ABI 3: bit s set = layer s (0..3) runs (hi, lo) weights; 0 for the fast and the exact arithmetic */
  float guard_margin;     /* ABI 3: the decision guard's threshold in effect for this size (0 when the guard is off) */
  int32_t x_stages;       /* ABI 3: bit s set = layer s runs the exact arithmetic inside a mixed tier (exact == 4); 0 otherwise */
  int32_t w2_units;       /* ABI 3: w2_stages at launch-unit granularity: bit 2 s = layer s's first unit (layer0.0 / its stride-2 conv + shortcut),
                             bit 2 s + 1 = its second (layer0.1 / its three stride-1 convs) */
  int32_t x_units;        /* ABI 3: x_stages at the same launch-unit granularity */
  int32_t rounding;       /* ABI 3: which realisation of the single-pass weights' tap-diffused rounding the calibration kept (0 = the default) */
  int32_t calib_cus;      /* ABI 4: CUs the last calibration priced (synthetic + caller's, without those the flat guard re-evaluates exactly anyway) */
  int32_t calib_caller_cus; /* ABI 4: ... of which supplied by the caller through mlt_calibrate */
  /* ---- round 6 (appended: written only when struct_size covers them; a 72-byte ABI-4 struct is still accepted) ----
   * MAGNITUDE guard.  The fp16 tiers' error is relative: it scales with M = max over logits of sum_k |w_ck gap_k|, the size of the feature-driven
   * part of the logits (the head's poc / qp / bias terms are exact).  A weight set that amplifies content far outside its training range -- a
   * residual plane of hundreds of ten-bit steps -- produces logits and absolute errors 20-80 x those of ordinary content there; such a set is
   * admitted to a non-exact tier BEHIND this guard: CUs with M > mag_guard_thr are re-evaluated with the exact arithmetic (third guard beside
   * the flat-content and the decision guard, same re-run path, counted in guard_reruns).  The threshold is the largest magnitude (on a
   * quarter-octave grid) up to which the calibration CUs -- the 560 synthetic ones, the caller's, and 320 further in-distribution CUs (texture +
   * 1/f scenes) -- meet the admission rule in its stricter "refinement" form (5.5 .. 6.5 x rms <= 0.95 x, max <= 0.6 x tolerance) with at most
   * 5 % of the in-distribution CUs above it; calib_rms / calib_max are the figures of the CUs at or below it.  0: the tier was admitted by the
   * plain rule, no such guard. */
  float mag_guard_thr;      /* the threshold in effect (0: no magnitude guard: exact arithmetic, small models, MLT_FLAG_NO_MAGNITUDE_GUARD) */
  float mag_guard_flagged;  /* fraction of the in-distribution calibration CUs (texture, 1/f scenes, the caller's) above the threshold: what the guard costs on ordinary content */
  int32_t mag_guard_kind;   /* 2: the tier was admitted BEHIND the guard (above).  1: RANGE guard -- the plain rule admitted the tier, which is still only validated on
                               the magnitudes its calibration CUs had while its error grows linearly with M: mag_guard_thr = 1.5 x the largest calibrated magnitude
                               (1.5 x the 0.65 x tolerance its largest calibration error may reach = the tolerance); nothing inside the calibrated range is ever
                               flagged.  0: none */
} mlt_arith_info;
int mlt_arithmetic(mlt_ctx *ctx, int size, mlt_arith_info *out);

/* ABI 4: calibrate on the INTEGRATOR's content.  mlt_load_weights decides the arithmetic of a size on 560 synthetic CUs generated inside the
 * library; this call repeats that decision -- the same admission rule, the same search (csrc/mlt_tier_search.h) -- with n CUs of the caller's
 * (HOST memory, dense [n][size][size] int16 org / pred as in mlt_predict_batch, int32 poc / qp; e.g. what host/mlt_split_predictor.hpp's call
 * dump recorded from real sequences: tools/calibrate_from_dump.py) APPENDED to the synthetic set (their own content class: the worst pooled
 * rms over classes counts) or REPLACING it.  Caller CUs the flat-content guard re-evaluates exactly anyway are left out of the statistics
 * (mlt_arith_info.calib_caller_cus = those that counted).  MLT_CALIB_REPLACE with fewer than 256 CUs that count (a tiny n, or content the
 * flat guard takes anyway) cannot carry the statistical admission rule: the call then behaves like MLT_CALIB_APPEND (the synthetic set stays;
 * mlt_arith_info.calib_cus > calib_caller_cus tells) -- no arithmetic is ever admitted on an empty or near-empty set.  1 <= n <= 4096.  The size must have been loaded with mlt_load_weights / weights_dir
 * (the library keeps the blob); sizes configured exact (MLT_FLAG_EXACT_128) or loaded with MLT_FLAG_NO_CALIBRATION are left alone.  Every
 * device of a multi-device context is re-calibrated; like a reload it invalidates captured graphs, and the outcome is read with
 * mlt_arithmetic.  On failure the size is unloaded (the caller keeps -1 / full RDO until it loads weights again). */
#define MLT_CALIB_APPEND 0
#define MLT_CALIB_REPLACE 1
int mlt_calibrate(mlt_ctx *ctx, int size, const int16_t *org, const int16_t *pred, const int32_t *poc, const int32_t *qp, int n, int mode);

/* Replaces EncCu.cpp:806-921 for ONE CU: gathers size x size luma from the original and the
 * prediction buffers (Pel = int16, element strides as AreaBuf exposes them, Buffer.h:94-105),
 * absdiff, 1/1023 normalisation, network, argmax.  Synchronous.
 *   split_mode  <- argmax of the decision head (first maximal index, like torch.argmax)
 *   logits_opt  <- all head logits, lvl1..lvlN concatenated (mlt_num_logits(size) floats) or NULL */
int mlt_predict(mlt_ctx *ctx, const int16_t *org, int org_stride, const int16_t *pred, int pred_stride,
                int size, int32_t poc, int32_t qp, int32_t *split_mode, float *logits_opt);

/* n CUs from HOST memory.  org / pred: dense [n][size][size] int16.  Synchronous.  logits may be NULL.
 * Batches larger than one staging sub-chunk (512 CUs, MLT_STAGE_CHUNK) are pipelined: the H2D copy of the next
 * sub-chunk overlaps the kernels of the current one -- effective only when org / pred are pinned (mlt_alloc_pinned). */
int mlt_predict_batch(mlt_ctx *ctx, int n, int size, const int16_t *org, const int16_t *pred,
                      const int32_t *poc, const int32_t *qp, int32_t *split_mode, float *logits);

/* Same with every pointer in DEVICE memory; enqueues on the context's stream; call mlt_synchronize before reading the
 * results.  With a guard active for `size` the call BLOCKS once per chunk until the chunk's fast pass has delivered the NUMBER of
 * flagged CUs (4 bytes) -- it sleeps for the expected duration of the batch and polls only for the last ~0.2 ms (MLT_GUARD_SPIN_WAIT=1
 * polls from the start, MLT_GUARD_BLOCKING_WAIT=1 sleeps on the event) -- then enqueues their exact re-evaluation; without guards it
 * never synchronises.  This is the
 * HBM-resident path bench.py times. */
int mlt_predict_batch_device(mlt_ctx *ctx, int n, int size, const void *d_org, const void *d_pred,
                             const void *d_poc, const void *d_qp, void *d_split_mode, void *d_logits);

/* Deferred single-CU prediction (encoder-side batching, SURVEY.md 8f N3: "async predict + deferred setNewModeList").
 * mlt_submit copies one CU's planes (same arguments as mlt_predict) into pinned staging and returns a ticket at once;
 * nothing runs yet.  mlt_flush launches every CU submitted so far for that size as ONE batch and returns without
 * waiting; mlt_wait returns a ticket's result, flushing first if its batch has not been launched.  An encoder that
 * can postpone EncModeCtrl::setNewModeList for k independent CUs (CTUs of a wavefront, EncCu.cpp:792-800) pays one
 * ~0.2 ms launch for all k instead of k synchronous calls.  Up to MLT_DEFER_CAP CUs per batch (a full batch is flushed
 * by the next submit); a ticket stays valid until two further batches of its size have been started.  Results are
 * bit-identical to mlt_predict (guards included: flagged CUs of a batch are re-evaluated by its first mlt_wait). */
#define MLT_DEFER_CAP 64
typedef uint64_t mlt_ticket;
int mlt_submit(mlt_ctx *ctx, const int16_t *org, int org_stride, const int16_t *pred, int pred_stride,
               int size, int32_t poc, int32_t qp, mlt_ticket *ticket);
int mlt_flush(mlt_ctx *ctx, int size);
int mlt_wait(mlt_ctx *ctx, int size, mlt_ticket ticket, int32_t *split_mode, float *logits_opt);

/* ---- Per-level decisions with confidence, and a confidence gate on the split (new exports; MLT_ABI_VERSION stays 4) ----
 * The network is a multi-level tree (three heads for the 128 model: 2 / 3 / 4 classes; four for the CU models: 2 / 3 / 4 / 6).  The decision record
 * carries, per CU, every head's argmax and how sure the network is of it, computed on the device from the logits the call returns: softmax in fp32 on
 * the max-subtracted logits with the full-precision expf, every class through the same operations (tied rows give tied probabilities).
 * mlt_config.head_index[] keeps its meaning: it selects the DECISION head, whose fields fill split_mode / raw_mode / confidence / margin. */
typedef struct mlt_decision {   /* 48 bytes, little-endian, no padding */
  int32_t split_mode;     /* what the encoder consumes: raw_mode, or -1 when the gate withholds it */
  int32_t raw_mode;       /* argmax of the decision head (first maximal index), gate ignored */
  float   confidence;     /* softmax probability of raw_mode within the decision head */
  float   margin;         /* top-1 minus top-2 logit of the decision head.  Defined for finite logits: the scan starts from -3.4e38, so a -inf logit
                             counts as -3.4e38, and a NaN logit never wins a comparison (the margin is then that of the other classes; the decision
                             guard tests for the NaN itself) */
  int32_t level_mode[4];  /* argmax of every head, lvl1..lvl4 (first-max rule); -1 for a head the model lacks */
  float   level_conf[4];  /* its softmax probability; 0 for a head the model lacks */
} mlt_decision;

/* Confidence gate of one CU size: split_mode = confidence >= min_confidence ? raw_mode : -1 (a NaN confidence gates), applied ON THE DEVICE to the
 * split output of EVERY entry point, old and new -- -1 is what EncModeCtrl::setNewModeList treats as "no prediction" (exhaustive RDO), so an
 * integrator trades encode-time saving against BD-rate with this one number.  0 <= min_confidence < 1; 0 = off (the default: every call returns what
 * it returned without the gate, from the same launches).  NaN, negative or >= 1 -> MLT_ERR_ARG; size not loaded -> MLT_ERR_SIZE_DISABLED.  Addresses
 * every device of a multi-device context, takes effect for batches launched after it returns, and invalidates captured graphs the way a weight reload
 * does.  Not a property of the weights: mlt_load_weights of that size and mlt_calibrate keep it.
 * Gate guard: on sizes that run a non-exact tier with the decision guard on, a CU whose confidence lies within 0.75 x tolerance of the threshold is
 * re-evaluated with the exact arithmetic like a near-tie (two logits within `tolerance` of the reference move a softmax probability by at most
 * tolerance / 2; the factor 1.5 on top is the decision guard's), so fp16 rounding does not decide which side of the gate a CU falls on. */
int mlt_set_confidence_gate(mlt_ctx *ctx, int size, float min_confidence);
int mlt_get_confidence_gate(mlt_ctx *ctx, int size, float *min_confidence);

/* The decision-record twins of mlt_predict / mlt_predict_batch / mlt_predict_batch_device / mlt_wait: same arguments, same implementation (chunking,
 * staging pipeline, guards, sharding over devices[], deferred slots), a record per CU in place of the split mode; the logits they return are
 * bit-identical to their twins', and with the gate off raw_mode == split_mode == the twin's split.  d_decisions: n x 48 bytes of DEVICE memory. */
int mlt_predict_decision(mlt_ctx *ctx, const int16_t *org, int org_stride, const int16_t *pred, int pred_stride,
                         int size, int32_t poc, int32_t qp, mlt_decision *out, float *logits_opt);
int mlt_predict_batch_decisions(mlt_ctx *ctx, int n, int size, const int16_t *org, const int16_t *pred,
                                const int32_t *poc, const int32_t *qp, mlt_decision *out, float *logits);
int mlt_predict_batch_device_decisions(mlt_ctx *ctx, int n, int size, const void *d_org, const void *d_pred,
                                       const void *d_poc, const void *d_qp, void *d_decisions, void *d_logits);
int mlt_wait_decision(mlt_ctx *ctx, int size, mlt_ticket ticket, mlt_decision *out, float *logits_opt);

/* ---- Candidate split sets: top-p mode masks on every entry point (new exports; MLT_ABI_VERSION stays 4) ----
 * Between "test exactly one split" (the integer) and "test everything" (-1): per CU, the smallest set of classes of the DECISION head that carries a chosen share
 * of the softmax probability, with a cap above which the CU falls back to full RDO.  Computed on the device from the logits the call returns (K classes, l[0..K-1]):
 *   1. rank     stable sort of the classes by logit, descending; equal logits put the lower class first (the first-max rule, extended); order[r] = class at rank r
 *   2. prob     e[k] = expf(l[k] - l[order[0]]), sum added in class order, prob[k] = e[k] / sum, fp32 -- the operations behind mlt_decision.confidence, so
 *               prob[raw_mode] is bit-equal to it
 *   3. cum      cum[r] = prob[order[0]] + ... + prob[order[r]], fp32, added in rank order
 *   4. n        the smallest r + 1 with cum[r] >= coverage; K if rounding lets no prefix reach it
 *   5. cap      max_modes > 0 and n > max_modes: the network is unsure, all K classes are kept (full RDO, the meaning of the gate's -1); else the first n ranks
 *   6. mask     bit k set for every kept class k; count = popcount(mask)
 *   7. NaN      any NaN logit in the head keeps all K classes (order then lists them in class order)
 * The default policy (0, 0) gives mask = 1 << raw_mode, count = 1; (t, 1) is the confidence gate restated as a mask (one class iff confidence >= t, else all).
 * The bits are CLASS INDICES of the decision head; mapping classes to PartSplit stays the integrator's job, as for the integer (identity for head [2] of the 128
 * model).  Policy and confidence gate are independent: the gate changes split_mode only, the policy the candidate record only. */
typedef struct mlt_candidates {   /* 40 bytes, little-endian, no padding */
  uint32_t mask;      /* bit k = class k of the decision head stays in the RDO */
  int32_t  count;     /* popcount(mask) */
  int8_t   order[8];  /* classes, most probable first; -1 beyond K */
  float    prob[6];   /* softmax probability of class k (class order); 0 beyond K */
} mlt_candidates;

/* Candidate policy of one CU size.  0 <= coverage < 1 (NaN, negative or >= 1 -> MLT_ERR_ARG); 0 <= max_modes <= K of the size's decision head (else MLT_ERR_ARG);
 * size not loaded -> MLT_ERR_SIZE_DISABLED.  Like the gate: per-size state, addresses every device of a multi-device context, takes effect for batches launched
 * after it returns, invalidates captured graphs, survives mlt_load_weights and mlt_calibrate.
 * Candidate guard: on sizes that run a non-exact tier with the decision guard on, once a policy other than (0, 0) is set, a CU is re-evaluated with the exact
 * arithmetic (counted in guard_reruns) when (a) a proper prefix sum lies within 0.75 x tolerance of the coverage, or (b) classes are dropped and the logit gap
 * between the last kept and the first dropped class is below the size's guard margin -- so fp16 rounding decides neither how many classes are kept nor which
 * one is the last.  Like the gate guard it acts on EVERY entry point of that size, old ones included (the twins' logits stay bit-identical). */
int mlt_set_candidate_policy(mlt_ctx *ctx, int size, float coverage, int max_modes);
int mlt_get_candidate_policy(mlt_ctx *ctx, int size, float *coverage, int *max_modes);

/* The candidate twins of mlt_predict / mlt_predict_batch / mlt_predict_batch_device / mlt_wait: same arguments, same implementation (chunking, staging
 * pipeline, guards, sharding over devices[], deferred slots), a candidate record per CU, and -- dec_opt / d_decisions_opt != NULL -- the decision record beside
 * it.  Logits and decision records are bit-identical to what the existing twins return under the same policy and gate.  d_candidates: n x 40 bytes of DEVICE
 * memory.  A deferred batch carries candidate records once a policy is set or a candidate call has been made for the size on this context;
 * mlt_wait_candidates on a batch that was FLUSHED before either returns MLT_ERR_ARG (a ticket still accumulating is launched with them). */
int mlt_predict_candidates(mlt_ctx *ctx, const int16_t *org, int org_stride, const int16_t *pred, int pred_stride,
                           int size, int32_t poc, int32_t qp, mlt_candidates *out, mlt_decision *dec_opt, float *logits_opt);
int mlt_predict_batch_candidates(mlt_ctx *ctx, int n, int size, const int16_t *org, const int16_t *pred,
                                 const int32_t *poc, const int32_t *qp, mlt_candidates *out, mlt_decision *dec_opt, float *logits);
int mlt_predict_batch_device_candidates(mlt_ctx *ctx, int n, int size, const void *d_org, const void *d_pred,
                                        const void *d_poc, const void *d_qp, void *d_candidates, void *d_decisions_opt, void *d_logits);
int mlt_wait_candidates(mlt_ctx *ctx, int size, mlt_ticket ticket, mlt_candidates *out, mlt_decision *dec_opt, float *logits_opt);

/* ---- Device-resident pictures: predict CUs by position, gathered on the GPU (new exports; MLT_ABI_VERSION stays 4) ----
 * Every entry point above takes CUT-OUT CUs.  A caller that evaluates whole pictures (lookahead / pre-analysis, a sweep of a gate or candidate policy over real
 * sequences, frames that already sit in HBM) keeps the two luma planes on the device instead -- the original and the prediction, one mlt_picture each -- and names
 * CUs by the position of their top-left luma sample: one upload per frame serves every CU size, and a device kernel (picture_gather) cuts the CUs out into the dense
 * planes the batch path consumes.  The network kernels are the batch path's: every result is bit-identical to mlt_predict_batch* on the same CUs, whatever the
 * positions' alignment (the gathered planes are always aligned, so they always run the quad-fetching kernels).  The encoder's per-CU call gains nothing measurable from
 * pictures.
 * Geometry: 16 <= width, height <= 16384, else MLT_ERR_ARG.  A picture belongs to the context it was made on (for a single device of a multi-device context: the one
 * mlt_device_ctx returns) and every call below takes that context. */
typedef struct mlt_picture mlt_picture;   /* opaque; one int16 (Pel) luma plane in device memory, owned by a context */

/* Allocates the plane on EVERY device of a multi-device context (content undefined until the first upload).  Freed by mlt_picture_destroy or mlt_shutdown. */
int mlt_picture_create(mlt_ctx *ctx, int width, int height, mlt_picture **out);
/* Host -> device, height rows of width Pels, `stride` >= width in elements; a picture made by mlt_picture_create only.  Copies on each device's context stream (with
 * mlt_set_stream: the caller's) and returns once the host buffer may be reused.  May be called again on the same picture (the next frame, same geometry) without
 * reallocation; a later mlt_predict_at on the same context sees the new content (stream order). */
int mlt_picture_upload(mlt_ctx *ctx, mlt_picture *pic, const int16_t *plane, int stride);
/* A plane the caller already holds in DEVICE memory: no copy, the caller keeps ownership (mlt_picture_destroy / mlt_shutdown release the handle only) and orders its own
 * writes before the calls that read it.  Any base address with 2-byte alignment and any stride >= width; the declared extent is (height - 1) * stride + width elements
 * from d_plane and no byte outside it is ever read.  Single-device contexts only: MLT_ERR_ARG on a context with peers (use mlt_device_ctx(ctx, i)). */
int mlt_picture_wrap_device(mlt_ctx *ctx, const void *d_plane, int stride, int width, int height, mlt_picture **out);
int mlt_picture_destroy(mlt_ctx *ctx, mlt_picture *pic);

/* n CUs of size x size at xy[i] = {x, y} (top-left luma sample) of the picture pair; xy / poc / qp and the outputs are HOST arrays, synchronous like mlt_predict_batch.
 * Outputs as on the batch twins: split modes, logits (n x mlt_num_logits(size)), decision records, candidate records -- at least one of them non-NULL, else MLT_ERR_ARG.
 * Both pictures must belong to ctx and have equal width and height (else MLT_ERR_ARG); the size must be loaded (else MLT_ERR_SIZE_DISABLED).  Every position must
 * satisfy 0 <= x, x + size <= width, 0 <= y, y + size <= height: ALL positions are checked on the host BEFORE anything is enqueued; on a violation the call returns
 * MLT_ERR_ARG, leaves the outputs untouched and names the offending index through mlt_last_error.  Any x / y is accepted, not only multiples of the size, and so are
 * overlapping and duplicate positions.  n == 0 returns MLT_OK.  Confidence gate, candidate policy and all three guards apply exactly as on mlt_predict_batch* of that
 * size.  Processed in chunks of the context's pass size (4096 CUs); on a multi-device context in contiguous shards, one host thread per device. */
int mlt_predict_at(mlt_ctx *ctx, int size, const mlt_picture *org, const mlt_picture *pred, int n, const int32_t *xy, const int32_t *poc, const int32_t *qp,
                   int32_t *split_mode_opt, float *logits_opt, mlt_decision *dec_opt, mlt_candidates *cand_opt);

/* ---- QP sweeps: one network pass, the heads under up to 32 QPs per CU (new exports; MLT_ABI_VERSION stays 4) ----
 * "What would this frame's split prior be at QP 27, 32, 37?"  poc and qp enter the network in the heads only, so a sweep runs the conv trunk ONCE per CU and the
 * heads once per point of qps[] -- not n_qps full calls.  poc stays per CU (the CUs of a call may come from different frames); qps[0 .. n_qps) is a HOST array that
 * applies to every CU: 1 <= n_qps <= MLT_SWEEP_MAX_QPS, any values in any order, duplicates and negative values included.
 * OUTPUTS are slab-major: element (q, i) of the split modes, decision records and candidate records lives at index q * n + i, the logits of (q, i) start at
 * (q * n + i) * mlt_num_logits(size); every array holds n_qps * n elements.  At least one output must be non-NULL.
 * CONTRACT: slab q is byte for byte what the twin without a sweep returns on the same CUs with every qp[i] = qps[q], under the same gate, candidate policy, flags and
 * tier -- the twin of the device entry is mlt_predict_batch_device and its decision / candidate forms, the twin of the picture entry is mlt_predict_at.  The guards
 * see the logits, so whether a CU is re-evaluated exactly depends on the point: the exact re-run covers the CUs flagged under ANY point, and its results replace
 * the fast ones only in the slabs where that CU was flagged.
 * guard_reruns (mlt_arith_info) grows by the number of DISTINCT CUs re-evaluated -- the size of that union, which is what ran: at most the sum and at least the
 * maximum of what the n_qps twin calls would add.
 * ERRORS: everything is checked before anything is enqueued, and on an error the outputs stay untouched.  MLT_ERR_ARG: NULL ctx, NULL qps, n_qps out of range, no
 * output at all and, on the picture entry, everything its twin checks (the offending position's index is named through mlt_last_error); MLT_ERR_SIZE_DISABLED: a
 * size that is not loaded.  n == 0 returns MLT_OK.
 * Chunked by the context's pass size like the twins; the device entry blocks once per chunk for the guards' 4-byte count, the picture entry is synchronous and, on a
 * multi-device context, sharded (every device writes its range of every slab).  A sweep call with candidate records does NOT make deferred batches carry candidate
 * records.  Partition trees under several QPs: mlt_predict_tree_sweep and (several pictures) mlt_predict_trees_sweep below.  Not there: host-dense, single-CU and deferred forms, a sweep over poc. */
#define MLT_SWEEP_MAX_QPS 32
int mlt_predict_batch_device_sweep(mlt_ctx *ctx, int n, int size, const void *d_org, const void *d_pred, const void *d_poc, const int32_t *qps /* HOST */, int n_qps,
                                   void *d_split_opt, void *d_logits_opt, void *d_decisions_opt, void *d_candidates_opt);
int mlt_predict_at_sweep(mlt_ctx *ctx, int size, const mlt_picture *org, const mlt_picture *pred, int n, const int32_t *xy, const int32_t *poc,
                         const int32_t *qps, int n_qps, int32_t *split_opt, float *logits_opt, mlt_decision *dec_opt, mlt_candidates *cand_opt);

/* Pure host, no context: the COMPLETE CUs of the size-aligned grid in raster order -- (width / size) * (height / size) positions; the partial CUs at the right and
 * bottom border are left out (VTM splits them implicitly).  Returns the total count and writes min(count, cap) entries of {x, y} to xy; xy == NULL with cap == 0 is
 * the size query.  0 for an unsupported size or a picture smaller than the size. */
int mlt_grid_positions(int width, int height, int size, int32_t *xy, int cap);

/* ---- Partition trees of a picture: quadtree descent on the device (new exports; MLT_ABI_VERSION stays 4) ----
 * What a whole-picture caller wants from a multi-level tree network: evaluate the top_size CUs of a picture pair, evaluate the four half-size children only where
 * the network says "quad split", and so on down to min_size.  The descent rule is the reference's own: head [2] of the 128 model, class 1, is QT
 * (mlt_ctu_or_pq_dataset.py:17); the CU models' default head [0] returns 0 / 1 and EncModeCtrl::setNewModeList reads 1 as PartSplit 1 = QT (EncCu.cpp:913-921,
 * EncModeCtrl.cpp:110-149); square children come only from QT and the network only takes square CUs (EncCu.cpp:801).  The whole descent stays on the device: per
 * level the node list is compacted by a device kernel (tree_expand), the children's positions never visit the host, and the only host traffic per level is one
 * 4-byte count.  Every network launch is the one mlt_predict_at makes on the same positions, so every node's result is bit-identical to that call's.
 *
 * LEVELS    top_size, top_size / 2, ... min_size (depth 0, 1, ...).
 * ROOTS     of level top_size: the complete CUs of its aligned grid in raster order (mlt_grid_positions).  Of a lower level S: the complete S-aligned CUs whose
 *           enclosing 2S-aligned block is NOT complete (it crosses the right or bottom border), in raster order; flags bit 0 set, parent = -1.  A partial CU is
 *           split implicitly, as VTM does at picture borders, so the tree covers every complete min_size block of the picture.  (424 x 280: 6 roots at 128, 0 at
 *           64, 8 at 32 -- the column x = 384 -- and 26 at 16 -- the row y = 256.)
 * ORDER     nodes run level by level; within a level the roots come first, then the children: in the order of their parents in the previous level, four per
 *           parent in z-order (TL, TR, BL, BR).  A complete parent's children are all complete, so a node has 0 or 4 children, contiguous from first_child.  The
 *           order is part of the contract.
 * DESCENT   a node of size S > min_size descends iff
 *             default                   split_mode >= 0 && (descend_mask[S] >> split_mode) & 1   -- a split withheld by the confidence gate does not descend
 *             MLT_TREE_BY_CANDIDATES    (cand_mask & descend_mask[S]) != 0                       -- an unsure CU that keeps every class descends
 *           min_size nodes are evaluated and never descend.
 * NODES     every node is evaluated: network, guards, confidence gate and candidate policy of its size exactly as in mlt_predict_at with the one (poc, qp) pair;
 *           the optional per-node logits, decision and candidate records are bit-identical to mlt_predict_at on the nodes' positions.  cand_mask is
 *           mlt_candidates.mask under the size's policy (default policy: 1 << raw_mode; every class of the head when a logit of the decision head is NaN).
 * LEAF MAP  one byte per complete 16 x 16 block, [height / 16][width / 16]: (log2(leaf size) - 4) | ((split_mode + 1) << 4) of the leaf that covers the block;
 *           0xFF for blocks no node covers (possible only with min_size > 16).
 * ERRORS    all arguments are checked before anything is enqueued and on any error every output stays untouched: ctx, cfg, nodes, n_nodes non-NULL and
 *           cfg->struct_size == sizeof(mlt_tree_config), top_size / min_size as below, descend_mask bits below the class count of the size's decision head,
 *           logit_stride >= 15 when logits_opt is given (else MLT_ERR_ARG); every size top..min loaded (else MLT_ERR_SIZE_DISABLED); both pictures of ctx and of
 *           equal geometry (else MLT_ERR_ARG); node_cap >= mlt_tree_max_nodes(width, height, top_size, min_size) (else MLT_ERR_ARG) -- capacity is a property of
 *           the geometry, never of the content.
 * Synchronous, like mlt_predict_at.  On a multi-device context the tree runs on devices[0] (the picture has a plane there); the bytes are a one-device context's. */
typedef struct mlt_tree_config {
  uint32_t struct_size;      /* = sizeof(mlt_tree_config); anything else -> MLT_ERR_ARG */
  int32_t  top_size;         /* 128 / 64 / 32 / 16; 0 => 128 */
  int32_t  min_size;         /* <= top_size; 0 => 16.  Every size top..min must be loaded, else MLT_ERR_SIZE_DISABLED */
  uint32_t descend_mask[4];  /* per size {128,64,32,16}: bit k = class k of that size's DECISION head means "quad split".
                                0 => 1u << 1 (QT of the reference's default heads).  A bit at or above the head's class count -> MLT_ERR_ARG */
  uint32_t flags;            /* MLT_TREE_BY_CANDIDATES */
  int32_t  poc, qp;          /* one pair for the whole picture */
} mlt_tree_config;
#define MLT_TREE_BY_CANDIDATES 0x1u

typedef struct mlt_tree_node {   /* 32 bytes, little-endian, no padding */
  int32_t  x, y;          /* top-left luma sample */
  int16_t  size;          /* 128 / 64 / 32 / 16 */
  int8_t   depth;         /* 0 at top_size */
  uint8_t  flags;         /* bit 0: border root (above) */
  int32_t  parent;        /* node index; -1 for roots */
  int32_t  first_child;   /* node index of the first of its FOUR children (contiguous, z-order: TL, TR, BL, BR); -1 = leaf */
  int32_t  split_mode;    /* as every entry point returns it (gate applied: -1 = withheld) */
  float    confidence;    /* mlt_decision.confidence */
  uint32_t cand_mask;     /* mlt_candidates.mask under the size's policy */
} mlt_tree_node;

/* Pure host, no context.  top_size / min_size as in mlt_tree_config: 0 => 128 / 16.
 * mlt_tree_max_nodes: the sum over the levels top..min of (width / S) * (height / S) -- the node count of a tree that descends everywhere; 0 on bad arguments
 * (a size outside 128 / 64 / 32 / 16, min_size > top_size, width or height outside 16 .. 16384).
 * mlt_tree_roots: the roots of level `size` (ROOTS above), counted and capped like mlt_grid_positions: returns the total count and writes min(count, cap)
 * entries of {x, y}; 0 on bad arguments or for a size above top_size. */
int mlt_tree_max_nodes(int width, int height, int top_size, int min_size);
int mlt_tree_roots(int width, int height, int top_size, int size, int32_t *xy, int cap);

/* The partition tree of the picture pair.  nodes[0 .. *n_nodes): the nodes in the contract's order; leaf_map_opt: (height / 16) * (width / 16) bytes or NULL;
 * logits_opt: node i at logits_opt + i * logit_stride, mlt_num_logits(node size) floats (the rest of the row is left alone), or NULL; dec_opt / cand_opt: one
 * record per node or NULL.  All HOST memory, node_cap entries each.  A call with cand_opt does not make deferred batches carry candidate records. */
int mlt_predict_tree(mlt_ctx *ctx, const mlt_picture *org, const mlt_picture *pred, const mlt_tree_config *cfg,
                     mlt_tree_node *nodes, int node_cap, int *n_nodes,
                     uint8_t *leaf_map_opt,
                     float *logits_opt, int logit_stride,
                     mlt_decision *dec_opt, mlt_candidates *cand_opt);

/* ---- Partition trees of SEVERAL picture pairs in one call (new exports; MLT_ABI_VERSION stays 4) ----
 * What a caller with a GOP, or with one original and several candidate predictions, in device memory wants: per level ONE network pass over the nodes of all
 * pictures, one guard re-run and one 4-byte count, instead of those per picture.  On the device a level of all pictures is one position list (picture 0's nodes,
 * then picture 1's, ...), gathered from the entries' planes by one launch; after the last level tree_pack_kernel permutes into the order below.  The descent, its
 * kernels (tree_expand, tree_raster) and its device arena are mlt_predict_tree's: that call is the same descent over one picture.
 *
 * ENTRIES   pics[0 .. n_pictures): an (org, pred) pair of ctx and the pair's poc / qp.  ALL pictures of a call have ONE width x height.  The same picture may
 *           appear in several entries (one original against several predictions) and entries may repeat.  cfg->poc / cfg->qp are NOT read.
 * RESULT    picture p's tree is nodes[first_node[p] .. first_node[p + 1]); first_node[n_pictures] is the total node count.  The slice is BYTE FOR BYTE what
 *           mlt_predict_tree returns for (pics[p].org, pics[p].pred) with the same cfg and cfg.poc / qp = pics[p].poc / qp: node order, parent / first_child
 *           (indices inside the slice: every slice is a self-contained tree), split_mode, confidence, cand_mask.  Leaf map p (leaf_maps_opt + p * (height / 16) *
 *           (width / 16)), the decision and the candidate records (one per node, at the node's index) are those of that single call as well.
 * LOGITS    node i at logits_opt + i * logit_stride; unlike mlt_predict_tree the WHOLE 15-float row of every node is written: the first mlt_num_logits(size)
 *           floats are the single call's, the rest zeros.
 * GUARDS    confidence gate, candidate policy, the three guards and MLT_TREE_BY_CANDIDATES act as in mlt_predict_tree; guard_reruns (mlt_arithmetic) grows by
 *           the sum of what the single calls add.
 * ERRORS    everything is checked before anything is enqueued and on any error every output stays untouched.  MLT_ERR_ARG: n_pictures outside 1 ..
 *           MLT_TREES_MAX_PICTURES; pics, cfg, nodes or first_node NULL; cfg->struct_size wrong; a picture NULL or of another context; unequal geometry inside a
 *           pair or between entries; node_cap < n_pictures * mlt_tree_max_nodes(width, height, top_size, min_size); logit_stride < 15 with logits_opt; sizes,
 *           masks and flags as in mlt_predict_tree.  MLT_ERR_SIZE_DISABLED: a size top..min is not loaded.  NULL ctx: MLT_ERR_ARG.
 * All arrays are HOST memory.  Synchronous.  On a multi-device context the call runs on devices[0], like mlt_predict_tree, with a one-device context's bytes. */
#define MLT_TREES_MAX_PICTURES 256
typedef struct mlt_tree_picture {   /* 24 bytes on LP64 */
  const mlt_picture *org, *pred;    /* both of ctx, all pictures of the call of ONE width x height */
  int32_t poc, qp;                  /* per picture */
} mlt_tree_picture;

int mlt_predict_trees(mlt_ctx *ctx, int n_pictures, const mlt_tree_picture *pics, const mlt_tree_config *cfg,
                      mlt_tree_node *nodes, int node_cap, int32_t *first_node /* [n_pictures + 1] */,
                      uint8_t *leaf_maps_opt /* [n_pictures][height/16][width/16] */,
                      float *logits_opt, int logit_stride, mlt_decision *dec_opt, mlt_candidates *cand_opt);

/* ---- Partition trees of ONE picture pair under SEVERAL QPs in one call (new export; MLT_ABI_VERSION stays 4) ----
 * The partition tree of a frame at QP 22 / 27 / 32 / 37: poc and qp enter the network in the heads only, so the conv trunk of a node is the same under every
 * point -- but the descents diverge per QP, and not as nested sets.  The call runs ONE descent over the UNION of the points' trees: every node that exists under
 * any point is evaluated once (one gather, one trunk pass, the heads under every point: the QP sweep's kernel), and one tree per point is carved out of the union.
 *
 * POINTS    qps[0 .. n_qps) is a HOST array, 1 <= n_qps <= MLT_SWEEP_MAX_QPS, any values in any order, duplicates and negative values included.  cfg->poc is the
 *           picture's poc; cfg->qp is NOT read.
 * RESULT    tree q is nodes[first_node[q] .. first_node[q + 1]); first_node[n_qps] is the total node count.  The slice is BYTE FOR BYTE what mlt_predict_tree
 *           returns for the pair with cfg.qp = qps[q] -- node order, parent / first_child (indices inside the slice), split_mode, confidence, cand_mask -- that is,
 *           slice q of mlt_predict_trees over n_qps entries {org, pred, cfg->poc, qps[q]}.  Leaf map q (leaf_maps_opt + q * (height / 16) * (width / 16)), the
 *           decision and the candidate records (one per node, at the node's index) are that call's.  The output format is mlt_predict_trees' throughout.
 * LOGITS    as mlt_predict_trees: node i at logits_opt + i * logit_stride, the WHOLE 15-float row written, zeros behind mlt_num_logits(size).
 * UNION     union_nodes_opt[l], l = 0 at top_size: the number of distinct nodes of that level on which the network ran -- the distinct (x, y) among the nodes of
 *           that size over all slices; 0 for the levels below min_size.
 * GUARDS    confidence gate, candidate policy, the three guards and MLT_TREE_BY_CANDIDATES act per point exactly as in mlt_predict_tree.  A node is re-evaluated
 *           with the exact arithmetic iff it is flagged under at least one point whose tree contains it, and the exact results replace the fast ones in those
 *           slabs only.  guard_reruns (mlt_arithmetic) grows by the number of distinct nodes re-evaluated: at least the maximum and at most the sum of what the
 *           n_qps single calls add.
 * ERRORS    everything is checked before anything is enqueued and on any error every output stays untouched.  MLT_ERR_ARG: cfg, qps, nodes or first_node NULL;
 *           n_qps outside 1 .. MLT_SWEEP_MAX_QPS; everything mlt_predict_tree checks (struct_size, sizes, masks, flags, logit_stride < 15 with logits_opt, a
 *           picture NULL, of another context or of another geometry); node_cap < n_qps * mlt_tree_max_nodes(width, height, top_size, min_size).
 *           MLT_ERR_SIZE_DISABLED: a size top..min is not loaded.  MLT_ERR_NOMEM: the device arena cannot be grown.  NULL ctx: MLT_ERR_ARG.
 * All arrays are HOST memory.  Synchronous.  On a multi-device context the call runs on devices[0] with a one-device context's bytes.
 * Several pictures times several QPs in one call: mlt_predict_trees_sweep below.  Not there: a sweep over poc, an asynchronous form. */
int mlt_predict_tree_sweep(mlt_ctx *ctx, const mlt_picture *org, const mlt_picture *pred, const mlt_tree_config *cfg,
                           const int32_t *qps /* HOST */, int n_qps,
                           mlt_tree_node *nodes, int node_cap, int32_t *first_node /* [n_qps + 1] */,
                           int32_t *union_nodes_opt /* [4]: nodes the network evaluated per level top.., 0 for levels below min_size */,
                           uint8_t *leaf_maps_opt /* [n_qps][height/16][width/16] */,
                           float *logits_opt, int logit_stride, mlt_decision *dec_opt, mlt_candidates *cand_opt);

/* ---- Partition trees of SEVERAL picture pairs under SEVERAL QPs each in one call (new export; MLT_ABI_VERSION stays 4, no struct changes) ----
 * A GOP in device memory and four base QPs: mlt_predict_trees' level-wide network passes over all pictures combined with mlt_predict_tree_sweep's union descent.
 * ONE descent over the unions of all entries: per level one node list -- entry 0's union segment, entry 1's, ... -- one gather and one trunk pass per union node,
 * the heads under every point, and n_pictures x n_qps trees carved out of the unions.
 *
 * ENTRIES   as mlt_predict_trees: 1 .. MLT_TREES_MAX_PICTURES pairs of ONE geometry, repeats allowed; an entry is the unit (entries that repeat a pair are not
 *           merged).  pics[p].qp is the entry's QP OFFSET (an RA GOP does not code every frame at the base QP).  cfg->poc and cfg->qp are NOT read.
 * POINTS    qps[0 .. n_qps) is a HOST array, 1 <= n_qps <= MLT_SWEEP_MAX_QPS, any values in any order, duplicates and negative values included.  The QP of
 *           entry p under point q is pics[p].qp + qps[q]; the sum is formed in 64 bits and must fit int32.
 * RESULT    slice s = p * n_qps + q is nodes[first_node[s] .. first_node[s + 1]); first_node[n_pictures * n_qps] is the total node count.  Slice s is BYTE FOR
 *           BYTE what mlt_predict_tree returns for (pics[p].org, pics[p].pred) with cfg.poc = pics[p].poc and cfg.qp = pics[p].qp + qps[q] -- that is, slice s
 *           of mlt_predict_trees over the n_pictures x n_qps entries {org_p, pred_p, poc_p, qp_p + qps[q]} in that order.  Leaf map s (leaf_maps_opt +
 *           s * (height / 16) * (width / 16)), the decision and the candidate records are that call's; logits are whole 15-float rows, zeros behind
 *           mlt_num_logits(size).
 * UNION     union_nodes_opt[p * 4 + l], l = 0 at top_size: the number of distinct nodes of that level on which the network ran for entry p; 0 below min_size.
 * GUARDS    confidence gate, candidate policy, the three guards and MLT_TREE_BY_CANDIDATES act per (entry, point) exactly as in mlt_predict_tree.  A union node
 *           is re-evaluated with the exact arithmetic iff it is flagged under at least one point it is alive under; the exact results replace the fast ones in
 *           those slabs only.  guard_reruns grows by the number of distinct (entry, node) pairs re-run: with a[p][q] what the single calls add,
 *           sum_p max_q a[p][q] <= growth <= sum_{p, q} a[p][q].
 * ERRORS    everything is checked before anything is enqueued and on any error every output stays untouched.  MLT_ERR_ARG: what mlt_predict_trees and
 *           mlt_predict_tree_sweep check; pics[p].qp + qps[q] outside int32; n_pictures * n_qps * mlt_tree_max_nodes(...) (64 bits) beyond int32 or above
 *           node_cap.  MLT_ERR_SIZE_DISABLED: a size top..min is not loaded.  MLT_ERR_NOMEM: the device arena cannot be grown.  NULL ctx: MLT_ERR_ARG.
 * All arrays are HOST memory.  Synchronous.  On a multi-device context the call runs on devices[0] with a one-device context's bytes.
 * Not there: a sweep over poc, per-picture point lists beyond the offset, pictures of different geometry in one call, an asynchronous form. */
int mlt_predict_trees_sweep(mlt_ctx *ctx, int n_pictures, const mlt_tree_picture *pics, const mlt_tree_config *cfg,
                            const int32_t *qps /* HOST */, int n_qps,
                            mlt_tree_node *nodes, int node_cap, int32_t *first_node /* [n_pictures * n_qps + 1] */,
                            int32_t *union_nodes_opt /* [n_pictures][4] */,
                            uint8_t *leaf_maps_opt /* [n_pictures][n_qps][height/16][width/16] */,
                            float *logits_opt, int logit_stride, mlt_decision *dec_opt, mlt_candidates *cand_opt);

/* ---- Prediction pictures on the device: block motion search + compensation (new exports; MLT_ABI_VERSION stays 4) ----
 * Every whole-picture call above takes an original AND a prediction picture, and a caller that holds originals only (lookahead, pre-analysis, a GOP in HBM) has no
 * prediction before an encode.  These calls make one on the device: from the current original and a reference picture by an integer-sample block motion search
 * followed by quarter-sample motion compensation, or by the compensation alone from a motion field the caller already has.  The result is written into a picture
 * made by mlt_picture_create, which every call above then takes as `pred`.  Everything is integer arithmetic with ONE stated rule, so the bytes are the same on
 * every device and equal to the numpy restatement fastintercu-vvc_amd/motion.py.
 * THIS IS A PRE-ANALYSIS PREDICTION WITH ITS OWN ROUNDING: both filter passes run at full int32 precision and round once, (v + 2048) >> 12.  It is NOT the
 * encoder's interpolation with its intermediate rounding and shifts, and not its merge / skip prediction.
 *
 * BLOCKS    block = 8, 16, 32 or 64 luma samples (0: 16).  bx = ceil(width / block), by = ceil(height / block); block (i, j) covers x in [i * block,
 *           min((i + 1) * block, width)) and likewise y: border blocks are clipped, every sample belongs to exactly one block.
 * FIELD     [by][bx][2] int16 {mvx, mvy} in QUARTER luma samples, raster order.  Every int16 value is legal.
 * REFERENCE SAMPLES are read with clamped coordinates in every rule:  R(x, y) = ref[clamp(y, 0, height - 1)][clamp(x, 0, width - 1)].
 * COMPENSATION  with the quarter-sample luma taps
 *             C[0] = {  0, 0,   0, 64,  0,   0, 0,  0 }
 *             C[1] = { -1, 4, -10, 58, 17,  -5, 1,  0 }
 *             C[2] = { -1, 4, -11, 40, 40, -11, 4, -1 }
 *             C[3] = {  0, 1,  -5, 17, 58, -10, 4, -1 }
 *           and, for a sample (x, y) of a block with vector (mvx, mvy):  ix = mvx >> 2, fx = mvx & 3 (arithmetic shift), likewise iy, fy;
 *             t_j = sum_k C[fx][k] * R(x + ix + k - 3, y + iy + j - 3)   for j = 0 .. 7
 *             v   = sum_j C[fy][j] * t_j
 *             dst(x, y) = clip(0, 1023, (v + 2048) >> 12)                 all in int32: |v| <= 112 * 112 * 32768 < 2^31.
 *           One formula serves all 16 fractions; for an integer vector it is clip(0, 1023, R(x + ix, y + iy)).
 * SEARCH    per block, over all (dx, dy) in [-range, range]^2:  SAD = sum over the block's samples of |cur(x, y) - R(x + dx, y + dy)| (the int16 values as they
 *           are, the sum in uint32), cost = SAD + lambda * (|dx| + |dy|).  The winner has the smallest key (cost, |dx| + |dy|, dy, dx), compared lexicographically
 *           with dy and dx as signed integers.  Its vector is (4 * dx, 4 * dy), its cost the block's cost.
 * ORDER     both calls enqueue on the context's stream(s): later calls on the same context see dst in stream order.  On a multi-device context both run on every
 *           device and dst has its plane on each (mlt_predict_at shards over them); the bytes are identical.  Destroying a picture that an enqueued call still
 *           reads or writes is safe: releasing a library-owned plane waits for the device, and of a wrapped picture only the handle goes.
 * ERRORS    everything is checked before anything is enqueued; on an error dst and the host outputs stay untouched.  MLT_ERR_ARG: a NULL ctx, cfg, picture or
 *           field; a struct_size other than sizeof(mlt_motion_config); block, range, lambda or flags out of range; a picture of another context; pictures of
 *           unequal width or height; dst equal to ref or cur; a dst made by mlt_picture_wrap_device (that plane is the caller's and const).  No weights are needed.
 * Sub-sample refinement and a per-block choice among several references: mlt_picture_predict_refs / mlt_picture_compensate_refs below.
 * Not there: bi-prediction, chroma, motion fields that stay in device memory across calls. */
typedef struct mlt_motion_config {   /* 20 bytes */
  uint32_t struct_size;  /* = sizeof; anything else -> MLT_ERR_ARG */
  int32_t block;         /* 8 / 16 / 32 / 64; 0 => 16 */
  int32_t range;         /* search only: candidates dx, dy in [-range, range], 0 <= range <= 64 */
  int32_t lambda;        /* search only: cost = SAD + lambda * (|dx| + |dy|), 0 <= lambda <= 65535 */
  uint32_t flags;        /* 0; anything else -> MLT_ERR_ARG */
} mlt_motion_config;

/* Pure host, no context: returns bx * by and writes bx / by (either may be NULL); 0 on bad arguments (a block other than 8 / 16 / 32 / 64, a width or height
 * outside 1 .. 16384). */
int mlt_motion_blocks(int width, int height, int block, int *bx, int *by);
/* The inverse of mlt_picture_upload: height rows of width Pels from devices[0]'s plane, after the context stream's earlier work; synchronous.  `stride` >= width
 * in elements; no host element outside the rows' first `width` entries is written.  Owned and wrapped pictures alike. */
int mlt_picture_download(mlt_ctx *ctx, const mlt_picture *pic, int16_t *plane, int stride);
/* dst <- the compensation of ref with the HOST field mv ([by][bx][2], cfg->block; range and lambda are not read).  Returns once mv may be reused, like
 * mlt_picture_upload. */
int mlt_picture_compensate(mlt_ctx *ctx, const mlt_picture *ref, const mlt_motion_config *cfg, const int16_t *mv /* HOST */, mlt_picture *dst);
/* The search of cur in ref, then dst <- the compensation of ref with the found field: dst is byte for byte what mlt_picture_compensate writes for (ref, cfg,
 * mv_out).  mv_out_opt ([by][bx][2]) and cost_out_opt ([by][bx]) are HOST arrays or NULL; with either the call is synchronous, with neither it returns after
 * enqueueing. */
int mlt_picture_predict(mlt_ctx *ctx, const mlt_picture *cur, const mlt_picture *ref, const mlt_motion_config *cfg, mlt_picture *dst,
                        int16_t *mv_out_opt, uint32_t *cost_out_opt);

/* ---- Quarter-sample refinement and per-block reference choice (new exports; MLT_ABI_VERSION stays 4; nothing above changes) ----
 * mlt_picture_predict stops at an integer-sample vector into one reference.  These two calls add the next rungs with ONE selection rule: the integer winner of
 * every reference is refined over a window of fractional vectors, evaluated on the COMPENSATION RULE'S OWN OUTPUT, and each block takes the best (reference,
 * vector).  Integer arithmetic only: the bytes are the same on every device and equal to motion.refine / motion.compensate_refs / motion.predict_refs.
 * Blocks, the field layout, R(x, y) (clamped), the taps C[f] and  P_mv(x, y) = clip(0, 1023, (v + 2048) >> 12)  are exactly those of COMPENSATION above;
 * P_mv^r is P_mv computed from refs[r].
 *
 * REFERENCES  refs[0 .. n_refs), 1 <= n_refs <= MLT_MOTION_MAX_REFS.  The same picture may be listed more than once.
 * STEP 1      integer search, per reference r: SEARCH above, unchanged (its own rule, key and cost) -> (dx_r, dy_r).
 * STEP 2      refinement, per reference r: the candidates mv = (4 dx_r + qx, 4 dy_r + qy) with qx, qy in Wd(subpel),
 *               Wd(0) = { 0 }     Wd(1) = { -2, 0, 2 }     Wd(2) = { -3, ..., 3 }
 *             -- 1, 9 or 49 candidates, exhaustive, no staged descent: no evaluation order can matter.
 *               SADP   = sum over the block's clipped samples of |cur(x, y) - P_mv^r(x, y)|   (cur: the int16 values as they are)
 *               cost_q = 4 * SADP + lambda * (|mvx| + |mvy|)   in uint32: 4 * 4096 * 33791 + 65535 * 518 < 2^32.
 * STEP 3      the winner over all (r, mv) has the smallest (cost_q, |mvx| + |mvy|, r, mvy, mvx), compared lexicographically with mvy and mvx signed -- as one
 *             unsigned 64-bit key: cost_q << 32 | l1 << 22 | r << 20 | (mvy + 512) << 10 | (mvx + 512)   (|mv| <= 259, l1 <= 518).
 *             Outputs: the block's vector, its reference index, its cost_q.
 * STEP 4      dst is, block by block, P_mv^r of the winner.
 * CONSEQUENCES  cost_q is in QUARTER units and on CLIPPED samples: it equals 4 x the integer search's cost only while every reference sample the block touches
 *             lies in 0 .. 1023.  With subpel = 0 and n_refs = 1 the vector field and dst are byte for byte mlt_picture_predict's.
 * CONTRACTS   dst of mlt_picture_predict_refs is byte for byte mlt_picture_compensate_refs(refs, mv_out, ref_out); with n_refs = 1 also
 *             mlt_picture_compensate(refs[0], mv_out).
 * ORDER       as above: a call with a host output is synchronous, one without returns after enqueueing, in stream order; every device of a multi-device context
 *             runs the call and produces identical bytes.  No weights are needed.
 * ERRORS      everything is checked before anything is enqueued; on an error dst and the host outputs stay untouched.  MLT_ERR_ARG: everything the calls above
 *             refuse, for EVERY reference; a struct_size other than sizeof(mlt_motion_refs_config); n_refs outside 1 .. MLT_MOTION_MAX_REFS; subpel outside
 *             0 .. 2; a ref_idx entry >= n_refs (mlt_last_error names the block); dst equal to cur or to any reference.
 * Not there: bi-prediction, chroma, motion fields that stay in device memory across calls. */
#define MLT_MOTION_MAX_REFS 4
typedef struct mlt_motion_refs_config {   /* 24 bytes */
  uint32_t struct_size;  /* = sizeof; anything else -> MLT_ERR_ARG */
  int32_t block;         /* as mlt_motion_config */
  int32_t range;         /* search only, as mlt_motion_config */
  int32_t lambda;        /* search only: the integer search's lambda AND cost_q's, 0 <= lambda <= 65535 */
  int32_t subpel;        /* search only: 0 integer / 1 half / 2 quarter refinement window */
  uint32_t flags;        /* 0; anything else -> MLT_ERR_ARG */
} mlt_motion_refs_config;
/* Steps 1 - 4.  mv_out_opt ([by][bx][2]), ref_out_opt ([by][bx]) and cost_out_opt ([by][bx], cost_q) are HOST arrays or NULL; with any of them the call is
 * synchronous, with none it returns after enqueueing. */
int mlt_picture_predict_refs(mlt_ctx *ctx, const mlt_picture *cur, const mlt_picture *const *refs, int n_refs, const mlt_motion_refs_config *cfg,
                             mlt_picture *dst, int16_t *mv_out_opt, uint8_t *ref_out_opt, uint32_t *cost_out_opt);
/* Step 4 alone: dst <- block by block the compensation of refs[ref_idx[block]] with the HOST field mv (cfg->block; range, lambda and subpel are not read).
 * ref_idx_opt: HOST [by][bx], NULL = every block reads refs[0].  Returns once mv and ref_idx_opt may be reused. */
int mlt_picture_compensate_refs(mlt_ctx *ctx, const mlt_picture *const *refs, int n_refs, const mlt_motion_refs_config *cfg, const int16_t *mv /* HOST */,
                                const uint8_t *ref_idx_opt /* HOST */, mlt_picture *dst);

int mlt_synchronize(mlt_ctx *ctx);

/* Use an existing hipStream_t (e.g. the caller's) instead of the context's own stream; NULL switches back to a
 * stream owned by the context (mlt_predict replays its kernel chain from a hipGraph only on an owned stream). */
int mlt_set_stream(mlt_ctx *ctx, void *hip_stream);

/* Pinned host staging buffers for mlt_predict_batch. */
void *mlt_alloc_pinned(size_t bytes);
void mlt_free_pinned(void *p);

/* Number of logits returned per CU for `size` (9 for 128, 15 for 64/32/16, 0 if unsupported). */
int mlt_num_logits(int size);

/* Per-kernel device timing (HIP events on the context's stream): enable, run, then read.
 * mlt_profile_read fills up to `cap` entries; returns the number of distinct kernels. */
typedef struct mlt_kernel_time {
  char name[48];
  uint32_t launches;
  float total_ms;
  double flops;  /* algorithmic FLOPs summed over those launches */
  double bytes;  /* algorithmic HBM bytes (inputs + outputs + weights once) summed over launches */
} mlt_kernel_time;
int mlt_profile_enable(mlt_ctx *ctx, int on);
int mlt_profile_read(mlt_ctx *ctx, mlt_kernel_time *out, int cap);

const char *mlt_last_error(const mlt_ctx *ctx); /* ctx may be NULL: last init error */
int mlt_abi_version(void);
/* 16 hex digits: sha256 over the sources (fastintercu-vvc_amd/csrc/, sorted by name) this binary was built from -- what bench.py reports as
 * derived.source_sig and what the Python host side checks against the tree before it uses the library ("unsigned-build!!" for a build outside build.py). */
const char *mlt_build_signature(void);

/* Debug hook (host only: no device, no context): the per-conv kernels' launch table as text -- what the library would launch for every layer shape,
 * arithmetic and variant, and the packing view the host derives from it.  Returns the length written (NUL-terminated), or -1 when `cap` is too small. */
int mlt_debug_conv_table(char *out, size_t cap);

/* Release everything (natural home: EncCu::destroy, EncCu.cpp:160-206). NULL is allowed. */
void mlt_shutdown(mlt_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* MLTCNN_H */
