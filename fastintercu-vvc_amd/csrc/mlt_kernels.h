// mlt_kernels.h -- launch interface between the host runtime (mlt_runtime.h and its translation units) and mlt_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MLT_MAX_HEADS_K 4
#define MLT_MAX_LOGITS_K 16
// Flat-content guard statistic (round 3: widened from "exactly constant"): an aligned 4-pixel quad is NEAR-FLAT when the RANGE (max - min)
// of its four org values AND of its four |org - pred| values -- as the network sees them: uint16 cast, absdiff, clip to 10 bits --
// is <= MLT_FLAT_RANGE -- +-1 LSB dither, sensor noise on smooth areas, every exactly-constant area (sky, letterbox bars,
// screen content) -- or the four values are LINEAR to within one step (ramps of any slope); per plane either test may hold.  Content
// on which neighbouring pixels carry correlated fp16 rounding errors that the global pooling cannot average away.
// Round 4: a quad is EXACTLY FLAT when each plane is constant or exactly linear (range 0, or both second differences 0).  A CU is flagged
// when >= 1/8 of its quads are exactly flat (identical activations at every pixel: the error mechanism proper, 1.2 - 2.3e-3 measured on
// constant CUs whatever the weight arithmetic) OR >= 1/2 are near-flat.  With the single 1/8 rule on near-flat quads, 22 % of the CUs of
// the natural-statistics class (synth.natural_patches: smooth areas + sensor noise) were re-run exactly although their single-pass error
// is no larger than that of textured CUs (profiles/r04*_natural_probe.txt); the two-level rule flags 3 % of them, and the calibration
// set carries the content it lets through (a near-flat band over 40-48 % of the quads).
// Round 6: the range is 6, not 8.  Measured on nine seeded weight sets and the trained families in their shipped tiers WITHOUT the guard
// (scripts/r06_flat_guard_need_probe.py, profiles/r06i_flat_guard_need*.txt): what needs the guard is content whose variation stays near the
// first activations' fp16 step -- constant areas (1.5 - 2.7e-3), +-1 LSB dither (heavier tail, up to 9.5e-4), low-contrast texture of amplitude
// <= 4 (like texture for most sets, but ONE logit of 405,504 at 1.01e-3 in the most marginal tier when a range of 4 let that class through:
// profiles/r06j_tail_probe.txt) -- while the 2.3 - 3 % of the natural-statistics CUs the range of 8 flagged (near-flat fractions 0.50 - 0.72,
// made of quads of range 7 - 8: slow gradients + sensor noise) err like their unflagged neighbours (max 6.1e-4 against 7.4e-4): 125 exact
// re-runs per 4096-CU batch of natural scenes for nothing (1.02 M -> 0.83 M CU/s).  With 6 every class the rule was built for stays guarded
// (dither 100 % near-flat, amplitude-4 texture 69 - 73 %, ramps, constants) and natural scenes are flagged at 0 % (largest near-flat fraction 0.47).
#define MLT_FLAT_RANGE 6
#define MLT_FLAT_EXACT_SHIFT 16   // the per-CU statistic packs both counts: near-flat quads in bits 0-15, exactly flat quads in bits 16-31

struct ConvArgs {
  const void *x;      // input  [n][Hin][Hin][CIN]  fp16 NHWC
  void *y;            // output [n][Hout][Hout][COUT] fp16 NHWC
  const void *w;      // packed fp16 weights (mlt_model.cpp: pack_conv)
  const float *bias;  // folded BN bias per output channel
  const void *res;    // optional residual, same shape as y (NULL: none)
  const void *zero;   // >= 64 KiB of zeros (DMA staging fetches padding from here)
  int n;
  int ntiles;                  // logical tiles (grid.x may be smaller: workgroups are persistent over tiles)
  int hin_l, hout_l;           // log2 of input / output height (= width)
  int tw_l, th_l, spw_l;       // log2 of tile width, tile height, samples per workgroup
  int ph, pw, rp, half;        // patch rows, cols, row pitch (pixels), parity-split half width
  uint32_t pw_magic, ph_magic, rp_magic; // ceil(2^32 / d), d >= 2
  int patch_bytes;             // LDS bytes reserved for the patch (multiple of 1024)
  int relu;
  int y_c16;                   // 1: y is written chunk-major, [n][COUT/16][Hout*Hout][16] -- the layout the next stage's whole-stage
                               // kernel stages its 16-channel input patches from (contiguous 32-byte pixels instead of 32-byte pieces
                               // of 128/256-byte NHWC pixels: measured 2.2x HBM over-fetch on those)
  int ysc_c16;                 // 1: y_sc chunk-major as well (its reader is the 64-channel chain's residual load: one cache line per
                               // lane quad instead of four)
  float acc_scale;             // accumulators are multiplied by this before the bias (weights are stored * 2^s)
  // SC variant: second output = bn(conv1x1_stride2(x)) (projection shortcut, arch:44-50)
  void *y_sc;
  const float *bias_sc;
  // fp32 global-average-pool partial sums [n][gap_slots][COUT] (NULL: none); gap_l = log2(lanes per sample)
  float *gap;
  int gap_slots, gap_l;
  // exact mode (NSPLIT == 2): byte offsets from each hi plane to its lo plane
  size_t x_lo_off, y_lo_off, res_lo_off, ysc_lo_off, w_lo_off;  // exact arithmetic: byte offsets hi plane -> lo plane (x_lo_off / res_lo_off == 0: that input has no lo plane, its lo part is zero)
  int lo8_scale;               // NSPLIT == 5 (hi fp16 + FP8 lo plane): E8M0 scale byte of the lo plane, replicated (mlt_model.h: lo8_exp)
  int xl_sa0, xl_sa1, xl_sb1;  // NSPLIT == 6 (exact-lite): replicated E8M0 bytes -- A operand lanes 0-31 (e4m3 Wl: 127 - xl_ewl) / lanes 32-63 (e4m3 Wh: 127 - xl_ewh),
                               // B operand lanes 32-63 (e4m3 Xl: 127 - MLT_XL_LO_EXP); B lanes 0-31 (e4m3 Xh) are unscaled
};

struct ConvCfg { int kc, ct, mt, gt, dma, mt_dma, lat, gt_w2; };  // gt_w2: taps per weight step of the layer's (nsplit 4, DEFAULT) row -- the hi+lo-WEIGHTS tier on the fast tiling --, 0 where the layer has none  // cin chunk, couts / pixels per workgroup, taps per weight step, LDS-DMA staging variant (0 none, 1 resident, 2 ring) and its pixels per workgroup

struct Stem5Args {
  const int16_t *org, *pred;   // Pel planes
  long org_row_stride, org_cu_stride, pred_row_stride, pred_cu_stride;  // in elements
  const void *w;               // [plane][7 k-steps][64 lanes][8 halves]: 5 composed 5x5(+border) steps, 2 shortcut steps
  const float *bias, *bias_sc;
  void *y, *y_sc;              // t and sc, [n][S/2][S/2][32] fp16
  size_t y_lo_off, ysc_lo_off, w_lo_off;
  float acc_scale;
  int n, s_l, hout_l, tw_l, th_l, spw_l;
  int rh, rw, halfw;           // raw patch rows, cols, half row pitch (columns are parity-split)
  uint32_t rw_magic, rh_magic;
};

struct Block32Args {
  const void *x;               // block input  [n][H][H][32] fp16 (also the residual)
  void *y;                     // block output [n][H][H][32] fp16
  const void *w1, *w2;         // packed fp16 weights of conv1 / conv2 (18 KiB each, fast mode layout)
  const float *bias1, *bias2;  // folded BN biases
  int n, h_l, ntiles;          // H = 1 << h_l (>= 32); tiles of 16 x 32 output pixels (hi+lo-weights form: 8 x 32)
  // hi+lo-weights form: byte offsets hi plane -> lo plane, accumulator scales (weights are stored * 2^s)
  size_t w1_lo_off, w2_lo_off;
  float scale1, scale2;
};

struct StemBlockArgs {
  const int16_t *org, *pred;   // Pel planes
  long org_row_stride, org_cu_stride, pred_row_stride, pred_cu_stride;  // in elements
  const void *w;               // composed first-layer weights (Stem5Args.w layout, fast plane)
  const void *w2;              // layer0.0.conv2 packed weights (18 KiB)
  const float *bias, *bias_sc, *bias2;
  void *y;                     // b0 [n][H][H][32] fp16
  int32_t *flat;               // NULL, or [n] zero-initialised: += number of near-constant (MLT_FLAT_RANGE) 4-pixel quads of each CU
                               // (flat-content guard; same statistic as flat_stat_kernel)
  float acc_scale;             // composed-weight storage scale (2^-12)
  int n, hout_l, ntiles;       // H = 1 << hout_l (>= 32), picture 2H x 2H; tiles of 16 x 32 output pixels
  // hi+lo-weights form: byte offsets hi plane -> lo plane of w / w2, accumulator scale of conv2
  size_t w_lo_off, w2_lo_off;
  float scale2;
};

// All of layer0 of 128 x 128 CUs in one launch (layer0_stream_kernel, round 5): stem_block_kernel's and block32_kernel's arithmetic, streamed row by
// row through LDS rings by one persistent 16-wave workgroup per CU -- b0 never reaches HBM, no halo is staged or computed twice.
#define MLT_L0F_LDS_BYTES 161040 /* ... with the stride-2 conv of layer1 as a fifth stage: rings of 6 / 8 / 6 / 6 rows, 64 + 64 more biases */
#define MLT_L0_LDS_BYTES 145872  /* 3 rings x 8 map rows + zero row (66 px x 80 B), 16 + 1 raw rows (136 dwords), biases, 4 KiB of first-layer k-steps, 2 counters */
struct Layer0Args {
  const int16_t *org, *pred;   // Pel planes, 128 x 128 per CU
  long org_row_stride, org_cu_stride, pred_row_stride, pred_cu_stride;  // in elements (8-byte aligned quads: see stem_block_kernel)
  const void *w;               // composed first-layer weights (StemBlockArgs.w)
  const void *w2, *w3, *w4;    // layer0.0.conv2, layer0.1.conv1, layer0.1.conv2: packed fp16, 18 KiB each (fast plane)
  const float *bias, *bias_sc, *bias2, *bias3, *bias4;
  void *y;                     // layer0 output [n][64][64][32] fp16
  int32_t *flat;               // NULL, or [n] zero-initialised (flat-content guard statistic, as StemBlockArgs.flat)
  float acc_scale;             // composed-weight storage scale
  int n;
  // fifth stage (layer0_stream_kernel<true>): layer1.0.conv1 + shortcut, packed as for conv_mfma_kernel<32, 64, 2, ...> (ct 64, kc 32, 10 taps)
  const void *w5;
  const float *bias5, *bias5_sc;
  void *y_t, *y_sc;            // t [n][32][32][64] fp16 NHWC; sc chunk-major [n][4][1024][16] (ConvArgs.ysc_c16: what the 64-channel chain reads)
                               // layer0_stream_xs_kernel: y_sc receives xs [n][32][32][32] fp16 = out[2Y][2X][.] instead (Layer1Args.sc)
  float scale5;
};

// The three stride-1 convs of layer1 (64 channels at 32 x 32) as a streaming pipeline (layer1_stream_kernel, round 5): chain_kernel<64>'s
// arithmetic, weights resident in registers, rows through LDS rings, b0 never in HBM.
#define MLT_L1_LDS_BYTES 159008  /* rings of 4 / 8 / 4 map rows + zero row (34 px x 144 B), 2 sc rows, 16 accumulator hand-over blocks of 4 KiB, biases */
#define MLT_L1X_LDS_BYTES 159264 /* layer1_stream_xs_kernel: + the shortcut's 64 biases */
struct Layer1Args {
  const void *t;               // [n][32][32][64] fp16 NHWC: relu(bn1(conv1 x)) of layer1.0
  const void *sc;              // the projection shortcut, chunk-major [n][4][1024][16] fp16 (ConvArgs.ysc_c16)
                               // layer1_stream_xs_kernel: its INPUT xs [n][32][32][32] fp16 (layer0's output at even rows and columns) and, to compute it here,
  const void *w_sc;            // ... layer1.0.conv1's packed weights (Layer0Args.w5: the shortcut is their tap 9),
  const float *bias_sc;        // ... the shortcut's 64 folded BN biases
  float scale_sc;              // ... and that conv's accumulator scale (Layer0Args.scale5)
  const void *w[3];            // layer1.0.conv2, layer1.1.conv1, layer1.1.conv2: packed fp16 (ct 64, kc 64: 72 KiB each)
  const float *bias[3];
  float scale[3];
  void *y;                     // stage output [n][32][32][64] fp16, NHWC or chunk-major (y_c16)
  int y_c16;
  float *gap;                  // fp32 GAP partial sums [n][gap_slots][64]
  int gap_slots, n;
};

// Fused chain of stride-1 3x3 convs on whole samples (chain_kernel): the BasicBlock tail of a stage,
//   b0 = relu(bn2(conv2(t)) + sc) ; t1 = relu(bn1(conv1(b0))) ; out = relu(bn2(conv2(t1)) + b0)      (arch:52-57)
// with every intermediate kept on chip (activations in LDS, b0 as the residual in registers).
struct ChainConv {
  const void *w;       // packed fp16 weights (same packing as the stand-alone conv of this layer)
  size_t w_lo_off;     // hi+lo-weights form (chain_kernel<..., W2>): byte offset of the lo plane
  int lo8_scale;       // ... with an FP8 lo plane (LO8): the E8M0 scale byte 127 - lo8_exp, replicated into all four bytes
  const float *bias;   // folded BN bias
  float acc_scale;
  int relu;
  int res_mode;        // 0 none, 1 from `res` (HBM, same layout as the output), 2 from the tile saved by an earlier conv
  int save;            // 1: keep this conv's activated output tile in registers as a later conv's residual
  const void *res;
  void *y;             // non-final conv: also write the activated output to HBM (same bytes as NHWC, but in the writing wave's own
                       // order: it is read back only by that wave) -- the later residual when the chain does not keep it in
                       // registers (64-channel stage: 128 accumulator registers leave no room)
};
struct ChainArgs {
  const void *x;       // [n][H][H][C] fp16: input of the first conv; S2 variant: the STAGE input [n][2H][2H][C/2]
  // S2 variant (whole stage in one launch): the stage's first conv -- 3x3 stride 2 + its 1x1 stride-2 projection shortcut
  // (arch:44-55) -- runs in front of the chain; its weights are packed for 16-channel chunks (mlt_model.cpp: conv1_s2c)
  const void *s2_w;
  const float *s2_bias, *s2_bias_sc;
  float s2_scale;
  const void *zero;    // >= 64 KiB of zeros (padding source of the patch DMA)
  ChainConv cv[3];
  int nconv;           // 3: the launchers refuse any other, no kernel reads it
  void *y;             // [n][H][H][C] fp16 output of the last conv, or NULL (only the GAP sums are needed)
  int y_c16;           // y chunk-major (ConvArgs.y_c16)
  int x_c16;           // S2: the stage input x is chunk-major
  int res0_c16;        // cv[0].res (the shortcut sc from HBM) is chunk-major (ConvArgs.ysc_c16)
  float *gap;          // fp32 GAP partial sums of the last conv's output [n][gap_slots][C], or NULL
  int gap_slots, gap_l;
  int n;
};
hipError_t mlt_launch_chain(int c, int h, bool with_s2, bool oob_zero, bool w2, const ChainArgs &a, int grid_x, hipStream_t st);  // oob_zero: see mlt_probe_lds_oob; w2: hi+lo weights (two planes, no stride-2 front conv, oob_zero only)
// The whole 256-channel stage (8 x 8 maps, stride-2 conv + shortcut inside) with both cout passes per wave (stage256_wide_kernel): the same bits as
// mlt_launch_chain(256, 8, true, true, false, ...), which stays the form of devices that fail the LDS probe.
hipError_t mlt_launch_stage256_wide(const ChainArgs &a, int grid_x, hipStream_t st);
bool mlt_chain_supported(int c, int h);
hipError_t mlt_probe_lds_oob(int *d_ok, hipStream_t st);  // *d_ok = 1 iff DS reads beyond the LDS allocation return zeros on this device
bool mlt_stage_supported(int c, int h);  // ... including the stage's stride-2 conv + shortcut (S2 variant)

// Decision record of one CU (include/mltcnn.h: mlt_decision -- same 48 bytes; mlt_runtime.h asserts the layout).
struct DecisionRec {
  int32_t split_mode, raw_mode;
  float confidence, margin;
  int32_t level_mode[MLT_MAX_HEADS_K];
  float level_conf[MLT_MAX_HEADS_K];
};
// Confidence gate guard: with the decision guard and a gate both on, a CU whose decision-head confidence lies within this fraction of the
// tolerance of the gate's threshold is re-evaluated exactly, so that fp16 rounding never decides which side of the gate it falls on.  Two logits
// within tol of the reference move a softmax probability by at most tol / 2: d p_top = p_top sum_j p_j (d l_top - d l_j), the differences move
// by at most 2 tol, and sum_{j != top} p_top p_j = p_top (1 - p_top) <= 1/4.  The decision guard uses 3 x tol where 2 x is the bound (the
// admission of the fast arithmetic is statistical); the same factor 1.5 on tol / 2 gives 0.75 tol.
#define MLT_CONF_BAND_FRAC 0.75f

// Candidate record of one CU (include/mltcnn.h: mlt_candidates -- same 40 bytes; mlt_runtime.h asserts the layout): the smallest set of classes of the decision
// head that carries `coverage` of the softmax probability (head_candidates, mlt_tail_kernels.inc).
#define MLT_MAX_CAND_K 6   // classes of the widest head (lvl4 of the CU models)
struct CandRec {
  uint32_t mask;
  int32_t count;
  int8_t order[8];
  float prob[MLT_MAX_CAND_K];
};

// The thresholds of the parity guards' selection rule (guard_rule, mlt_tail_kernels.inc -- the one statement of the rule; the host fills them in guard_thresholds).
// A CU is flagged -- re-evaluated with the exact arithmetic -- when
//   its count of EXACTLY flat quads (statistic >> MLT_FLAT_EXACT_SHIFT) >= flat_thr or its count of near-flat quads (statistic & 0xFFFF) >= near_thr (flat guard), or,
//   margin > 0: top1 - top2 of the decision head is not >= margin or a logit is NaN (decision guard), and with it
//     conf_band > 0: |confidence - min_conf| is not >= conf_band (the gate guard, MLT_CONF_BAND_FRAC), and
//     cand_band > 0: a proper prefix sum lies within cand_band of cand_cov, or classes are dropped over a logit gap below margin (the candidate guard), or,
//   mag_thr > 0: its logit magnitude is not <= mag_thr (round 6: the magnitude guard, mlt_runtime.h: SizeState.mag_thr).
struct GuardRule {
  int flat_thr, near_thr;
  float margin, mag_thr, conf_band, cand_band;
};

struct HeadArgs {
  const float *gap[MLT_MAX_HEADS_K];  // GAP partial sums [n][slots][C] fp32 (written by the stage's last conv)
  int slots[MLT_MAX_HEADS_K];
  const float *w[MLT_MAX_HEADS_K];    // [classes][C+2] fp32
  const float *b[MLT_MAX_HEADS_K];
  int c[MLT_MAX_HEADS_K], hw[MLT_MAX_HEADS_K], classes[MLT_MAX_HEADS_K];
  int n_heads, decision_head;
  const int32_t *poc, *qp;
  float *logits;   // [n][sum classes] or NULL
  int32_t *split;  // [n] (NULL: not wanted -- the record carries it)
  // Decision records and the confidence gate (NULL / 0: not wanted, and then no softmax is computed).  dec[n] <- the record of CU n (every head's
  // first-max argmax and its fp32 softmax probability; the decision head's margin).  min_conf > 0: split[n] (and dec[n].split_mode) = -1 unless the
  // decision head's confidence >= min_conf (a NaN confidence gates).
  DecisionRec *dec;
  float min_conf;
  // Candidate sets (heads_cand_kernel: mlt_launch_heads picks it when cand != NULL or the policy is not the default (0, 0); every other launch runs heads_kernel).
  // cand[n] <- the candidate record of CU n under (cand_cov, cand_max).
  CandRec *cand;
  float cand_cov;
  int cand_max;
  // Round 6, the MAGNITUDE guard's statistic: mag[n] <- max over all logits of sum_k |w_ck feat_k| -- the size of the feature-driven part of the logits, which is
  // what the fp16 pipeline's RELATIVE error acts on (poc, qp and the bias enter exactly).  NULL: not wanted.
  float *mag;
  // The guards' selection as the tail of this kernel (g_count != NULL; `rule` is all zeros otherwise): CU n is flagged when guard_rule says so under `rule`, on its
  // flat-content statistic g_flat[n] (NULL: no flat guard), which is CLEARED afterwards (consume-and-clear: the next pass's first kernel adds into it, no memset).
  // Single-CU launches (n == 1, g_next == NULL: mlt_predict's captured graph): g_count[0] = 1 and g_idx[0] = 0 when CU 0 is flagged, else g_count[0] = 0.
  // Batches (g_next != NULL; guard_select_kernel -- a launch of its own, 23 us + a launch gap of a 4 ms step -- stays behind MLT_TUNING=1 MLT_GUARD_SELECT_KERNEL=1):
  // g_count[0] is a running count, ZERO on entry: a workgroup whose CU is flagged appends it to g_idx (the list is UNORDERED -- the exact re-run treats every CU
  // independently, so the results do not depend on the order); workgroup 0 zeroes g_next[0], the counter the slot's next launch will count on (the runtime
  // alternates between two counters: the one zeroed here was read by the previous launch's count copy, which precedes this kernel in stream order).  No atomics,
  // no fences on the unflagged path.
  int32_t *g_count, *g_idx, *g_flat, *g_next;
  GuardRule rule;
};

// QP sweep (sweep_heads_kernel, mlt_tail_kernels.inc): the heads of one pass under n_qps values of qp.  `h` is read as by heads_kernel except h.qp (NULL: point
// q takes qps[q] for every CU; else a per-CU OFFSET: CU n takes qps[q] + h.qp[n], added as integers -- fix-up launches read it per CU of the re-run, like
// h.poc) and h.mag (unused); the outputs of point q start `slab` CUs behind those of point q - 1 (h.logits: slab x sum-classes floats).
// Fast pass (fix_idx == NULL): workgroup i is CU i and row i, every point is written; with the selection (h.g_next != NULL) mask[i] <- bit q set when CU i is
// flagged under qps[q] (guard_rule), and a CU with a non-zero mask is appended to h.g_idx.  Fix-up (fix_idx != NULL, no selection): workgroup j is CU j of
// the exact re-run, its row is fix_idx[j], and only the points whose bit is set in mask[fix_idx[j]] are written.
#define MLT_SWEEP_MAX_QPS_K 32
struct HeadSweepArgs {
  HeadArgs h;
  int32_t qps[MLT_SWEEP_MAX_QPS_K];
  int n_qps;
  long slab;
  const int32_t *fix_idx;
  uint32_t *mask;   // [rows]
  const uint32_t *active;   // fast pass with the selection: mask[i] is ANDed with active[i] -- the points CU i takes part in (tree sweeps); NULL: all points
};

// ---- parity guard (fast arithmetic): device-side selection of the CUs that are re-evaluated with the exact arithmetic ----
struct FlatStatArgs {
  const int16_t *org, *pred;   // Pel planes
  long org_row_stride, org_cu_stride, pred_row_stride, pred_cu_stride;  // in elements
  int32_t *flat;               // [n] number of near-constant 4-pixel quads (MLT_FLAT_RANGE)
  int n, s_l;                  // CU size S = 1 << s_l
};
struct GuardSelectArgs {
  const int32_t *flat;         // [n] (FlatStatArgs.flat) or NULL: no flat guard
  const float *logits;         // [n][n_logits] or NULL (the decision guard and what rides on it are off)
  int32_t *idx;                // [n] out: indices of the selected CUs, ascending
  int32_t *count;              // [1] out
  int n, n_logits, head_off, head_classes;
  const float *mag;            // [n] (HeadArgs.mag) or NULL: no magnitude guard
  GuardRule rule;              // CU i is selected when guard_rule says so, on flat[i], mag[i] and -- recomputed from logits[i] -- the decision head's confidence and candidate flag
  float min_conf;              // the gate and the candidate policy the heads kernel ran under (HeadArgs)
  float cand_cov;
  int cand_max;
};
struct GuardGatherArgs {
  const int16_t *org, *pred;
  long org_row_stride, org_cu_stride, pred_row_stride, pred_cu_stride;
  const int32_t *poc, *qp, *idx;
  int16_t *g_org, *g_pred;     // dense [k][S][S]
  int32_t *g_poc, *g_qp;       // [k]
  int k, s_l;
};
struct GuardScatterArgs {
  const int32_t *idx, *g_split;
  const float *g_logits;
  int32_t *split;              // [n] or NULL
  float *logits;               // [n][n_logits] or NULL
  int k, n_logits;
  const DecisionRec *g_dec;    // [k] records of the re-run, or NULL
  DecisionRec *dec;            // [n] or NULL
  const CandRec *g_cand;       // [k] candidate records of the re-run, or NULL
  CandRec *cand;               // [n] or NULL
};
// ---- device-resident pictures (mlt_predict_at): CUs named by position, gathered out of two pitched planes into dense staging (mlt_picture_kernels.inc) ----
struct PictureGatherArgs {
  const int16_t *org, *pred;   // sample (0, 0) of the two pictures; they are independent sources (base, pitch, alignment class each)
  long org_pitch, pred_pitch;  // in elements
  const int32_t *xy;           // [c][2]: x, y of every CU's top-left sample, validated by the host against the pictures' width and height
  int16_t *g_org, *g_pred;     // dense [c][S][S], 16-byte aligned
  int c, s_l;                  // CU size S = 1 << s_l (16 .. 128)
  int vec_org, vec_pred;       // the plane's extent starts and ends on 16-byte boundaries: aligned 16-byte loads may be used (else 2-byte loads only)
};
hipError_t mlt_launch_picture_gather(const PictureGatherArgs &a, hipStream_t st);
// ---- prediction pictures (mlt_picture_predict, mlt_picture_compensate): block motion search and quarter-sample compensation (mlt_motion_kernels.inc).  Blocks of
// B = 1 << block_l samples, clipped at the right and bottom border; the field is [by][bx][2] int16 {mvx, mvy} in quarter samples, raster order ----
#define MLT_MOTION_MAX_REFS_K 4   // include/mltcnn.h: MLT_MOTION_MAX_REFS (mlt_runtime.h asserts it)
struct MotionSearchArgs {
  const int16_t *cur, *ref;    // sample (0, 0) of the two pictures (independent bases and pitches; 2-byte loads only)
  long cur_pitch, ref_pitch;   // in elements
  int width, height;           // of both
  int block_l, range, lambda;  // candidates dx, dy in [-range, range], cost = SAD + lambda (|dx| + |dy|)
  int bx;                      // blocks per row (the grid is bx x by workgroups)
  int16_t *mv;                 // [by][bx][2] out, 4-byte aligned
  uint32_t *cost;              // [by][bx] out
};
struct PictureCompensateArgs {
  const int16_t *ref;          // sample (0, 0)
  long ref_pitch;
  int16_t *dst;                // sample (0, 0) of the prediction picture; width x height as ref
  long dst_pitch;
  int vec_dst;                 // dst's base and pitch are multiples of 16 bytes: whole 8-sample items are 16-byte stores
  int width, height;
  int block_l, bx, by;
  int tiles_y;                 // tiles of 16 rows per block (set by the launcher)
  const int16_t *mv;           // [by][bx][2]
  const uint8_t *ref_idx;      // NULL: every block reads `ref`; else [by][bx], block b reads refs[ref_idx[b]] (every entry < the number of references set)
  const int16_t *refs[MLT_MOTION_MAX_REFS_K];   // sample (0, 0) of the references of the table form, width x height each
  long ref_pitches[MLT_MOTION_MAX_REFS_K];
};
// mlt_picture_predict_refs: quarter-sample refinement of every reference's integer winner and the per-block choice among the references
struct MotionRefineArgs {
  const int16_t *cur;          // sample (0, 0) (2-byte loads only, as the references)
  long cur_pitch;
  const int16_t *refs[MLT_MOTION_MAX_REFS_K];
  long ref_pitches[MLT_MOTION_MAX_REFS_K];
  int n_refs;                  // 1 .. 4
  int width, height;
  int block_l, subpel, lambda; // subpel 0 / 1 / 2: candidates q in {0}, {-2, 0, 2}, {-3 .. 3} a side around 4 x the integer winner
  int bx;                      // blocks per row (the grid is bx x by workgroups)
  const int16_t *mv_int;       // the integer winners {4 dx, 4 dy}: slice r = mv_int + r * mv_int_slice, [by][bx][2]
  size_t mv_int_slice;         // in elements
  int16_t *mv;                 // [by][bx][2] out, 4-byte aligned
  uint32_t *cost;              // [by][bx] out: cost_q
  uint8_t *ref_out;            // [by][bx] out
};
int mlt_motion_search_lds(int block, int range);   // dynamic LDS bytes of motion_search_kernel: ((block + 2 range)^2 + block^2) x 2 + 32
int mlt_motion_refine_lds(int block);              // ... of motion_refine_kernel: (block + 8) block x 4 + 128 + ((block + 8)^2 + block^2) x 2
hipError_t mlt_launch_motion_search(const MotionSearchArgs &a, int by, hipStream_t st);
hipError_t mlt_launch_motion_refine(const MotionRefineArgs &a, int by, hipStream_t st);
hipError_t mlt_launch_picture_compensate(PictureCompensateArgs a, hipStream_t st);
// ---- partition trees (mlt_predict_tree, mlt_predict_trees): the quadtree descent between two network levels (mlt_tree_kernels.inc).  The arena is LEVEL-MAJOR
// over the pictures of the call (mlt_predict_tree: one) -- level l is one node range, picture 0's segment, then picture 1's, ...; a segment in the contract's order
// (roots, then children in their parents' order) ----
#define MLT_TREES_LEVELS 4
#define MLT_TREES_ROW 15      // floats of a node's logits row, in the arena and in the packed output (include/mltcnn.h: MLT_MAX_LOGITS; mlt_runtime.h asserts it)
// A node of the tree (include/mltcnn.h: mlt_tree_node -- same 32 bytes; mlt_runtime.h asserts the layout).
struct TreeNodeRec {
  int32_t x, y;
  int16_t size;
  int8_t depth;
  uint8_t flags;
  int32_t parent, first_child, split_mode;
  float confidence;
  uint32_t cand_mask;
};
// One entry of mlt_predict_trees (mlt_tree_picture as the device sees it): the gather's per-launch arguments of the one-picture path, per entry.
struct TreesEntry {
  const int16_t *org, *pred;   // sample (0, 0)
  long org_pitch, pred_pitch;  // elements
  int32_t vec_org, vec_pred;   // PictureGatherArgs.vec_org / vec_pred of THIS entry's planes
  int32_t poc, qp;
};
// The segment table, [MLT_TREES_LEVELS][n_pictures] each: where picture p's nodes of level l start in the arena, how many they are, and where they start in the
// packed (picture-major) output.  Written by the expand launches (a level's rows by the launch that writes the level's nodes; pack_base by the last one).
struct TreesSegs { int32_t *start, *n, *pack_base; };
// What an expand launch of either descent (the plain one below, the union descent of the tree sweeps further down) knows of the arena, of the level just evaluated
// and of the next one: the part the shared device helpers work on.
struct TreeLevelArgs {
  TreeNodeRec *nodes;          // every node of the call, level-major; node_cap entries
  int32_t *xy;                 // [node_cap][2]: the nodes' positions -- a level's slice is the position list its network pass gathers from
  int32_t *pic;                // [node_cap] picture index of every node, beside xy
  int node_cap;
  int32_t *seg_start, *seg_n;  // the segment table: a launch reads the level's rows and writes the next level's
  int n_pictures;
  int lvl_start, lvl_n;        // the level just evaluated, as one list over all pictures: nodes [lvl_start, lvl_start + lvl_n)
  int size;                    // its CU size; the next level's is size / 2
  int lvl;                     // its depth; lvl = -1 with lvl_n = 0 and size = 2 x top_size opens the trees
  const int32_t *next_roots;   // [n_next_roots][2] the roots EVERY picture's next segment opens with, raster order
  int n_next_roots, root_flags;   // root_flags: their mlt_tree_node.flags (bit 0 below top_size)
  int32_t *count;              // [1] out: the whole next level's node count = n_pictures x n_next_roots + 4 x descending nodes (NULL: not wanted)
};
struct TreeExpandArgs : TreeLevelArgs {
  int n_levels;                // lvl == n_levels - 1: the last launch also writes pack_base and first_node
  const DecisionRec *dec;      // [lvl_n] the level's decision records
  const CandRec *cand;         // [lvl_n] its candidate records, or NULL: cand_mask = 1 << raw_mode, every class when a logit of the decision head is NaN
  const float *logits;         // [lvl_n][n_logits] (read only when cand == NULL)
  int n_logits, head_off, head_classes;   // the decision head inside a row of logits
  uint32_t descend_mask;       // classes of the decision head that mean "quad split"; 0: the level never descends (min_size)
  int by_candidates;           // descend on cand_mask & descend_mask instead of on split_mode
  int32_t *pack_base;          // the segment table's third part, out (last launch)
  int32_t *first_node;         // [n_pictures + 1] out (last launch)
};
struct TreeRasterArgs {
  const TreeNodeRec *nodes;
  const int32_t *pic;
  int lvl_start, lvl_n;
  int blk_l;                   // log2(size / 16): a node covers (1 << blk_l)^2 map bytes
  uint8_t *map;                // [n_pictures][map_h][map_w], one byte per 16 x 16 block: picture p's map starts at map + p * map_bytes
  size_t map_bytes;
  int map_w, map_h;
};
struct PictureGatherMultiArgs {
  const TreesEntry *entries;   // [n_entries]
  const int32_t *pic;          // [c] entry of every CU
  const int32_t *xy;           // [c][2], inside every entry's (common) width x height
  int16_t *g_org, *g_pred;     // dense [c][S][S], 16-byte aligned
  int32_t *g_poc, *g_qp;       // [c] out: the CU's entry's poc / qp
  int c, s_l, n_entries;
};
struct TreesPackArgs {
  const TreeNodeRec *nodes; const int32_t *pic; const float *logits; const DecisionRec *dec; const CandRec *cand;   // level-major (logits / dec / cand: NULL = not wanted)
  TreeNodeRec *o_nodes; float *o_logits; DecisionRec *o_dec; CandRec *o_cand;                                       // picture-major; o_logits: MLT_TREES_ROW floats per node
  TreesSegs segs;
  const int32_t *first_node;
  int n_pictures, n_levels, total;
  int lvl_start[MLT_TREES_LEVELS], n_logits[MLT_TREES_LEVELS];   // a level's logits are dense [lvl_n][n_logits] from row lvl_start of the MLT_TREES_ROW-float rows
};
// ---- tree sweeps (mlt_predict_tree_sweep, mlt_predict_trees_sweep): the UNION descent of n_pictures entries (one: mlt_predict_tree_sweep) under n_qps points each
// (mlt_tree_kernels.inc; the arena: mlt_layout.h TreeSweepArena).  A level is one node range over all entries -- entry 0's union segment, entry 1's, ... (the
// segment table: [MLT_TREES_LEVELS][n_pictures] start and count).  A union node carries pic (its entry), alive (bit q: part of the entry's tree q) and desc (bit q:
// descends under point q); its per-point records / logits / candidate records are slab-major: element (q, i) of a level lies q * slab + i behind the level's
// element (0, 0).
struct TreeSweepExpandArgs : TreeLevelArgs {   // nodes: the union's (parent / first_child: union indices; split_mode / confidence / cand_mask stay unset); pic: a node's entry
  uint32_t *alive, *desc;      // [node_cap]
  int next_start, next_cap;    // where the next level starts and how many nodes it may hold
  const DecisionRec *dec;      // the level's element (0, 0) of each slab array
  const CandRec *cand;         // NULL: the default policy's mask from the logits (TreeExpandArgs.cand)
  const float *logits;
  long slab;
  int n_qps, n_logits, head_off, head_classes;
  uint32_t descend_mask;
  int by_candidates;           // (next_roots: alive under every point; count: 4 x the nodes descending under ANY point)
};
struct TreeSweepRasterArgs {
  const TreeNodeRec *nodes;
  const uint32_t *alive, *desc;
  const int32_t *pic;
  const DecisionRec *dec;      // the level's element (0, 0)
  long slab;
  int lvl_start, lvl_n, blk_l, n_qps, n_pictures;
  uint8_t *map;                // [n_pictures][n_qps][map_h][map_w]
  size_t map_bytes;
  int map_w, map_h;
};
// after the last level: idx[q][g] <- the index of union node g inside slice (pic[g], q) (-1: not part of it), total[p * n_qps + q] <- the slice's node count |
// the slices themselves, first_node [n_pictures * n_qps + 1], union_nodes [n_pictures][MLT_TREES_LEVELS]
struct TreeSweepPackArgs {
  const TreeNodeRec *nodes; const uint32_t *alive, *desc; const DecisionRec *dec; const float *logits; const CandRec *cand;   // whole arena arrays
  const int32_t *pic, *seg_start, *seg_n;
  int n_pictures;
  int32_t *idx, *total, *first_node, *union_nodes;
  TreeNodeRec *o_nodes; float *o_logits; DecisionRec *o_dec; CandRec *o_cand;   // [out_cap]; NULL = not wanted
  int n_qps, n_levels, node_cap, out_cap;
  int lvl_start[MLT_TREES_LEVELS], lvl_n[MLT_TREES_LEVELS], lvl_cap[MLT_TREES_LEVELS];   // level l: union nodes [lvl_start, lvl_start + lvl_n), slab stride lvl_cap
  int n_logits[MLT_TREES_LEVELS], head_off[MLT_TREES_LEVELS], head_classes[MLT_TREES_LEVELS], has_cand[MLT_TREES_LEVELS];
};
hipError_t mlt_launch_tree_expand_sweep(const TreeSweepExpandArgs &a, hipStream_t st);
hipError_t mlt_launch_tree_sweep_raster(const TreeSweepRasterArgs &a, hipStream_t st);
hipError_t mlt_launch_tree_sweep_rank(const TreeSweepPackArgs &a, hipStream_t st);
hipError_t mlt_launch_tree_sweep_pack(const TreeSweepPackArgs &a, hipStream_t st);
hipError_t mlt_launch_tree_expand(const TreeExpandArgs &a, hipStream_t st);
hipError_t mlt_launch_tree_raster(const TreeRasterArgs &a, hipStream_t st);
hipError_t mlt_launch_picture_gather_multi(const PictureGatherMultiArgs &a, hipStream_t st);
hipError_t mlt_launch_trees_pack(const TreesPackArgs &a, hipStream_t st);
hipError_t mlt_launch_flat_stat(const FlatStatArgs &a, bool aligned8, hipStream_t st);
hipError_t mlt_launch_guard_select(const GuardSelectArgs &a, hipStream_t st);
hipError_t mlt_launch_guard_gather(const GuardGatherArgs &a, hipStream_t st);
hipError_t mlt_launch_guard_scatter(const GuardScatterArgs &a, hipStream_t st);

enum { MLT_CONV_DEFAULT = 0, MLT_CONV_DMA = 1, MLT_CONV_LATENCY = 2, MLT_CONV_CENTRE = 3 };  // kernel variant of a layer shape
bool mlt_conv_has_centre_variant(int cin, int cout);  // 1x1 (centre-tap) instantiation for stride-1 layers on 1x1 maps
hipError_t mlt_launch_conv(int cin, int cout, int stride, int nsplit, int variant, const ConvArgs &a, int grid_x, hipStream_t st);  // nsplit: 1 fast, 2 exact, 4 weights hi+lo on the FAST tiling (MLT_MODEL_W2), 6 exact-lite; any other, or a key without a row, is refused
bool mlt_conv_cfg(int cin, int cout, int stride, int exact, ConvCfg *out);
int mlt_conv_ring_bytes(int cin, int cout, int stride, int nsplit, int variant);  // LDS bytes of the weight ring of the kernel mlt_launch_conv selects for the key (-1: none)
hipError_t mlt_launch_stem5(const Stem5Args &a, int nsplit, int grid_x, int lds, hipStream_t st);  // nsplit as mlt_launch_conv
hipError_t mlt_launch_block32(const Block32Args &a, bool w2, int grid_x, hipStream_t st);     // w2: hi+lo weights (8 x 32 tiles)
hipError_t mlt_launch_stem_block(const StemBlockArgs &a, bool w2, int grid_x, hipStream_t st);
// xs: the pair layer0_stream_xs_kernel -> layer1_stream_xs_kernel (the shortcut's input is handed over and layer1 computes the shortcut); both or neither
hipError_t mlt_launch_layer0_stream(const Layer0Args &a, bool fuse5, bool mfma32, bool xs, int grid_x, hipStream_t st);
hipError_t mlt_launch_layer1_stream(const Layer1Args &a, bool mfma32, bool xs, int grid_x, hipStream_t st);
hipError_t mlt_launch_heads(const HeadArgs &a, int n, hipStream_t st);
hipError_t mlt_launch_heads_sweep(const HeadSweepArgs &a, int n, hipStream_t st);
