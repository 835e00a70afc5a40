// mlt_split_predictor.hpp -- C++ host-side mirror of the reference call site, above the C ABI (include/mltcnn.h).
//
// The reference has no operator/plugin interface for this path: the CNN is an inline block of
// EncCu::xCompressCU (vtm-mlt-cpp/source/Lib/EncoderLib/EncCu.cpp:799-930).  This class gives that block a name
// and keeps its argument meaning and error behaviour:
//   gate()              == the useCNN condition                       EncCu.cpp:746-756
//   predictSplitMode()  == gather + absdiff + normalise + forward + argmax   EncCu.cpp:806-921
//   failure             -> returns -1, exactly what the reference leaves in predictedSplitMode when
//                          torch throws (EncCu.cpp:902-905,923-926); EncModeCtrl::setNewModeList(…,-1,…) is then a
//                          no-op (EncModeCtrl.cpp:147-148) and the encoder runs its exhaustive RDO.
// Header-only; link with -lmltcnn_hip.  One instance per EncCu (the encoder is single-threaded, or one EncCu per
// thread under WPP / split parallelism, EncCu.cpp:233).
//
// Decisions: the split mode is what the encoder consumes (EncCu.cpp:921 -> EncModeCtrl.cpp:110-149), so the library's DECISION GUARD is
// on by default (ABI 4; margin 3 x tolerance; MLT_FLAG_NO_DECISION_GUARD turns it off): a CU whose decision-head top-2 margin is too
// small for the fast arithmetic's calibrated error to leave the argmax alone is re-evaluated with the exact arithmetic before the call returns.
//
// MLTCNN_STATS=1 (any build): the destructor prints ONE line to stderr -- calls and wall-clock seconds inside predictSplitMode / submit /
// flush / wait, calls per CU size, seconds inside mlt_init (weights + calibration) -- the "share of an encode spent inside the predictor" figure
// tools/eval_harness.py reads (N4).
//
// MLTCNN_MIN_CONF (any build, read next to MLTCNN_STATS): the library's CONFIDENCE GATE (mlt_set_confidence_gate) -- either one number for every enabled
// size ("0.9") or per size ("128:0.9,64:0.8").  A CU whose decision-head softmax probability stays below the threshold comes back as -1 from
// predictSplitMode() / waitSplitMode(): "no prediction", EncModeCtrl::setNewModeList is a no-op and the encoder runs its exhaustive RDO for that CU.
// A gated call is NOT a failure: no "error" line, not counted in failed=; under MLTCNN_STATS=1 the stats line ends with gated=<count> when a gate
// is set.  Malformed value: a message on stderr, the gate stays off.  predictDecision() / waitDecision() return the whole decision record.
//
// MLTCNN_CANDIDATES (any build, read next to MLTCNN_MIN_CONF): the library's CANDIDATE POLICY (mlt_set_candidate_policy) -- "coverage[/max]" for every enabled
// size ("0.9", "0.9/2") or per size ("128:0.9/2,64:0.8").  predictCandidates() / waitCandidates() then return, per CU, the smallest set of classes of the
// decision head that carries `coverage` of the softmax probability -- every class when that takes more than `max` of them (full RDO) -- as a bit mask over
// CLASS INDICES; keptClasses() lists them in rank order.  Malformed value: a message on stderr, every policy stays at its default (the argmax alone).  Under
// MLTCNN_STATS=1 the stats line ends with kept_modes=<sum of the counts returned> when a policy is set.
//
// Test hooks, compiled in only with -DMLTCNN_TEST_HOOKS (tools/build_vtm.sh does; a production build carries none of them):
//   MLTCNN_FAULT_INJECT=1      the predictor reports ok() without touching a device and every predictSplitMode() fails (-1):
//                              exercises the reference's swallow-and-continue contract from the real call site on a box without a GPU
//   MLTCNN_FORCE_SPLIT=k       (with MLTCNN_FAULT_INJECT=1) every prediction "succeeds" with split mode k instead of failing: real, decision-
//                              dependent encoder paths (EncModeCtrl::setNewModeList, EncModeCtrl.cpp:110-149) on a box without a GPU -- how
//                              the probe-and-replay schedule is debugged against the serial encoder in the build container
//   MLTCNN_CALL_DUMP_FILE=path every predictSplitMode() call is appended to `path` (little-endian records, see dumpCall; one
//                              write(2) per record on an O_APPEND descriptor, so instances on several threads cannot interleave):
//                              tests/test_vtm_encoder.py re-checks each one against the CPU oracle
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#ifdef MLTCNN_TEST_HOOKS
#include <fcntl.h>
#include <unistd.h>
#endif

#include "../include/mltcnn.h"

namespace mlt {

using Pel = int16_t;  // CommonLib/TypeDef.h:277 (RExt__HIGH_BIT_DEPTH_SUPPORT off)

class SplitPredictor {
 public:
  // weightsDir replaces the hard-coded "/home/ubuntu/whyeo/vtm-mlt-final/torch_model" (EncCu.cpp:899); files are
  // MLTORPQ_splitMode_<S>.mltw (tools/convert_weights.py).  sizeMask: MLT_SIZE_* bits (reference: 128 only, :754).
  // flags: MLT_FLAG_* bits; 0 = the library's defaults (decision guard and flat guard on, see above).  devices / nDevices: one predictor serving several GPUs
  // (mlt_config.devices: batches submitted through submitSplitMode() are dealt round-robin); nullptr: `device`.
  explicit SplitPredictor(const std::string &weightsDir, int device = 0, uint32_t sizeMask = MLT_SIZE_128, uint32_t flags = 0,
                          const int *devices = nullptr, int nDevices = 0) {
    mlt_config cfg{};
    cfg.struct_size = sizeof cfg;
    cfg.device = device;
    for (int i = 0; i < nDevices && i < MLT_MAX_DEVICES && devices; ++i) { cfg.devices[i] = devices[i]; cfg.n_devices = i + 1; }
    cfg.weights_dir = weightsDir.c_str();
    cfg.size_mask = sizeMask;
    for (int &h : cfg.head_index) h = -1;  // reference defaults: element [2] for 128, [0] otherwise (EncCu.cpp:913-919)
    cfg.max_batch = 1;
    cfg.flags = flags;
    cfg.guard_margin = 0.f;  // the decision guard's default threshold (3 x tolerance)
    cfg.tolerance = 0.f;     // default |dlogit| contract (1e-3) for the load-time calibration of the fast arithmetic
    m_mask = sizeMask ? sizeMask : MLT_SIZE_128;
    if (const char *s = std::getenv("MLTCNN_STATS")) m_stats = std::atoi(s) != 0;
#ifdef MLTCNN_TEST_HOOKS
    if (const char *d = std::getenv("MLTCNN_CALL_DUMP_FILE")) m_dumpPath = d;
    if (const char *f = std::getenv("MLTCNN_FAULT_INJECT")) m_faultInject = std::atoi(f) != 0;
    if (const char *f = std::getenv("MLTCNN_FORCE_SPLIT")) m_forceSplit = std::atoi(f);
    if (m_faultInject) return;
#endif
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = mlt_init(&cfg, &m_ctx);   // loads, folds, packs and CALIBRATES the weights of every enabled size (once per encoder process)
    m_initSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc != MLT_OK) {
      std::fprintf(stderr, "error loading the model\n");  // the reference's message (EncCu.cpp:904)
      std::fprintf(stderr, "  mltcnn: %s\n", mlt_last_error(nullptr));
      m_ctx = nullptr;
    }
    if (m_ctx)
      if (const char *g = std::getenv("MLTCNN_MIN_CONF")) applyMinConf(g);
    if (m_ctx)
      if (const char *g = std::getenv("MLTCNN_CANDIDATES")) applyCandidates(g);
  }
  ~SplitPredictor() {
    if (m_stats) {   // (one fprintf for the whole line: predictors of several EncCu threads share stderr)
      char line[768];
      int k = std::snprintf(line, sizeof line, "mltcnn-stats predict_calls=%llu predict_s=%.6f submit_calls=%llu submit_s=%.6f wait_calls=%llu wait_s=%.6f flush_calls=%llu flush_s=%.6f "
                            "calls_128=%llu calls_64=%llu calls_32=%llu calls_16=%llu failed=%llu init_s=%.6f",
                            m_n[0], m_t[0], m_n[1], m_t[1], m_n[2], m_t[2], m_n[3], m_t[3], m_bySize[0], m_bySize[1], m_bySize[2], m_bySize[3], m_failed, m_initSeconds);
      if (m_gateSet && k > 0 && k < (int)sizeof line) k += std::snprintf(line + k, sizeof line - (size_t)k, " gated=%llu", m_gated);
      if (m_policySet && k > 0 && k < (int)sizeof line) std::snprintf(line + k, sizeof line - (size_t)k, " kept_modes=%llu", m_keptModes);
      std::fprintf(stderr, "%s\n", line);
    }
    mlt_shutdown(m_ctx);
  }
  SplitPredictor(const SplitPredictor &) = delete;
  SplitPredictor &operator=(const SplitPredictor &) = delete;

  bool ok() const { return m_ctx != nullptr || m_faultInject; }

  // EncCu.cpp:746-756.  chType: partitioner.chType (0 = luma / joint tree); isIntraSlice: slice type == I_SLICE;
  // (cux, cuy, cuw, cuh): tempCS->area.Y(); (picW, picH): slice->getPic()->Y().
  bool gate(int chType, bool isIntraSlice, int cux, int cuy, int cuw, int cuh, int picW, int picH) const {
    if (chType != 0 || isIntraSlice || cuw != cuh) return false;
    const uint32_t bit = cuw == 128 ? MLT_SIZE_128 : cuw == 64 ? MLT_SIZE_64 : cuw == 32 ? MLT_SIZE_32 : cuw == 16 ? MLT_SIZE_16 : 0u;
    if (!(bit & m_mask)) return false;
    return cux + cuw <= picW && cuy + cuh <= picH;
  }

  // EncCu.cpp:806-921.  org: bestCS->getOrgBuf().Y() {buf, stride}; pred: bestCS->getPredBuf().Y() {buf, stride};
  // poc: bestCS->slice->getPOC(); cuQP: currTestMode.qp.  Returns predictedSplitMode (0 none, 1 QT, 2 BT_H, 3 BT_V, ...)
  // or -1 on any failure.
  int predictSplitMode(const Pel *org, int orgStride, const Pel *pred, int predStride, int cuw, int poc, int cuQP, float *logitsOpt = nullptr) {
    int32_t split = -1;
    float lg[MLT_MAX_LOGITS] = {0};
    Timer tm(this, 0, cuw);
    if (m_faultInject && m_forceSplit >= 0) return m_forceSplit;
    if (!m_ctx || mlt_predict(m_ctx, org, orgStride, pred, predStride, cuw, poc, cuQP, &split, (logitsOpt || !m_dumpPath.empty()) ? lg : nullptr) != MLT_OK) {
      std::fprintf(stderr, "error\n");  // EncCu.cpp:925
      split = -1;
      ++m_failed;
    } else if (split < 0) ++m_gated;   // withheld by the confidence gate: not a failure
    if (logitsOpt) for (int i = 0; i < mlt_num_logits(cuw); ++i) logitsOpt[i] = lg[i];
    if (!m_dumpPath.empty()) dumpCall(org, orgStride, pred, predStride, cuw, poc, cuQP, split, lg);
    return split;
  }

  // Encoder-side batching: stage the CU now, decide later.  submitSplitMode() returns a ticket (or
  // false on failure: treat like predictedSplitMode = -1); waitSplitMode() returns the split mode of that ticket and runs
  // every CU staged so far for this size as ONE batch if that has not happened yet.  With k CUs whose setNewModeList
  // call can be postponed together (e.g. the CTUs of a WPP anti-diagonal) the per-CU cost falls from ~150 us to
  // ~150 us / k (+ ~8 us).  At most MLT_DEFER_CAP CUs per batch; a full batch is launched by the next submit.
  bool submitSplitMode(const Pel *org, int orgStride, const Pel *pred, int predStride, int cuw, int poc, int cuQP, mlt_ticket *ticket) {
    Timer tm(this, 1, cuw);
    if (m_faultInject && m_forceSplit >= 0) { *ticket = 0; return true; }
    return m_ctx && mlt_submit(m_ctx, org, orgStride, pred, predStride, cuw, poc, cuQP, ticket) == MLT_OK;
  }
  void flush(int cuw) { Timer tm(this, 3, 0); if (m_ctx) (void)mlt_flush(m_ctx, cuw); }  // start the batch early, e.g. before unrelated host work
  int waitSplitMode(int cuw, mlt_ticket ticket, float *logitsOpt = nullptr) {
    int32_t split = -1;
    Timer tm(this, 2, 0);
    if (m_faultInject && m_forceSplit >= 0) return m_forceSplit;
    if (!m_ctx || mlt_wait(m_ctx, cuw, ticket, &split, logitsOpt) != MLT_OK) return -1;
    if (split < 0) ++m_gated;
    return split;
  }

  // The whole decision record (include/mltcnn.h: mlt_decision -- every level's argmax and confidence, the gated and the raw split mode) for callers that want
  // more than the one integer.  false on failure (out->split_mode = -1: treat like predictedSplitMode = -1).
  bool predictDecision(const Pel *org, int orgStride, const Pel *pred, int predStride, int cuw, int poc, int cuQP, mlt_decision *out, float *logitsOpt = nullptr) {
    Timer tm(this, 0, cuw);
    *out = mlt_decision{};
    out->split_mode = out->raw_mode = -1;
    if (!m_ctx || mlt_predict_decision(m_ctx, org, orgStride, pred, predStride, cuw, poc, cuQP, out, logitsOpt) != MLT_OK) {
      std::fprintf(stderr, "error\n");  // EncCu.cpp:925
      out->split_mode = -1;
      ++m_failed;
      return false;
    }
    if (out->split_mode < 0) ++m_gated;
    return true;
  }
  bool waitDecision(int cuw, mlt_ticket ticket, mlt_decision *out, float *logitsOpt = nullptr) {
    Timer tm(this, 2, 0);
    *out = mlt_decision{};
    out->split_mode = out->raw_mode = -1;
    if (!m_ctx || mlt_wait_decision(m_ctx, cuw, ticket, out, logitsOpt) != MLT_OK) { out->split_mode = -1; return false; }
    if (out->split_mode < 0) ++m_gated;
    return true;
  }

  // The candidate record (include/mltcnn.h: mlt_candidates -- which classes of the decision head stay in the RDO under the size's candidate policy), with the
  // decision record beside it when decOpt != nullptr.  false on failure: every class kept (full RDO) and decOpt->split_mode = raw_mode = -1.
  bool predictCandidates(const Pel *org, int orgStride, const Pel *pred, int predStride, int cuw, int poc, int cuQP, mlt_candidates *out, mlt_decision *decOpt = nullptr,
                         float *logitsOpt = nullptr) {
    Timer tm(this, 0, cuw);
    if (!m_ctx || mlt_predict_candidates(m_ctx, org, orgStride, pred, predStride, cuw, poc, cuQP, out, decOpt, logitsOpt) != MLT_OK) {
      std::fprintf(stderr, "error\n");  // EncCu.cpp:925
      failCandidates(cuw, out, decOpt);
      ++m_failed;
      return false;
    }
    m_keptModes += (unsigned long long)out->count;
    if (decOpt && decOpt->split_mode < 0) ++m_gated;
    return true;
  }
  bool waitCandidates(int cuw, mlt_ticket ticket, mlt_candidates *out, mlt_decision *decOpt = nullptr, float *logitsOpt = nullptr) {
    Timer tm(this, 2, 0);
    if (!m_ctx || mlt_wait_candidates(m_ctx, cuw, ticket, out, decOpt, logitsOpt) != MLT_OK) { failCandidates(cuw, out, decOpt); return false; }
    m_keptModes += (unsigned long long)out->count;
    if (decOpt && decOpt->split_mode < 0) ++m_gated;
    return true;
  }

  // Device-resident pictures (include/mltcnn.h: mlt_picture, mlt_predict_at) for callers that evaluate WHOLE frames -- a lookahead or pre-analysis pass, not the
  // per-CU call of xCompressCU, which gains nothing measurable from them.  uploadPicture() copies one luma plane (Pel rows of `stride` elements)
  // to the device; *pic == nullptr: the picture is created first (width x height), else it is reused for the next frame of the same geometry.  The pictures live
  // until the predictor is destroyed.  false on failure.
  bool uploadPicture(mlt_picture **pic, const Pel *plane, int stride, int width, int height) {
    if (!m_ctx || !pic) return false;
    if (!*pic && mlt_picture_create(m_ctx, width, height, pic) != MLT_OK) { *pic = nullptr; return false; }
    return mlt_picture_upload(m_ctx, *pic, plane, stride) == MLT_OK;
  }
  // Prediction pictures made on the device (include/mltcnn.h: mlt_picture_compensate, mlt_picture_predict) for callers that hold ORIGINALS only: dst, a picture made
  // by uploadPicture() / mlt_picture_create, receives the quarter-sample compensation of ref with the host field mv ([by][bx][2] {mvx, mvy}, quarter samples,
  // blocks of `block` samples) -- or, predictPicture(), with the field an integer-sample search of cur in ref finds (candidates in [-range, range]^2, cost = SAD +
  // lambda (|dx| + |dy|); mvOut [by][bx][2] / costOut [by][bx]: host arrays or nullptr, and with neither the call returns after enqueueing).  dst then serves as
  // `pred` of predictAt / predictTree and their sweeps, in stream order.  This is a pre-analysis prediction with its own rounding, not the encoder's interpolation.
  // false on failure, and dst is left alone.
  bool compensatePicture(const mlt_picture *ref, const int16_t *mv, mlt_picture *dst, int block = 16) {
    if (!m_ctx) return false;
    mlt_motion_config cfg{};
    cfg.struct_size = (uint32_t)sizeof cfg; cfg.block = block;
    return mlt_picture_compensate(m_ctx, ref, &cfg, mv, dst) == MLT_OK;
  }
  bool predictPicture(const mlt_picture *cur, const mlt_picture *ref, mlt_picture *dst, int block = 16, int range = 16, int lambda = 0, int16_t *mvOut = nullptr,
                      uint32_t *costOut = nullptr) {
    if (!m_ctx) return false;
    mlt_motion_config cfg{};
    cfg.struct_size = (uint32_t)sizeof cfg; cfg.block = block; cfg.range = range; cfg.lambda = lambda;
    return mlt_picture_predict(m_ctx, cur, ref, &cfg, dst, mvOut, costOut) == MLT_OK;
  }
  // ... with quarter-sample refinement and a per-block choice among nRefs (1 .. MLT_MOTION_MAX_REFS) references (include/mltcnn.h: mlt_picture_predict_refs,
  // mlt_picture_compensate_refs): every reference's integer winner is refined over the half (subpel 1) or quarter (subpel 2) sample window (0: none) and each block
  // takes the best (reference, vector) by cost_q = 4 SADP + lambda (|mvx| + |mvy|).  refOut / refIdx [by][bx]: the blocks' reference indices (refIdx nullptr:
  // refs[0] everywhere); costOut is cost_q.  false on failure, and dst is left alone.
  bool compensatePictureRefs(const mlt_picture *const *refs, int nRefs, const int16_t *mv, const uint8_t *refIdx, mlt_picture *dst, int block = 16) {
    if (!m_ctx) return false;
    mlt_motion_refs_config cfg{};
    cfg.struct_size = (uint32_t)sizeof cfg; cfg.block = block;
    return mlt_picture_compensate_refs(m_ctx, refs, nRefs, &cfg, mv, refIdx, dst) == MLT_OK;
  }
  bool predictPictureRefs(const mlt_picture *cur, const mlt_picture *const *refs, int nRefs, mlt_picture *dst, int block = 16, int range = 16, int lambda = 0,
                          int subpel = 2, int16_t *mvOut = nullptr, uint8_t *refOut = nullptr, uint32_t *costOut = nullptr) {
    if (!m_ctx) return false;
    mlt_motion_refs_config cfg{};
    cfg.struct_size = (uint32_t)sizeof cfg; cfg.block = block; cfg.range = range; cfg.lambda = lambda; cfg.subpel = subpel;
    return mlt_picture_predict_refs(m_ctx, cur, refs, nRefs, &cfg, dst, mvOut, refOut, costOut) == MLT_OK;
  }
  // n CUs of cuw x cuw at xy[i] = {x, y} of the picture pair, one batch: splitModes[i] as predictSplitMode() returns it, and -- candOpt / decOpt != nullptr -- the
  // candidate and decision records beside it.  false on failure: every split mode -1, every candidate record keeps all classes (full RDO), no prediction in the
  // decision records.
  bool predictAt(const mlt_picture *org, const mlt_picture *pred, int cuw, int n, const int32_t *xy, const int32_t *poc, const int32_t *cuQP, int32_t *splitModes,
                 mlt_candidates *candOpt = nullptr, mlt_decision *decOpt = nullptr, float *logitsOpt = nullptr) {
    Timer tm(this, 0, cuw);
    if (!m_ctx || !splitModes || mlt_predict_at(m_ctx, cuw, org, pred, n, xy, poc, cuQP, splitModes, logitsOpt, decOpt, candOpt) != MLT_OK) {
      std::fprintf(stderr, "error\n");  // EncCu.cpp:925
      for (int i = 0; i < n; ++i) {
        if (splitModes) splitModes[i] = -1;
        if (candOpt) failCandidates(cuw, candOpt + i, decOpt ? decOpt + i : nullptr);
        else if (decOpt) { decOpt[i] = mlt_decision{}; decOpt[i].split_mode = decOpt[i].raw_mode = -1; }
      }
      ++m_failed;
      return false;
    }
    for (int i = 0; i < n; ++i) {
      if (splitModes[i] < 0) ++m_gated;
      if (candOpt) m_keptModes += (unsigned long long)candOpt[i].count;
    }
    return true;
  }

  // predictAt() under nQps values of the CU QP from ONE network pass (include/mltcnn.h: mlt_predict_at_sweep; 1 <= nQps <= MLT_SWEEP_MAX_QPS): the outputs hold
  // nQps slabs of n entries, element (q, i) at q * n + i, slab q being what predictAt() gives with every cuQP[i] = qps[q].  false on failure: every split mode of
  // every slab -1, every candidate record keeps all classes (full RDO), no prediction in the decision records.
  bool predictAtSweep(const mlt_picture *org, const mlt_picture *pred, int cuw, int n, const int32_t *xy, const int32_t *poc, const int32_t *qps, int nQps,
                      int32_t *splitModes, mlt_candidates *candOpt = nullptr, mlt_decision *decOpt = nullptr, float *logitsOpt = nullptr) {
    Timer tm(this, 0, cuw);
    const long total = (nQps > 0 && nQps <= MLT_SWEEP_MAX_QPS && n > 0) ? (long)nQps * n : 0;
    if (!m_ctx || !splitModes || mlt_predict_at_sweep(m_ctx, cuw, org, pred, n, xy, poc, qps, nQps, splitModes, logitsOpt, decOpt, candOpt) != MLT_OK) {
      std::fprintf(stderr, "error\n");  // EncCu.cpp:925
      for (long i = 0; i < total; ++i) {
        if (splitModes) splitModes[i] = -1;
        if (candOpt) failCandidates(cuw, candOpt + i, decOpt ? decOpt + i : nullptr);
        else if (decOpt) { decOpt[i] = mlt_decision{}; decOpt[i].split_mode = decOpt[i].raw_mode = -1; }
      }
      ++m_failed;
      return false;
    }
    for (long i = 0; i < total; ++i) {
      if (splitModes[i] < 0) ++m_gated;
      if (candOpt) m_keptModes += (unsigned long long)candOpt[i].count;
    }
    return true;
  }

  // The partition tree of a picture pair (include/mltcnn.h: mlt_predict_tree): the quadtree descent from topSize down to minSize on the device, one (poc, qp) pair
  // for the picture.  nodes: level by level in the contract's order; leafMap: one byte per complete 16 x 16 block, [mapH][mapW], (log2(leaf size) - 4) |
  // ((split_mode + 1) << 4), 0xFF where no node covers the block.  On failure the tree is EMPTY (no nodes, no map): the caller visits every CU, as with -1.
  struct PartitionTree {
    std::vector<mlt_tree_node> nodes;
    std::vector<uint8_t> leafMap;
    int mapW = 0, mapH = 0;
    bool empty() const { return nodes.empty(); }
  };
  PartitionTree predictTree(const mlt_picture *org, const mlt_picture *pred, int width, int height, int poc, int qp, int topSize = 128, int minSize = 16,
                            bool byCandidates = false) {
    Timer tm(this, 0, 0);   // (a tree is one call, not a CU of one size)
    PartitionTree t;
    const int cap = mlt_tree_max_nodes(width, height, topSize, minSize);
    mlt_tree_config cfg{};
    cfg.struct_size = (uint32_t)sizeof cfg;
    cfg.top_size = topSize; cfg.min_size = minSize; cfg.poc = poc; cfg.qp = qp;
    cfg.flags = byCandidates ? MLT_TREE_BY_CANDIDATES : 0u;
    int n = 0;
    if (cap > 0) {
      t.nodes.resize((size_t)cap);
      t.mapW = width / 16; t.mapH = height / 16;
      t.leafMap.assign((size_t)t.mapW * (size_t)t.mapH, (uint8_t)0xFF);
    }
    if (!m_ctx || cap <= 0 || mlt_predict_tree(m_ctx, org, pred, &cfg, t.nodes.data(), cap, &n, t.leafMap.data(), nullptr, 0, nullptr, nullptr) != MLT_OK) {
      std::fprintf(stderr, "error\n");  // EncCu.cpp:925
      ++m_failed;
      return PartitionTree();
    }
    t.nodes.resize((size_t)n);
    for (const mlt_tree_node &nd : t.nodes)
      if (nd.split_mode < 0) ++m_gated;
    return t;
  }

  // The partition trees of ONE picture pair under several QPs from one call (include/mltcnn.h: mlt_predict_tree_sweep): one descent over the union of the trees,
  // the conv trunk once per union node, the heads once per QP.  Tree q is what predictTree returns with qp = qps[q].  unionNodesOpt: [4], the nodes the network
  // evaluated per level from topSize down.  On failure every tree is EMPTY (the vector still has one entry per QP).
  std::vector<PartitionTree> predictTreeSweep(const mlt_picture *org, const mlt_picture *pred, int width, int height, int poc, const std::vector<int32_t> &qps,
                                              int topSize = 128, int minSize = 16, bool byCandidates = false, int32_t *unionNodesOpt = nullptr) {
    Timer tm(this, 0, 0);
    const int Q = (int)qps.size(), per = mlt_tree_max_nodes(width, height, topSize, minSize);
    const long long cap = (long long)Q * per;
    std::vector<PartitionTree> trees((size_t)Q);
    mlt_tree_config cfg{};
    cfg.struct_size = (uint32_t)sizeof cfg;
    cfg.top_size = topSize; cfg.min_size = minSize; cfg.poc = poc;
    cfg.flags = byCandidates ? MLT_TREE_BY_CANDIDATES : 0u;
    const int mapW = width / 16, mapH = height / 16;
    const size_t mapBytes = (size_t)mapW * (size_t)mapH;
    std::vector<mlt_tree_node> nodes;
    std::vector<uint8_t> maps;
    std::vector<int32_t> first((size_t)Q + 1, 0);
    const bool sized = Q >= 1 && Q <= MLT_SWEEP_MAX_QPS && per > 0 && cap <= 0x7fffffff;
    if (sized) { nodes.resize((size_t)cap); maps.assign((size_t)Q * mapBytes, (uint8_t)0xFF); }
    if (!m_ctx || !sized || mlt_predict_tree_sweep(m_ctx, org, pred, &cfg, qps.data(), Q, nodes.data(), (int)cap, first.data(), unionNodesOpt, maps.data(), nullptr, 0,
                                                   nullptr, nullptr) != MLT_OK) {
      std::fprintf(stderr, "error\n");  // EncCu.cpp:925
      ++m_failed;
      return trees;
    }
    for (int q = 0; q < Q; ++q) {
      PartitionTree &t = trees[(size_t)q];
      t.nodes.assign(nodes.begin() + first[(size_t)q], nodes.begin() + first[(size_t)q + 1]);
      t.leafMap.assign(maps.begin() + (long)((size_t)q * mapBytes), maps.begin() + (long)(((size_t)q + 1) * mapBytes));
      t.mapW = mapW; t.mapH = mapH;
      for (const mlt_tree_node &nd : t.nodes)
        if (nd.split_mode < 0) ++m_gated;
    }
    return trees;
  }

  // The partition trees of SEVERAL picture pairs of one geometry under several QPs each from one call (include/mltcnn.h: mlt_predict_trees_sweep): one descent
  // over the unions of all entries, the conv trunk once per union node.  pics[p] = {org, pred, poc, qp OFFSET of the entry}; tree [p][q] is what predictTree
  // returns for entry p with qp = pics[p].qp + qps[q].  unionNodesOpt: [pics.size()][4].  On failure every tree is EMPTY (the result still has one row per
  // entry and one tree per QP).
  std::vector<std::vector<PartitionTree>> predictTreesSweep(const std::vector<mlt_tree_picture> &pics, int width, int height, const std::vector<int32_t> &qps,
                                                            int topSize = 128, int minSize = 16, bool byCandidates = false, int32_t *unionNodesOpt = nullptr) {
    Timer tm(this, 0, 0);
    const int P = (int)pics.size(), Q = (int)qps.size(), per = mlt_tree_max_nodes(width, height, topSize, minSize);
    const long long slices = (long long)P * Q, cap = slices * per;
    std::vector<std::vector<PartitionTree>> trees((size_t)P, std::vector<PartitionTree>((size_t)Q));
    mlt_tree_config cfg{};
    cfg.struct_size = (uint32_t)sizeof cfg;
    cfg.top_size = topSize; cfg.min_size = minSize;
    cfg.flags = byCandidates ? MLT_TREE_BY_CANDIDATES : 0u;
    const int mapW = width / 16, mapH = height / 16;
    const size_t mapBytes = (size_t)mapW * (size_t)mapH;
    std::vector<mlt_tree_node> nodes;
    std::vector<uint8_t> maps;
    std::vector<int32_t> first((size_t)slices + 1, 0);
    const bool sized = P >= 1 && P <= MLT_TREES_MAX_PICTURES && Q >= 1 && Q <= MLT_SWEEP_MAX_QPS && per > 0 && cap <= 0x7fffffff;
    if (sized) { nodes.resize((size_t)cap); maps.assign((size_t)slices * mapBytes, (uint8_t)0xFF); }
    if (!m_ctx || !sized || mlt_predict_trees_sweep(m_ctx, P, pics.data(), &cfg, qps.data(), Q, nodes.data(), (int)cap, first.data(), unionNodesOpt, maps.data(), nullptr, 0,
                                                    nullptr, nullptr) != MLT_OK) {
      std::fprintf(stderr, "error\n");  // EncCu.cpp:925
      ++m_failed;
      return trees;
    }
    for (long long s = 0; s < slices; ++s) {
      PartitionTree &t = trees[(size_t)(s / Q)][(size_t)(s % Q)];
      t.nodes.assign(nodes.begin() + first[(size_t)s], nodes.begin() + first[(size_t)s + 1]);
      t.leafMap.assign(maps.begin() + (long)((size_t)s * mapBytes), maps.begin() + (long)(((size_t)s + 1) * mapBytes));
      t.mapW = mapW; t.mapH = mapH;
      for (const mlt_tree_node &nd : t.nodes)
        if (nd.split_mode < 0) ++m_gated;
    }
    return trees;
  }

  // The class indices a candidate record keeps, most probable first (classes[] holds up to 8); returns how many.
  static int keptClasses(const mlt_candidates &c, int classes[8]) {
    int n = 0;
    for (int r = 0; r < 8; ++r)
      if (c.order[r] >= 0 && ((c.mask >> c.order[r]) & 1u)) classes[n++] = c.order[r];
    return n;
  }

  // MLTCNN_CANDIDATES' value -> policies for {128, 64, 32, 16}: "c[/m]" (every size) or "S:c[/m],S:c[/m],..." (sizes not named: the default (0, 0)), each
  // 0 <= c < 1 and 0 <= m <= 6 (the library checks m against the size's decision head).  Pure host logic; false (every policy at its default) for anything malformed.
  static bool parseCandidates(const char *spec, float cov[4], int maxModes[4]) {
    static const int sizes[4] = {128, 64, 32, 16};
    for (int i = 0; i < 4; ++i) { cov[i] = 0.f; maxModes[i] = 0; }
    // one "c[/m]" item ending at ',' or the end of the string
    auto item = [](const char *p, const char **next, float *c, int *m) -> bool {
      char *end = nullptr;
      const float v = std::strtof(p, &end);
      if (end == p || !(v >= 0.f && v < 1.f)) return false;
      long mm = 0;
      if (*end == '/') {
        const char *q = end + 1;
        if (*q < '0' || *q > '9') return false;
        mm = std::strtol(q, &end, 10);
        if (mm < 0 || mm > 6) return false;
      }
      if (*end != ',' && *end != 0) return false;
      *c = v; *m = (int)mm; *next = end;
      return true;
    };
    bool ok = spec && *spec != 0;
    if (ok && !std::strchr(spec, ':')) {
      const char *end = nullptr;
      float c = 0.f; int m = 0;
      ok = item(spec, &end, &c, &m) && *end == 0;
      for (int i = 0; i < 4 && ok; ++i) { cov[i] = c; maxModes[i] = m; }
    } else if (ok) {
      const char *p = spec;
      while (ok && *p) {
        char *end = nullptr;
        const long sz = std::strtol(p, &end, 10);
        int si = -1;
        for (int i = 0; i < 4; ++i) if (sz == sizes[i]) si = i;
        ok = end != p && *end == ':' && si >= 0;
        if (!ok) break;
        const char *after = nullptr;
        ok = item(end + 1, &after, &cov[si], &maxModes[si]);
        if (!ok) break;
        p = *after ? after + 1 : after;
        if (*after == ',' && !*p) ok = false;   // trailing comma
      }
    }
    if (!ok) for (int i = 0; i < 4; ++i) { cov[i] = 0.f; maxModes[i] = 0; }
    return ok;
  }

  // MLTCNN_MIN_CONF's value -> thresholds for {128, 64, 32, 16}: "v" (every size) or "S:v,S:v,..." (sizes not named: 0 = off), each 0 <= v < 1.
  // Pure host logic; false (thr all zero) for anything malformed -- the gate then stays off.
  static bool parseMinConf(const char *spec, float thr[4]) {
    static const int sizes[4] = {128, 64, 32, 16};
    for (int i = 0; i < 4; ++i) thr[i] = 0.f;
    bool ok = spec && *spec != 0;
    if (ok && !std::strchr(spec, ':')) {
      char *end = nullptr;
      const float v = std::strtof(spec, &end);
      ok = end != spec && *end == 0 && v >= 0.f && v < 1.f;
      for (int i = 0; i < 4 && ok; ++i) thr[i] = v;
    } else if (ok) {
      const char *p = spec;
      while (ok && *p) {
        char *end = nullptr;
        const long sz = std::strtol(p, &end, 10);
        int si = -1;
        for (int i = 0; i < 4; ++i) if (sz == sizes[i]) si = i;
        ok = end != p && *end == ':' && si >= 0;
        if (!ok) break;
        p = end + 1;
        const float v = std::strtof(p, &end);
        ok = end != p && (*end == ',' || *end == 0) && v >= 0.f && v < 1.f;
        if (!ok) break;
        thr[si] = v;
        p = *end ? end + 1 : end;
        if (*end == ',' && !*p) ok = false;   // trailing comma
      }
    }
    if (!ok) for (int i = 0; i < 4; ++i) thr[i] = 0.f;
    return ok;
  }

 private:
  void applyMinConf(const char *spec) {
    static const int sizes[4] = {128, 64, 32, 16};
    float thr[4];
    if (!parseMinConf(spec, thr)) {
      std::fprintf(stderr, "mltcnn: MLTCNN_MIN_CONF=\"%s\" is malformed (want 0 <= v < 1, \"v\" or \"128:v,64:v,...\"): confidence gate off\n", spec);
      return;
    }
    for (int i = 0; i < 4; ++i) {
      if (!(m_mask & (1u << i)) || thr[i] <= 0.f) continue;
      if (mlt_set_confidence_gate(m_ctx, sizes[i], thr[i]) == MLT_OK) m_gateSet = true;
      else std::fprintf(stderr, "mltcnn: confidence gate for size %d not set: %s\n", sizes[i], mlt_last_error(m_ctx));
    }
  }

  void applyCandidates(const char *spec) {
    static const int sizes[4] = {128, 64, 32, 16};
    float cov[4];
    int mx[4];
    if (!parseCandidates(spec, cov, mx)) {
      std::fprintf(stderr, "mltcnn: MLTCNN_CANDIDATES=\"%s\" is malformed (want \"c[/m]\" or \"128:c[/m],64:c[/m],...\", 0 <= c < 1, 0 <= m <= 6): default candidate policy\n", spec);
      return;
    }
    for (int i = 0; i < 4; ++i) {
      if (!(m_mask & (1u << i)) || (cov[i] <= 0.f && mx[i] == 0)) continue;
      if (mlt_set_candidate_policy(m_ctx, sizes[i], cov[i], mx[i]) == MLT_OK) m_policySet = true;
      else std::fprintf(stderr, "mltcnn: candidate policy for size %d not set: %s\n", sizes[i], mlt_last_error(m_ctx));
    }
  }
  // a failed candidate call: every class of the decision head kept (the encoder tests everything; this class configures the reference's heads: element [2] of the
  // 128 model, four classes, element [0] otherwise, two), no prediction in the decision record
  static void failCandidates(int cuw, mlt_candidates *out, mlt_decision *decOpt) {
    *out = mlt_candidates{};
    const int k = cuw == 128 ? 4 : 2;
    out->mask = (1u << k) - 1u;
    out->count = k;
    for (int r = 0; r < 8; ++r) out->order[r] = (int8_t)(r < k ? r : -1);
    if (decOpt) { *decOpt = mlt_decision{}; decOpt->split_mode = decOpt->raw_mode = -1; }
  }

  // one record per call: int32 {magic 0x4D4C5443, cuw, poc, qp, split, nLogits}, float logits[MLT_MAX_LOGITS], int16 org[cuw*cuw], int16 pred[cuw*cuw]
  // -- built in a buffer and written with ONE write(2) on an O_APPEND descriptor (atomic with respect to other appenders: predictors
  // of several EncCu threads share one dump file); a failed write is reported once.
  void dumpCall(const Pel *org, int orgStride, const Pel *pred, int predStride, int cuw, int poc, int cuQP, int split, const float *lg) const {
#ifdef MLTCNN_TEST_HOOKS
    const int32_t hdr[6] = {0x4D4C5443, cuw, poc, cuQP, split, mlt_num_logits(cuw)};
    std::vector<char> rec(sizeof hdr + sizeof(float) * MLT_MAX_LOGITS + 2 * sizeof(Pel) * (size_t)cuw * cuw);
    char *w = rec.data();
    std::memcpy(w, hdr, sizeof hdr); w += sizeof hdr;
    std::memcpy(w, lg, sizeof(float) * MLT_MAX_LOGITS); w += sizeof(float) * MLT_MAX_LOGITS;
    for (int pl = 0; pl < 2; ++pl)
      for (int y = 0; y < cuw; ++y) {
        const Pel *src = (pl ? pred : org) + (ptrdiff_t)y * (pl ? predStride : orgStride);
        std::memcpy(w, src, sizeof(Pel) * (size_t)cuw); w += sizeof(Pel) * (size_t)cuw;
      }
    const int fd = ::open(m_dumpPath.c_str(), O_WRONLY | O_CREAT | O_APPEND, 0644);
    const bool ok = fd >= 0 && ::write(fd, rec.data(), rec.size()) == (ssize_t)rec.size();
    if (fd >= 0) ::close(fd);
    if (!ok && !m_dumpFailed) { m_dumpFailed = true; std::fprintf(stderr, "mltcnn: cannot append to %s\n", m_dumpPath.c_str()); }
#else
    (void)org; (void)orgStride; (void)pred; (void)predStride; (void)cuw; (void)poc; (void)cuQP; (void)split; (void)lg;
#endif
  }

  // MLTCNN_STATS: wall-clock inside the predictor, per entry point (0 predict, 1 submit, 2 wait, 3 flush)
  struct Timer {
    SplitPredictor *p; int k; std::chrono::steady_clock::time_point t0;
    Timer(SplitPredictor *pp, int kk, int cuw) : p(pp->m_stats ? pp : nullptr), k(kk) {
      if (!p) return;
      t0 = std::chrono::steady_clock::now();
      if (cuw) ++p->m_bySize[cuw == 128 ? 0 : cuw == 64 ? 1 : cuw == 32 ? 2 : 3];
    }
    ~Timer() { if (p) { p->m_t[k] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); ++p->m_n[k]; } }
  };
  bool m_stats = false;
  unsigned long long m_n[4] = {0, 0, 0, 0}, m_bySize[4] = {0, 0, 0, 0}, m_failed = 0;
  double m_t[4] = {0, 0, 0, 0};
  unsigned long long m_gated = 0;   // calls the confidence gate withheld (split -1 from a call that succeeded)
  bool m_gateSet = false;           // MLTCNN_MIN_CONF set a gate on at least one size
  unsigned long long m_keptModes = 0;   // sum of the counts predictCandidates / waitCandidates returned
  bool m_policySet = false;         // MLTCNN_CANDIDATES set a policy on at least one size
  double m_initSeconds = 0.0;   // wall-clock of mlt_init (weights + load-time calibration): what an encoder process pays once

  mlt_ctx *m_ctx = nullptr;
  uint32_t m_mask = MLT_SIZE_128;
  bool m_faultInject = false;   // (only ever set with MLTCNN_TEST_HOOKS)
  int m_forceSplit = -1;        // (only ever set with MLTCNN_TEST_HOOKS)
  mutable bool m_dumpFailed = false;
  std::string m_dumpPath;
};

}  // namespace mlt
