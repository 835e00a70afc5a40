// mlt_api.cpp -- C ABI (include/mltcnn.h) of the MI355X MLT-CNN split predictor: init / shutdown / stream, the predict entry points, deferred prediction,
// confidence gate, profile.  The host runtime under them is declared in mlt_runtime.h (dispatcher, guards, loader: one translation unit each).
//
// Replaces the inline block EncCu.cpp:799-930 of the reference encoder: what was
//   xMalloc + copy loops (:810-830), cv::absdiff/convertTo/clip (:832-867), from_blob/cat/.to(kCUDA) (:869-887),
//   torch::jit::load PER CALL (:894-900), forward (:909), .cpu()/argmax (:920-921)
// becomes: one init (weights folded, packed, resident in HBM), then per call a strided H2D copy of the two
// Pel planes, a fixed chain of HIP kernel launches on one stream, and a few bytes D2H.
// There is NO CPU fallback: without a usable HIP device mlt_init fails with MLT_ERR_NO_DEVICE.
#include "mlt_runtime.h"

namespace {

std::string g_init_error;
std::mutex g_mutex;

}  // namespace

int GrowBuf::reserve(mlt_ctx *ctx, size_t want, const char *what, bool zero) {
  if (want <= bytes) return MLT_OK;
  if (p) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); release(); }
  const hipError_t e = pinned ? hipHostMalloc((void **)&p, want, hipHostMallocDefault) : hipMalloc((void **)&p, want);
  if (e != hipSuccess) { p = nullptr; ctx->err = std::string(what) + ": " + hipGetErrorString(e); return e == hipErrorOutOfMemory ? MLT_ERR_NOMEM : MLT_ERR_HIP; }
  bytes = want;
  if (zero) HIP_TRY(ctx, hipMemset(p, 0, want));
  return MLT_OK;
}

extern "C" {
#pragma GCC visibility push(default)

int mlt_abi_version(void) { return MLT_ABI_VERSION; }

// Signature of the sources this binary was built from (fastintercu-vvc_amd/build.py passes -DMLT_SOURCE_SIG; the marker is also what build.py's
// stale() greps the file for): the host side refuses a library that does not match the csrc/ beside it.
#ifndef MLT_SOURCE_SIG
#define MLT_SOURCE_SIG "unsigned-build!!"
#endif
static const char g_source_sig[] = "MLTCNN_SOURCE_SIG=" MLT_SOURCE_SIG;
const char *mlt_build_signature(void) { return g_source_sig + sizeof("MLTCNN_SOURCE_SIG=") - 1; }

int mlt_num_logits(int size) { return size == 128 ? 9 : (size == 64 || size == 32 || size == 16) ? 15 : 0; }

const char *mlt_last_error(const mlt_ctx *ctx) { return ctx ? ctx->err.c_str() : g_init_error.c_str(); }

#pragma GCC visibility pop
}  // extern "C"
namespace {
// one context on one device (cfg->device is ignored: `device` decides)
int init_one(const mlt_config *cfg, int device, mlt_ctx **out) {
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    g_init_error = "no usable HIP device (this library has no CPU fallback)";
    return MLT_ERR_NO_DEVICE;
  }
  if (hipSetDevice(device) != hipSuccess) { g_init_error = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  mlt_ctx *ctx = new (std::nothrow) mlt_ctx();
  if (!ctx) return MLT_ERR_NOMEM;
  ctx->device = device;
  ctx->max_batch = cfg->max_batch > 0 ? cfg->max_batch : 4096;
  if (cfg->tolerance > 0.f) ctx->tolerance = cfg->tolerance;
  ctx->xlite = (cfg->flags & MLT_FLAG_EXACT_LITE) != 0;
  // decision guard: two logits that are each within `tolerance` of the reference change their difference by at most 2 x tolerance.  The
  // admission of the fast arithmetic is calibrated, not proven (the tail probes put single logits at up to ~1.1 x tolerance), so the
  // default threshold is 3 x tolerance: everything below it is re-evaluated exactly (the extra re-runs are a fraction of a per cent)
  ctx->guard_margin = cfg->guard_margin > 0.f ? cfg->guard_margin : 3.f * ctx->tolerance;
  ctx->guard_margin_configured = cfg->guard_margin > 0.f;
  if (const char *e = tuning_env("MLT_CHUNK")) { int v = std::atoi(e); if (v > 0) ctx->chunk = v; }
  ctx->guard_select_kernel = tuning_env("MLT_GUARD_SELECT_KERNEL") != nullptr;
  if (const char *e = tuning_env("MLT_STAGE_CHUNK")) { int v = std::atoi(e); if (v > 0) ctx->stage_chunk = v; }
  if (ctx->stage_chunk > ctx->chunk) ctx->stage_chunk = ctx->chunk;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { g_init_error = "hipStreamCreate failed"; delete ctx; return MLT_ERR_HIP; }
  if (hipMalloc((void **)&ctx->zero_page, 65536) != hipSuccess || hipMemset(ctx->zero_page, 0, 65536) != hipSuccess) {
    g_init_error = "zero page allocation failed";
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return MLT_ERR_NOMEM;
  }
  ctx->own_stream = true;
  {
    // the chain kernels take conv padding from DS reads beyond the LDS allocation (zeros on gfx950) instead of zero masks: probe, once
    // per context, that this device behaves so -- (ab)using the zero page as the 4-byte result slot, restored afterwards; a device that
    // does not (or MLT_NO_LDS_OOB=1) gets the masked form of the same kernels
    int ok = 0;
    const bool ran = tuning_env("MLT_NO_LDS_OOB") == nullptr && mlt_probe_lds_oob((int *)ctx->zero_page, ctx->stream) == hipSuccess &&
                     hipMemcpyAsync(&ok, ctx->zero_page, sizeof ok, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
                     hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (hipMemsetAsync(ctx->zero_page, 0, sizeof ok, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
      g_init_error = "zero page reset failed";
      (void)hipFree(ctx->zero_page);
      (void)hipStreamDestroy(ctx->stream);
      delete ctx;
      return MLT_ERR_HIP;
    }
    ctx->lds_oob_zero = ran && ok == 1;
  }
  const uint32_t mask = cfg->size_mask ? cfg->size_mask : MLT_SIZE_128;  // reference gate: 128 only (EncCu.cpp:754)
  static const int sizes[4] = {128, 64, 32, 16};
  for (int i = 0; i < 4; ++i) {
    SizeState &st = ctx->sz[i];
    st.size = sizes[i];
    st.enabled = (mask >> i) & 1u;
    // precision: 128 -> fast (single fp16 pass) unless MLT_FLAG_EXACT_128; 64/32/16 -> exact (fp16 hi+lo pairs, 3 passes)
    // unless MLT_FLAG_FAST_SMALL.  See DESIGN.md "Numerics".
    st.want_exact = st.exact = sizes[i] == 128 ? (cfg->flags & MLT_FLAG_EXACT_128) != 0 : (cfg->flags & MLT_FLAG_FAST_SMALL) == 0;
    st.margin_guard = (cfg->flags & MLT_FLAG_NO_DECISION_GUARD) == 0;  // ABI 4: on by default (MLT_FLAG_DECISION_GUARD is accepted and has no effect)
    st.flat_guard = st.cfg_flat_guard = (cfg->flags & MLT_FLAG_NO_FLAT_GUARD) == 0;
    st.cfg_mag_guard = (cfg->flags & MLT_FLAG_NO_MAGNITUDE_GUARD) == 0;
    // the calibration decides "fast or exact" for the 128 model; MLT_FLAG_FAST_SMALL is an explicit request for fast
    st.calibrate = sizes[i] == 128 && (cfg->flags & MLT_FLAG_NO_CALIBRATION) == 0;
    // Round 6: only the 64 x 64 model.  A non-exact tier brings the guards with it, and a re-run of even ONE CU costs ~0.3 ms whatever the model (the exact chain's ~25
    // dependent launches, each streaming a layer's weight planes through a few workgroups): a tier must save more than that per batch to be worth having.
    //   16 x 16: layer0 works on 8 x 8 maps -- the calibrated prefix tier saved 9 % of the exact step and its one re-run per 4096-CU batch (the decision guard's usual
    //            catch) cost 0.34 ms of 0.43: 5.30 M CU/s against 8.66 M exact (profiles/r06m_small_exact_vs_prefix.txt);
    //   32 x 32: the exact-lite tier the search ended on is 0.3 - 2 % faster than exact on content that flags nothing and 29 % slower with 5 % flat CUs in the batch
    //            (2.51 M against 3.53 M, profiles/r06n_small_exact_vs_calibrated.txt);
    //   64 x 64: layer0.0 on the fused single-pass kernel saves 16 % (1.24 M against 1.05 M exact, also on natural scenes); break-even at ~4 % flagged CUs: it stays.
    // Exact also means 2e-5 instead of 1e-4 .. 4e-4 from the oracle and no data-dependent latency.
    st.small_mix = sizes[i] == 64 && st.want_exact && (cfg->flags & MLT_FLAG_NO_CALIBRATION) == 0;
    st.head_index = cfg->head_index[i] >= 0 ? cfg->head_index[i] : (sizes[i] == 128 ? 2 : 0);  // EncCu.cpp:913-919
    if (st.enabled && cfg->weights_dir) {
      char path[1024];
      std::snprintf(path, sizeof path, "%s/MLTORPQ_splitMode_%d.mltw", cfg->weights_dir, sizes[i]);  // cf. EncCu.cpp:899
      FILE *f = std::fopen(path, "rb");
      if (!f) { g_init_error = std::string("cannot open ") + path; mlt_shutdown(ctx); return MLT_ERR_WEIGHTS; }
      std::fseek(f, 0, SEEK_END);
      long len = std::ftell(f);
      std::fseek(f, 0, SEEK_SET);
      std::vector<char> buf(len > 0 ? len : 0);
      const size_t got = len > 0 ? std::fread(buf.data(), 1, len, f) : 0;
      std::fclose(f);
      int rc = got == (size_t)len ? mlt_load_weights(ctx, sizes[i], buf.data(), buf.size()) : MLT_ERR_WEIGHTS;
      if (rc) { g_init_error = ctx->err.empty() ? std::string("short read: ") + path : ctx->err; mlt_shutdown(ctx); return rc; }
    }
  }
  *out = ctx;
  return MLT_OK;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int mlt_init(const mlt_config *cfg, mlt_ctx **out) {
  std::lock_guard<std::mutex> lock(g_mutex);
  // ABI 4 is a hard break: older, shorter structs (the 56-byte ABI-2 mlt_config) are rejected -- such a binary would also pass a
  // 32-byte mlt_arith_info to mlt_arithmetic
  if (!cfg || !out || cfg->struct_size != sizeof(mlt_config)) { g_init_error = "bad mlt_config (struct_size does not match ABI 4)"; return MLT_ERR_ARG; }
  *out = nullptr;
  const int nd = cfg->n_devices;
  if (nd < 0 || nd > MLT_MAX_DEVICES) { g_init_error = "bad mlt_config.n_devices"; return MLT_ERR_ARG; }
  mlt_ctx *ctx = nullptr;
  int rc = init_one(cfg, nd > 0 ? cfg->devices[0] : cfg->device, &ctx);
  if (rc) return rc;
  for (int i = 1; i < nd; ++i) {  // one full context per further device; weights_dir is read (and calibrated) by each
    mlt_ctx *peer = nullptr;
    if ((rc = init_one(cfg, cfg->devices[i], &peer))) { mlt_shutdown(ctx); return rc; }
    ctx->peers.push_back(peer);
  }
  *out = ctx;
  return MLT_OK;
}

int mlt_num_devices(const mlt_ctx *ctx) { return ctx ? 1 + (int)ctx->peers.size() : 0; }

mlt_ctx *mlt_device_ctx(mlt_ctx *ctx, int index) {
  if (!ctx || index < 0 || index > (int)ctx->peers.size()) return nullptr;
  return device_of(ctx, index);
}

void mlt_shutdown(mlt_ctx *ctx) {
  if (!ctx) return;
  free_pictures(ctx);   // (a picture of a multi-device context holds a plane on every peer's device)
  for (mlt_ctx *p : ctx->peers) mlt_shutdown(p);
  ctx->peers.clear();
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (auto &kv : ctx->prof)
    for (auto &ev : kv.second.ev) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  for (int i = 0; i < 4; ++i) { free_model(ctx->sz[i].model); free_model(ctx->sz[i].model_exact); free_model(ctx->sz[i].model_w2); free_model(ctx->sz[i].model_xl); }
  for (SingleCu &sg : ctx->single) {
    if (sg.exec) (void)hipGraphExecDestroy(sg.exec);
    if (sg.graph) (void)hipGraphDestroy(sg.graph);
    if (sg.h_stage) (void)hipHostFree(sg.h_stage);
    if (sg.d_stage) (void)hipFree(sg.d_stage);
  }
  for (Deferred &df : ctx->deferred) {
    if (df.h_in) (void)hipHostFree(df.h_in);
    if (df.h_out) (void)hipHostFree(df.h_out);
    if (df.d_in) (void)hipFree(df.d_in);
    if (df.d_out) (void)hipFree(df.d_out);
    for (int b = 0; b < 2; ++b) if (df.done[b]) (void)hipEventDestroy(df.done[b]);
  }
  if (ctx->ws) (void)hipFree(ctx->ws);
  if (ctx->zero_page) (void)hipFree(ctx->zero_page);
  if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
  for (int b = 0; b < 2; ++b) { if (ctx->ev_h2d[b]) (void)hipEventDestroy(ctx->ev_h2d[b]); if (ctx->ev_done[b]) (void)hipEventDestroy(ctx->ev_done[b]); }
  for (GrowBuf *buf : {&ctx->stage, &ctx->guard_dev, &ctx->gstage, &ctx->sweep_guard_dev, &ctx->tree_dev, &ctx->motion_dev, &ctx->h_res}) buf->release();
  if (ctx->tree_host) (void)hipHostFree(ctx->tree_host);
  if (ctx->guard_host) (void)hipHostFree(ctx->guard_host);
  if (ctx->ev_guard) (void)hipEventDestroy(ctx->ev_guard);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int mlt_set_stream(mlt_ctx *ctx, void *hip_stream) {
  if (!ctx) return MLT_ERR_ARG;
  // (a peer context handed out by mlt_device_ctx lives on another GPU than the current one: the replacement stream must be created there)
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  ctx->stream = nullptr;
  ctx->own_stream = false;
  if (hip_stream) {
    ctx->stream = (hipStream_t)hip_stream;
  } else {  // NULL: back to a stream owned by the context
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->own_stream = true;
  }
  return MLT_OK;
}

int mlt_synchronize(mlt_ctx *ctx) {
  if (!ctx) return MLT_ERR_ARG;
  for (mlt_ctx *p : ctx->peers) {
    const int rc = mlt_synchronize(p);
    if (rc) { ctx->err = p->err; return rc; }
  }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLT_OK;
}

// mlt_predict_batch_device / _decisions / _candidates: at least one of d_split_mode / d_dec / d_cand
static int predict_batch_device_impl(mlt_ctx *ctx, int n, int size, const void *d_org, const void *d_pred, const void *d_poc, const void *d_qp,
                                     void *d_split_mode, void *d_logits, DecisionRec *d_dec, CandRec *d_cand = nullptr) {
  if (!ctx) return MLT_ERR_ARG;
  if (n < 0 || (!d_split_mode && !d_dec && !d_cand) || (n > 0 && (!d_org || !d_pred || !d_poc || !d_qp))) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if (d_cand) st->cand_used = true;
  if (n == 0) return MLT_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  const int nl = st->model.n_logits;
  const size_t cs = (size_t)size * size;
  for (int i0 = 0; i0 < n; i0 += ctx->chunk) {
    const int c = n - i0 < ctx->chunk ? n - i0 : ctx->chunk;
    const PassIO io{Planes::dense((const int16_t *)d_org + i0 * cs, (const int16_t *)d_pred + i0 * cs, size), (const int32_t *)d_poc + i0, (const int32_t *)d_qp + i0,
                    d_split_mode ? (int32_t *)d_split_mode + i0 : nullptr, d_logits ? (float *)d_logits + (size_t)i0 * nl : nullptr, d_dec ? d_dec + i0 : nullptr, d_cand ? d_cand + i0 : nullptr};
    rc = run_checked(ctx, *st, c, io);
    if (rc) return rc;
  }
  return MLT_OK;
}

int mlt_predict_batch_device(mlt_ctx *ctx, int n, int size, const void *d_org, const void *d_pred, const void *d_poc, const void *d_qp,
                             void *d_split_mode, void *d_logits) {
  if (ctx && !d_split_mode) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return predict_batch_device_impl(ctx, n, size, d_org, d_pred, d_poc, d_qp, d_split_mode, d_logits, nullptr);
}

int mlt_predict_batch_device_decisions(mlt_ctx *ctx, int n, int size, const void *d_org, const void *d_pred, const void *d_poc, const void *d_qp,
                                       void *d_decisions, void *d_logits) {
  if (ctx && !d_decisions) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return predict_batch_device_impl(ctx, n, size, d_org, d_pred, d_poc, d_qp, nullptr, d_logits, (DecisionRec *)d_decisions);
}

int mlt_predict_batch_device_candidates(mlt_ctx *ctx, int n, int size, const void *d_org, const void *d_pred, const void *d_poc, const void *d_qp,
                                        void *d_candidates, void *d_decisions_opt, void *d_logits) {
  if (ctx && !d_candidates) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return predict_batch_device_impl(ctx, n, size, d_org, d_pred, d_poc, d_qp, nullptr, d_logits, (DecisionRec *)d_decisions_opt, (CandRec *)d_candidates);
}

// One trunk pass per chunk, the heads under every point of qps[]: slab q of each output is the device-pointer twin's result with every qp[i] = qps[q].
int mlt_predict_batch_device_sweep(mlt_ctx *ctx, int n, int size, const void *d_org, const void *d_pred, const void *d_poc, const int32_t *qps, int n_qps,
                                   void *d_split_opt, void *d_logits_opt, void *d_decisions_opt, void *d_candidates_opt) {
  if (!ctx) return MLT_ERR_ARG;
  if (n < 0 || !qps || n_qps < 1 || n_qps > MLT_SWEEP_MAX_QPS || (!d_split_opt && !d_logits_opt && !d_decisions_opt && !d_candidates_opt) || (n > 0 && (!d_org || !d_pred || !d_poc))) {
    ctx->err = "mlt_predict_batch_device_sweep: bad argument (qps, 1 <= n_qps <= 32, at least one output)";
    return MLT_ERR_ARG;
  }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if (n == 0) return MLT_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  const int nl = st->model.n_logits;
  const size_t cs = (size_t)size * size;
  SweepPart sw;
  sw.n_qps = n_qps; sw.slab = n;
  std::memcpy(sw.qps, qps, (size_t)n_qps * 4);
  for (int i0 = 0; i0 < n; i0 += ctx->chunk) {
    const int c = n - i0 < ctx->chunk ? n - i0 : ctx->chunk;
    const PassIO io{Planes::dense((const int16_t *)d_org + i0 * cs, (const int16_t *)d_pred + i0 * cs, size), (const int32_t *)d_poc + i0, nullptr,
                    d_split_opt ? (int32_t *)d_split_opt + i0 : nullptr, d_logits_opt ? (float *)d_logits_opt + (size_t)i0 * nl : nullptr,
                    d_decisions_opt ? (DecisionRec *)d_decisions_opt + i0 : nullptr, d_candidates_opt ? (CandRec *)d_candidates_opt + i0 : nullptr, sw};
    if ((rc = run_checked_sweep(ctx, *st, c, io))) return rc;
  }
  return MLT_OK;
}

static int predict_batch_single(mlt_ctx *ctx, int n, int size, const int16_t *org, const int16_t *pred, const int32_t *poc, const int32_t *qp,
                      int32_t *split_mode, float *logits, mlt_decision *dec, mlt_candidates *cand) {   // at least one of split_mode / dec / cand
  if (!ctx) return MLT_ERR_ARG;
  if (n < 0 || (!split_mode && !dec && !cand) || (n > 0 && (!org || !pred || !poc || !qp))) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if (cand) st->cand_used = true;
  if (n == 0) return MLT_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  const int nl = st->model.n_logits;
  const size_t cs = (size_t)size * size;
  // Host batches are pipelined in sub-chunks through TWO staging sets: the H2D copy of sub-chunk k+1 (copy stream) runs
  // under the kernels of sub-chunk k (compute stream).  256 MiB of planes per 4096 CUs take about as long over PCIe as the
  // network does, so the overlap is worth ~1.5x end to end when the caller's buffers are pinned (mlt_alloc_pinned).
  const int cap = n < ctx->stage_chunk ? n : ctx->stage_chunk;
  const StageSet lay(size, cap, nl, dec != nullptr, cand != nullptr);   // (the records sit beside the split modes and the logits)
  const size_t setbytes = lay.bytes();
  const int nset = n > cap ? 2 : 1;
  if ((rc = ctx->stage.reserve(ctx, nset * setbytes, "staging"))) return rc;
  if (nset == 2 && !ctx->copy_stream) {
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
      HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_h2d[b], hipEventDisableTiming));
      if (!ctx->ev_done[b]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_done[b], hipEventDisableTiming));
    }
  }
  using Set = StageSet::Ptrs;
  auto set_of = [&](int b) { return lay.at(ctx->stage.p + (size_t)b * setbytes); };
  // (the fast results of a sub-chunk, and what the exact re-run of its flagged CUs overwrites)
  auto io_of = [&](const Set &S) { return PassIO{Planes::dense(S.d_org, S.d_pred, size), S.d_poc, S.d_qp, S.d_split, logits ? S.d_lg : nullptr, S.d_dec, S.d_cand}; };
  const bool guards = st->guards();
  GuardSlot gs[2];
  if (guards)
    for (int b = 0; b < nset; ++b)
      if ((rc = guard_slot(ctx, b, cap, nl, &gs[b]))) return rc;
  // Results come back through pinned buffers owned by the context: a D2H into the caller's (usually pageable) arrays
  // would block the host until the kernels are done and serialise the next sub-chunk's H2D behind them.
  const Lay::ResultSet res(cap, nl, dec != nullptr, cand != nullptr);
  if ((rc = ctx->h_res.reserve(ctx, 2 * res.bytes(), "result staging"))) return rc;
  int pend_i0[2] = {-1, -1}, pend_c[2] = {0, 0};
  auto fetch = [&](int b, int c) -> int {  // results of set b -> pinned (asynchronous)
    const Set S = set_of(b);
    char *hb = ctx->h_res.p + (size_t)b * res.bytes();
    HIP_TRY(ctx, hipMemcpyAsync(hb + res.split.off, S.d_split, (size_t)c * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (logits) HIP_TRY(ctx, hipMemcpyAsync(hb + res.lg.off, S.d_lg, (size_t)c * nl * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (dec) HIP_TRY(ctx, hipMemcpyAsync(hb + res.dec.off, S.d_dec, (size_t)c * sizeof(DecisionRec), hipMemcpyDeviceToHost, ctx->stream));
    if (cand) HIP_TRY(ctx, hipMemcpyAsync(hb + res.cand.off, S.d_cand, (size_t)c * sizeof(CandRec), hipMemcpyDeviceToHost, ctx->stream));
    return MLT_OK;
  };
  auto flush = [&](int b) -> int {  // sub-chunk in set b has completed: guard fix-up if needed, then hand its results to the caller
    if (pend_i0[b] < 0) return MLT_OK;
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_done[b]));
    if (guards) {
      const int k = *gs[b].h_count;
      int r = check_flagged_count(ctx, k, pend_c[b]);
      if (r) return r;
      if (k > 0) {  // the set's inputs are still in place (the next H2D into it is issued after this flush)
        if ((r = guard_fixup_async(ctx, *st, k, io_of(set_of(b)), gs[b]))) return r;
        if ((r = fetch(b, pend_c[b]))) return r;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      }
    }
    const char *hb = ctx->h_res.p + (size_t)b * res.bytes();
    if (split_mode) std::memcpy(split_mode + pend_i0[b], hb + res.split.off, (size_t)pend_c[b] * 4);
    if (logits) std::memcpy(logits + (size_t)pend_i0[b] * nl, hb + res.lg.off, (size_t)pend_c[b] * nl * 4);
    if (dec) std::memcpy(dec + pend_i0[b], hb + res.dec.off, (size_t)pend_c[b] * sizeof(DecisionRec));
    if (cand) std::memcpy(cand + pend_i0[b], hb + res.cand.off, (size_t)pend_c[b] * sizeof(CandRec));
    pend_i0[b] = -1;
    return MLT_OK;
  };
  if (!ctx->ev_done[0])
    for (int b = 0; b < 2; ++b) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_done[b], hipEventDisableTiming));
  int k = 0;
  for (int i0 = 0; i0 < n; i0 += cap, ++k) {
    const int c = n - i0 < cap ? n - i0 : cap;
    const int b = nset == 2 ? (k & 1) : 0;
    const Set S = set_of(b);
    hipStream_t cps = nset == 2 ? ctx->copy_stream : ctx->stream;
    if ((rc = flush(b))) return rc;  // set b: sub-chunk k-2 fully drained (host-side wait)
    HIP_TRY(ctx, hipMemcpyAsync(S.d_org, org + (size_t)i0 * cs, cs * 2 * c, hipMemcpyHostToDevice, cps));
    HIP_TRY(ctx, hipMemcpyAsync(S.d_pred, pred + (size_t)i0 * cs, cs * 2 * c, hipMemcpyHostToDevice, cps));
    HIP_TRY(ctx, hipMemcpyAsync(S.d_poc, poc + i0, (size_t)c * 4, hipMemcpyHostToDevice, cps));
    HIP_TRY(ctx, hipMemcpyAsync(S.d_qp, qp + i0, (size_t)c * 4, hipMemcpyHostToDevice, cps));
    if (nset == 2) {
      HIP_TRY(ctx, hipEventRecord(ctx->ev_h2d[b], cps));
      HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_h2d[b], 0));
    }
    if ((rc = run_fast_async(ctx, *st, c, io_of(S), gs[b]))) return rc;
    if ((rc = fetch(b, c))) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_done[b], ctx->stream));
    pend_i0[b] = i0; pend_c[b] = c;
  }
  if ((rc = flush(k & 1))) return rc;        // older of the two pending sub-chunks first
  if ((rc = flush((k & 1) ^ 1))) return rc;
  if (nset == 2) HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLT_OK;
}

// mlt_predict_batch / _decisions / _candidates (at least one of split_mode / dec / cand)
static int predict_batch_impl(mlt_ctx *ctx, int n, int size, const int16_t *org, const int16_t *pred, const int32_t *poc, const int32_t *qp,
                              int32_t *split_mode, float *logits, mlt_decision *dec, mlt_candidates *cand = nullptr) {
  if (!ctx) return MLT_ERR_ARG;
  if (n < 0 || (!split_mode && !dec && !cand) || (n > 0 && (!org || !pred || !poc || !qp))) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if (n == 0) return MLT_OK;
  if (!ctx->peers.empty() && n > 1) {   // multi-device context: every device runs the single-device path on its shard
    const int nlg = st->model.n_logits;
    const size_t csz = (size_t)size * size;
    return run_sharded(ctx, n, [&](int g, int lo, int hi) {
      return predict_batch_single(device_of(ctx, g), hi - lo, size, org + (size_t)lo * csz, pred + (size_t)lo * csz, poc + lo, qp + lo,
                                  split_mode ? split_mode + lo : nullptr, logits ? logits + (size_t)lo * nlg : nullptr, dec ? dec + lo : nullptr, cand ? cand + lo : nullptr);
    });
  }
  return predict_batch_single(ctx, n, size, org, pred, poc, qp, split_mode, logits, dec, cand);
}

int mlt_predict_batch(mlt_ctx *ctx, int n, int size, const int16_t *org, const int16_t *pred, const int32_t *poc, const int32_t *qp,
                      int32_t *split_mode, float *logits) {
  if (ctx && !split_mode) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return predict_batch_impl(ctx, n, size, org, pred, poc, qp, split_mode, logits, nullptr);
}

int mlt_predict_batch_decisions(mlt_ctx *ctx, int n, int size, const int16_t *org, const int16_t *pred, const int32_t *poc, const int32_t *qp,
                                mlt_decision *out, float *logits) {
  if (ctx && !out) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return predict_batch_impl(ctx, n, size, org, pred, poc, qp, nullptr, logits, out);
}

int mlt_predict_batch_candidates(mlt_ctx *ctx, int n, int size, const int16_t *org, const int16_t *pred, const int32_t *poc, const int32_t *qp,
                                 mlt_candidates *out, mlt_decision *dec_opt, float *logits) {
  if (ctx && !out) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return predict_batch_impl(ctx, n, size, org, pred, poc, qp, nullptr, logits, dec_opt, out);
}

// mlt_predict / mlt_predict_decision / mlt_predict_candidates (at least one of split_mode / dec / cand)
static int predict_one(mlt_ctx *ctx, const int16_t *org, int org_stride, const int16_t *pred, int pred_stride, int size, int32_t poc, int32_t qp,
                       int32_t *split_mode, float *logits_opt, mlt_decision *dec, mlt_candidates *cand = nullptr) {
  if (!ctx) return MLT_ERR_ARG;
  if (!org || !pred || (!split_mode && !dec && !cand) || org_stride < size || pred_stride < size) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  const int nl = st->model.n_logits;
  if (cand) st->cand_used = true;
  // (a graph of its own for the calls that want the record, and one for those that want the candidate record -- which always carries the decision record along:
  // plain calls replay the launches they always did)
  SingleCu &sg = ctx->single[size_index(size) + (cand ? 8 : dec ? 4 : 0)];
  if (!sg.h_stage) {
    sg.lay = Lay::SingleLay(size, nl);
    HIP_TRY(ctx, hipHostMalloc((void **)&sg.h_stage, sg.lay.bytes(), hipHostMallocDefault));
    HIP_TRY(ctx, hipMalloc((void **)&sg.d_stage, sg.lay.bytes()));
    HIP_TRY(ctx, hipMemset(sg.d_stage + sg.lay.scalars().off, 0, sg.lay.scalars().bytes));  // the flat-guard statistic of the single-CU path starts at zero (consume-and-clear)
  }
  const Lay::SingleLay &lay = sg.lay;
  const Lay::CuFields::Ptrs H = lay.at(sg.h_stage), D = lay.at(sg.d_stage);   // (H: the pinned mirror)
  // the gather of EncCu.cpp:810-830: rows of `size` Pels out of a `stride`-Pel pitch -> dense planes (pinned)
  for (int y = 0; y < size; ++y) {
    std::memcpy(H.d_org + (size_t)y * size, org + (size_t)y * org_stride, (size_t)size * 2);
    std::memcpy(H.d_pred + (size_t)y * size, pred + (size_t)y * pred_stride, (size_t)size * 2);
  }
  *H.d_poc = poc; *H.d_qp = qp;
  HIP_TRY(ctx, hipMemcpyAsync(sg.d_stage, sg.h_stage, lay.h2d_bytes(), hipMemcpyHostToDevice, ctx->stream));
  const Lay::Field fetch = lay.fetch(dec != nullptr, cand != nullptr);   // split, flagged count, logits [, record [, candidate record]]
  const PassIO io{Planes::dense(D.d_org, D.d_pred, size), D.d_poc, D.d_qp, D.d_split, D.d_lg, (dec || cand) ? D.d_dec : nullptr, cand ? D.d_cand : nullptr};
  const bool guards = st->guards();
  int32_t *h_count = lay.g.count.in<int32_t>(sg.h_stage);
  // (d_flat was zeroed with the staging buffer and is cleared by every call's heads kernel)
  const GuardSlot g{lay.g.at(sg.d_stage), nullptr, h_count, true};
  // the kernel chain of one CU (captured into a hipGraph below); with guards the flagged count comes back in *h_count with the results
  auto chain = [&]() -> int { return run_fast_async(ctx, *st, 1, io, g); };
  const bool no_graph = tuning().no_graph;
  bool replayed = false;
  if (!no_graph && !ctx->profile && ctx->own_stream) {
    if (sg.exec && (sg.ws_gen_at_capture != ctx->ws_gen || sg.stream_at_capture != ctx->stream)) {  // workspace re-allocated since: re-capture
      (void)hipGraphExecDestroy(sg.exec); (void)hipGraphDestroy(sg.graph);
      sg.exec = nullptr; sg.graph = nullptr;
    }
    if (!sg.exec) {
      // first call: run eagerly once (allocates the workspace, configures every kernel), then capture the same chain
      if ((rc = chain())) return rc;
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        rc = chain();
        hipGraph_t gr = nullptr;
        const hipError_t ce = hipStreamEndCapture(ctx->stream, &gr);
        if (rc == MLT_OK && ce == hipSuccess && gr && hipGraphInstantiate(&sg.exec, gr, nullptr, nullptr, 0) == hipSuccess) {
          sg.graph = gr; sg.ws_gen_at_capture = ctx->ws_gen; sg.stream_at_capture = ctx->stream;
        } else {
          if (gr) (void)hipGraphDestroy(gr);
          sg.exec = nullptr;
          (void)hipGetLastError();
        }
      }
      replayed = true;  // the eager run above already produced this call's result
    } else {
      HIP_TRY(ctx, hipGraphLaunch(sg.exec, ctx->stream));
      replayed = true;
    }
  }
  if (!replayed && (rc = chain())) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(sg.h_stage + fetch.off, sg.d_stage + fetch.off, fetch.bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (guards && *h_count != 0) {  // flagged (flat content / near-tie on the decision head): re-evaluate with the exact arithmetic
    if ((rc = guard_fixup_async(ctx, *st, 1, io, g))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(sg.h_stage + fetch.off, sg.d_stage + fetch.off, fetch.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (split_mode) *split_mode = *H.d_split;
  if (logits_opt) std::memcpy(logits_opt, H.d_lg, (size_t)nl * 4);
  if (dec) std::memcpy(dec, H.d_dec, sizeof(DecisionRec));
  if (cand) std::memcpy(cand, H.d_cand, sizeof(CandRec));
  return MLT_OK;
}

int mlt_predict(mlt_ctx *ctx, const int16_t *org, int org_stride, const int16_t *pred, int pred_stride, int size, int32_t poc, int32_t qp,
                int32_t *split_mode, float *logits_opt) {
  if (ctx && !split_mode) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return predict_one(ctx, org, org_stride, pred, pred_stride, size, poc, qp, split_mode, logits_opt, nullptr);
}

int mlt_predict_decision(mlt_ctx *ctx, const int16_t *org, int org_stride, const int16_t *pred, int pred_stride, int size, int32_t poc, int32_t qp,
                         mlt_decision *out, float *logits_opt) {
  if (ctx && !out) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return predict_one(ctx, org, org_stride, pred, pred_stride, size, poc, qp, nullptr, logits_opt, out);
}

int mlt_predict_candidates(mlt_ctx *ctx, const int16_t *org, int org_stride, const int16_t *pred, int pred_stride, int size, int32_t poc, int32_t qp,
                           mlt_candidates *out, mlt_decision *dec_opt, float *logits_opt) {
  if (ctx && !out) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return predict_one(ctx, org, org_stride, pred, pred_stride, size, poc, qp, nullptr, logits_opt, dec_opt, out);
}

// ---- deferred single-CU prediction ----
namespace {
// what a pass over set b of the size's deferred buffers reads and writes, and the set's guard slot (its counter pair toggles per launch: df.phase)
struct DeferredIO {
  PassIO io;
  GuardSlot g;
  DeferredIO(SizeState *st, Deferred &df, int b) {
    char *dout = df.d_out + (size_t)b * df.out.bytes();
    const Lay::CuFields::Ptrs in = df.in.at(df.d_in + (size_t)b * df.in.bytes()), od = df.out.at(dout);
    const long cu = (long)(df.in.plane / 2);
    io = PassIO{Planes{in.d_org, in.d_pred, st->size, cu, st->size, cu}, in.d_poc, in.d_qp, od.d_split, od.d_lg, od.d_dec, df.has_cand[b] ? od.d_cand : nullptr};
    g = GuardSlot{df.out.g.at(dout), &df.phase[b], df.out.g.count.in<int32_t>(df.h_out + (size_t)b * df.out.bytes())};
  }
};

int deferred_launch(mlt_ctx *ctx, SizeState *st, Deferred &df) {  // launch the accumulating generation as one batch
  if (df.n == 0) return MLT_OK;
  const int b = (int)(df.gen & 1), n = df.n;
  char *hi = df.h_in + (size_t)b * df.in.bytes(), *di = df.d_in + (size_t)b * df.in.bytes();
  // org planes, pred planes, poc + qp: only the first n planes of each are live
  HIP_TRY(ctx, hipMemcpyAsync(di + df.in.org.off, hi + df.in.org.off, (size_t)n * df.in.plane, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(di + df.in.pred.off, hi + df.in.pred.off, (size_t)n * df.in.plane, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(di + df.in.scalars().off, hi + df.in.scalars().off, df.in.scalars().bytes, hipMemcpyHostToDevice, ctx->stream));
  df.has_cand[b] = st->cand_used;
  const DeferredIO d(st, df, b);
  const int rc = run_fast_async(ctx, *st, n, d.io, d.g);
  df.guard_pending[b] = st->guards();
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(df.h_out + (size_t)b * df.out.bytes(), df.d_out + (size_t)b * df.out.bytes(), df.out.fetch_bytes(df.has_cand[b]), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(df.done[b], ctx->stream));
  df.n_launched[b] = n;
  df.gen_of_set[b] = df.gen;
  ++df.gen;
  df.n = 0;
  return MLT_OK;
}

// first mlt_wait on a finished batch: re-evaluate its flagged CUs with the exact arithmetic (the set's inputs stay in place
// until the set is reused two batches later)
int deferred_guard_fixup(mlt_ctx *ctx, SizeState *st, Deferred &df, int b) {
  if (!df.guard_pending[b]) return MLT_OK;
  df.guard_pending[b] = false;
  const DeferredIO d(st, df, b);
  // (the set's two selection counters came back with the results: the launch counted on one and zeroed the other -- GuardSlot.phase -- so their sum is the count)
  const int k = d.g.h_count[0] + d.g.h_count[1];
  if (k == 0) return MLT_OK;
  int rc = check_flagged_count(ctx, st->guards() ? k : -1, df.n_launched[b]);   // (a non-zero count for a size that has no guards any more is as bad)
  if (rc || (rc = guard_fixup_async(ctx, *st, k, d.io, d.g))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(df.h_out + (size_t)b * df.out.bytes(), df.d_out + (size_t)b * df.out.bytes(), df.out.fetch_bytes(df.has_cand[b]), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLT_OK;
}
}  // namespace

int mlt_submit(mlt_ctx *ctx, const int16_t *org, int org_stride, const int16_t *pred, int pred_stride, int size, int32_t poc, int32_t qp,
               mlt_ticket *ticket) {
  if (!ctx) return MLT_ERR_ARG;
  if (!ctx->peers.empty() && ticket) {  // multi-device: CUs are dealt round-robin; the ticket's top byte names the device
    const int G = 1 + (int)ctx->peers.size(), g = (int)(ctx->rr++ % (unsigned)G);
    if (g > 0) {
      mlt_ctx *p = device_of(ctx, g);
      const int rc = mlt_submit(p, org, org_stride, pred, pred_stride, size, poc, qp, ticket);
      if (rc) { ctx->err = p->err; return rc; }
      *ticket |= (mlt_ticket)g << 56;
      return MLT_OK;
    }
  }
  if (!org || !pred || !ticket || org_stride < size || pred_stride < size) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  Deferred &df = ctx->deferred[size_index(size)];
  if (!df.h_in) {
    df.in = Lay::DeferIn(size, MLT_DEFER_CAP);
    df.out = Lay::DeferOut(MLT_DEFER_CAP, st->model.n_logits);
    HIP_TRY(ctx, hipHostMalloc((void **)&df.h_in, 2 * df.in.bytes(), hipHostMallocDefault));
    HIP_TRY(ctx, hipHostMalloc((void **)&df.h_out, 2 * df.out.bytes(), hipHostMallocDefault));
    HIP_TRY(ctx, hipMalloc((void **)&df.d_in, 2 * df.in.bytes()));
    HIP_TRY(ctx, hipMalloc((void **)&df.d_out, 2 * df.out.bytes()));
    HIP_TRY(ctx, hipMemset(df.d_out, 0, 2 * df.out.bytes()));   // (the selection's counters start at zero)
    for (int b = 0; b < 2; ++b) HIP_TRY(ctx, hipEventCreateWithFlags(&df.done[b], hipEventDisableTiming));
  }
  if (df.n == MLT_DEFER_CAP && (rc = deferred_launch(ctx, st, df))) return rc;  // full: flush, start the next generation
  const int b = (int)(df.gen & 1);
  if (df.n == 0 && df.gen_of_set[b] != ~0ull) HIP_TRY(ctx, hipEventSynchronize(df.done[b]));  // set b's previous batch fully drained
  char *hi = df.h_in + (size_t)b * df.in.bytes();
  char *ho = hi + df.in.org.off + (size_t)df.n * df.in.plane, *hp = hi + df.in.pred.off + (size_t)df.n * df.in.plane;
  for (int y = 0; y < size; ++y) {  // the gather of EncCu.cpp:810-830
    std::memcpy(ho + (size_t)y * size * 2, org + (size_t)y * org_stride, (size_t)size * 2);
    std::memcpy(hp + (size_t)y * size * 2, pred + (size_t)y * pred_stride, (size_t)size * 2);
  }
  df.in.at(hi).d_poc[df.n] = poc;
  df.in.at(hi).d_qp[df.n] = qp;
  *ticket = df.gen * MLT_DEFER_CAP + (uint64_t)df.n;
  ++df.n;
  return MLT_OK;
}

int mlt_flush(mlt_ctx *ctx, int size) {
  if (!ctx) return MLT_ERR_ARG;
  for (mlt_ctx *p : ctx->peers) {
    const int rc = mlt_flush(p, size);
    if (rc) { ctx->err = p->err; return rc; }
  }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  Deferred &df = ctx->deferred[size_index(size)];
  return df.h_in ? deferred_launch(ctx, st, df) : MLT_OK;
}

// mlt_wait / mlt_wait_decision / mlt_wait_candidates (at least one of split_mode / dec / cand)
static int wait_impl(mlt_ctx *ctx, int size, mlt_ticket ticket, int32_t *split_mode, float *logits_opt, mlt_decision *dec, mlt_candidates *cand = nullptr) {
  if (!ctx) return MLT_ERR_ARG;
  if (!ctx->peers.empty()) {
    const int g = (int)(ticket >> 56);
    if (g > (int)ctx->peers.size()) { ctx->err = "unknown ticket"; return MLT_ERR_ARG; }
    if (g > 0) {
      mlt_ctx *p = device_of(ctx, g);
      const int rc = wait_impl(p, size, ticket & (((mlt_ticket)1 << 56) - 1), split_mode, logits_opt, dec, cand);
      if (rc) ctx->err = p->err;
      return rc;
    }
  }
  if (!split_mode && !dec && !cand) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if (cand) st->cand_used = true;   // (before a still accumulating batch is launched below: it then carries the candidate records)
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  Deferred &df = ctx->deferred[size_index(size)];
  const uint64_t gen = ticket / MLT_DEFER_CAP;
  const int slot = (int)(ticket % MLT_DEFER_CAP), b = (int)(gen & 1), nl = st->model.n_logits;
  if (!df.h_in || gen > df.gen || (gen == df.gen && slot >= df.n)) { ctx->err = "unknown ticket"; return MLT_ERR_ARG; }
  if (gen == df.gen && (rc = deferred_launch(ctx, st, df))) return rc;  // still accumulating: launch it now
  if (df.gen_of_set[b] != gen || slot >= df.n_launched[b]) { ctx->err = "ticket expired (two newer batches were started)"; return MLT_ERR_ARG; }
  if (cand && !df.has_cand[b]) { ctx->err = "the ticket's batch was flushed before the size had a candidate policy or a candidate call: it carries no candidate records"; return MLT_ERR_ARG; }
  HIP_TRY(ctx, hipEventSynchronize(df.done[b]));
  if ((rc = deferred_guard_fixup(ctx, st, df, b))) return rc;
  const Lay::CuFields::Ptrs oh = df.out.at(df.h_out + (size_t)b * df.out.bytes());   // (the pinned mirror)
  if (split_mode) *split_mode = oh.d_split[slot];
  if (logits_opt) std::memcpy(logits_opt, oh.d_lg + (size_t)slot * nl, (size_t)nl * 4);
  if (dec) std::memcpy(dec, oh.d_dec + slot, sizeof(DecisionRec));
  if (cand) std::memcpy(cand, oh.d_cand + slot, sizeof(CandRec));
  return MLT_OK;
}

int mlt_wait(mlt_ctx *ctx, int size, mlt_ticket ticket, int32_t *split_mode, float *logits_opt) {
  if (ctx && !split_mode) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return wait_impl(ctx, size, ticket, split_mode, logits_opt, nullptr);
}

int mlt_wait_decision(mlt_ctx *ctx, int size, mlt_ticket ticket, mlt_decision *out, float *logits_opt) {
  if (ctx && !out) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return wait_impl(ctx, size, ticket, nullptr, logits_opt, out);
}

int mlt_wait_candidates(mlt_ctx *ctx, int size, mlt_ticket ticket, mlt_candidates *out, mlt_decision *dec_opt, float *logits_opt) {
  if (ctx && !out) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  return wait_impl(ctx, size, ticket, nullptr, logits_opt, dec_opt, out);
}

int mlt_set_confidence_gate(mlt_ctx *ctx, int size, float min_confidence) {
  if (!ctx) return MLT_ERR_ARG;
  if (!(min_confidence >= 0.f && min_confidence < 1.f)) { ctx->err = "mlt_set_confidence_gate: threshold must be in [0, 1)"; return MLT_ERR_ARG; }   // (NaN fails the test)
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  for (mlt_ctx *p : ctx->peers)
    if ((rc = mlt_set_confidence_gate(p, size, min_confidence))) { ctx->err = p->err; return rc; }
  // mlt_predict's captured graphs bake the heads kernel's arguments in -- the threshold among them: dropped like after a reload, re-captured by the next call
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  drop_graphs(ctx, size_index(size));
  // deferred batches already launched keep the threshold they were launched with: their pending exact re-runs happen now, not at their first mlt_wait
  Deferred &df = ctx->deferred[size_index(size)];
  for (int b = 0; b < 2; ++b)
    if (df.guard_pending[b] && (rc = deferred_guard_fixup(ctx, st, df, b))) return rc;
  st->min_conf = min_confidence;
  return MLT_OK;
}

int mlt_get_confidence_gate(mlt_ctx *ctx, int size, float *min_confidence) {
  if (!ctx) return MLT_ERR_ARG;
  if (!min_confidence) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  SizeState *st;
  const int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  *min_confidence = st->min_conf;
  return MLT_OK;
}

int mlt_set_candidate_policy(mlt_ctx *ctx, int size, float coverage, int max_modes) {
  if (!ctx) return MLT_ERR_ARG;
  if (!(coverage >= 0.f && coverage < 1.f)) { ctx->err = "mlt_set_candidate_policy: coverage must be in [0, 1)"; return MLT_ERR_ARG; }   // (NaN fails the test)
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if (max_modes < 0 || max_modes > st->model.heads[st->head_index].classes) { ctx->err = "mlt_set_candidate_policy: max_modes must be in [0, classes of the decision head]"; return MLT_ERR_ARG; }
  for (mlt_ctx *p : ctx->peers)
    if ((rc = mlt_set_candidate_policy(p, size, coverage, max_modes))) { ctx->err = p->err; return rc; }
  // as for the gate: the one-CU graphs bake the policy into the heads kernel's arguments, and deferred batches already launched keep the policy they were
  // launched with -- their pending exact re-runs happen now
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  drop_graphs(ctx, size_index(size));
  Deferred &df = ctx->deferred[size_index(size)];
  for (int b = 0; b < 2; ++b)
    if (df.guard_pending[b] && (rc = deferred_guard_fixup(ctx, st, df, b))) return rc;
  st->cand_cov = coverage; st->cand_max = max_modes;
  st->cand_used = true;
  return MLT_OK;
}

int mlt_get_candidate_policy(mlt_ctx *ctx, int size, float *coverage, int *max_modes) {
  if (!ctx) return MLT_ERR_ARG;
  if (!coverage || !max_modes) { ctx->err = "bad argument"; return MLT_ERR_ARG; }
  SizeState *st;
  const int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  *coverage = st->cand_cov; *max_modes = st->cand_max;
  return MLT_OK;
}

void *mlt_alloc_pinned(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}

void mlt_free_pinned(void *p) { if (p) (void)hipHostFree(p); }

int mlt_profile_enable(mlt_ctx *ctx, int on) {
  if (!ctx) return MLT_ERR_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (auto &kv : ctx->prof)
    for (auto &ev : kv.second.ev) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  ctx->prof.clear();
  ctx->prof_order.clear();
  ctx->profile = on != 0;
  return MLT_OK;
}

int mlt_profile_read(mlt_ctx *ctx, mlt_kernel_time *out, int cap) {
  if (!ctx) return -1;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
  int i = 0;
  for (const std::string &name : ctx->prof_order) {
    ProfAcc &acc = ctx->prof[name];
    if (out && i < cap) {
      mlt_kernel_time &t = out[i];
      std::memset(&t, 0, sizeof t);
      std::snprintf(t.name, sizeof t.name, "%s", name.c_str());
      t.launches = acc.launches; t.flops = acc.flops; t.bytes = acc.bytes;
      float total = 0.f;
      for (auto &ev : acc.ev) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) total += ms; }
      t.total_ms = total;
    }
    ++i;
  }
  return i;
}

#pragma GCC visibility pop
}  // extern "C"
