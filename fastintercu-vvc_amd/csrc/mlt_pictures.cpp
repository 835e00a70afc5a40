// mlt_pictures.cpp -- device-resident pictures (include/mltcnn.h): mlt_picture_create / _upload / _wrap_device / _destroy, mlt_predict_at, mlt_grid_positions.
//
// A picture is a pitched int16 luma plane per device of its context.  mlt_predict_at validates the positions on the host, then per chunk: positions + poc + qp H2D,
// picture_gather_kernel (mlt_picture_kernels.inc) -> the dense [c][S][S] planes of a staging set, run_checked on those planes -- the launches, guards and exact
// re-runs of mlt_predict_batch_device, so every result is the dense path's bit for bit -- results D2H.  The network kernels know nothing about pictures.
// predict_at_chunks is that per-chunk pass; the tree descent (mlt_tree.cpp: mlt_predict_tree, mlt_predict_trees) runs it on position lists that already live on the device.
#include "mlt_runtime.h"

namespace {

bool owns(const mlt_ctx *ctx, const mlt_picture *pic) {
  for (const mlt_picture *p : ctx->pictures)
    if (p == pic) return true;
  return false;
}

void release(mlt_ctx *ctx, mlt_picture *pic) {
  if (pic->owned)
    for (size_t g = 0; g < pic->plane.size(); ++g)
      if (pic->plane[g]) { (void)hipSetDevice(device_of(ctx, (int)g)->device); (void)hipFree(pic->plane[g]); }
  delete pic;
}

}  // namespace

int enqueue_gather(mlt_ctx *dev, const GatherSrc &src, const int32_t *d_xy, const int32_t *d_pic, int16_t *g_org, int16_t *g_pred, int32_t *g_poc, int32_t *g_qp, int c,
                   int size) {
  // algorithmic bytes: both planes of every CU read once and written once (several pairs: + the CU's entry index read, its poc and qp written)
  const double bytes = (double)c * size * size * 2 * 2 * 2;
  if (d_pic) {
    PictureGatherMultiArgs ga{};
    ga.entries = src.entries; ga.n_entries = src.n_entries; ga.pic = d_pic; ga.xy = d_xy;
    ga.g_org = g_org; ga.g_pred = g_pred; ga.g_poc = g_poc; ga.g_qp = g_qp; ga.c = c; ga.s_l = ilog2(size);
    PROF_LAUNCH_TRY(dev, "picture_gather_multi", 0.0, bytes + (double)c * 12, mlt_launch_picture_gather_multi(ga, dev->stream));
    return MLT_OK;
  }
  const AtPlanes &pl = src.pl;
  PictureGatherArgs ga{};
  ga.org = pl.org; ga.pred = pl.pred; ga.org_pitch = pl.org_pitch; ga.pred_pitch = pl.pred_pitch; ga.vec_org = pl.org_vec; ga.vec_pred = pl.pred_vec;
  ga.xy = d_xy; ga.g_org = g_org; ga.g_pred = g_pred; ga.c = c; ga.s_l = ilog2(size);
  PROF_LAUNCH_TRY(dev, "picture_gather", 0.0, bytes, mlt_launch_picture_gather(ga, dev->stream));
  return MLT_OK;
}

// One device: CUs [0, n) of a position list from the planes this device holds (dev: the device's own context), in chunks of the pass size.  Host lists
// (mlt_predict_at): positions, poc and qp go H2D per chunk and the results D2H.  Device lists (the tree descent: at.device): the gather reads the positions where
// they are, every CU takes (poc_all, qp_all) -- or, for a list over several picture pairs (a descent over more than one picture: at.pic), its entry's planes, poc and qp from the
// device table, through picture_gather_multi_kernel -- and the network writes logits and records straight into the caller's device arrays (every store to them is a
// 4-byte or a struct store: no alignment beyond the arrays' own is assumed) -- the launches in between are the same, so are the results.
int predict_at_chunks(mlt_ctx *dev, SizeState *st, const AtPlanes &pl, int n, const AtList &at, const AtOut &out) {
  if (hipSetDevice(dev->device) != hipSuccess) { dev->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  const int size = st->size, nl = st->model.n_logits;
  if (out.cand && !at.device) st->cand_used = true;
  const int cap = n < dev->chunk ? n : dev->chunk;
  const StageSet lay(size, cap, nl, out.dec != nullptr && !at.device, out.cand != nullptr && !at.device);
  int rc;
  if ((rc = dev->stage.reserve(dev, lay.bytes() + (at.device ? 0 : Lay::up256((size_t)cap * 8)), "staging"))) return rc;   // the set, then the chunk's positions
  const StageSet::Ptrs S = lay.at(dev->stage.p);
  int32_t *d_xy = (int32_t *)(dev->stage.p + lay.bytes());
  if (at.device && !at.pic) {   // one (poc, qp) pair: filled once, every chunk reads its first c entries
    HIP_TRY(dev, hipMemsetD32Async((hipDeviceptr_t)S.d_poc, at.poc_all, (size_t)cap, dev->stream));
    HIP_TRY(dev, hipMemsetD32Async((hipDeviceptr_t)S.d_qp, at.qp_all, (size_t)cap, dev->stream));
  }
  for (int i0 = 0; i0 < n; i0 += cap) {
    const int c = n - i0 < cap ? n - i0 : cap;
    if (!at.device) {
      HIP_TRY(dev, hipMemcpyAsync(d_xy, at.xy + 2 * (size_t)i0, (size_t)c * 8, hipMemcpyHostToDevice, dev->stream));
      HIP_TRY(dev, hipMemcpyAsync(S.d_poc, at.poc + i0, (size_t)c * 4, hipMemcpyHostToDevice, dev->stream));
      HIP_TRY(dev, hipMemcpyAsync(S.d_qp, at.qp + i0, (size_t)c * 4, hipMemcpyHostToDevice, dev->stream));
    }
    // a device list: the chunk's slice of it and (several pairs) of its entry indices
    if ((rc = enqueue_gather(dev, GatherSrc{pl, at.entries, at.n_entries}, at.device ? at.xy + 2 * (size_t)i0 : d_xy, at.pic ? at.pic + i0 : nullptr, S.d_org, S.d_pred,
                             S.d_poc, S.d_qp, c, size)))
      return rc;
    // (the guards and their exact re-run read the gathered planes; the staging pointers are 256-byte aligned: CLS_QUADS whatever the picture's alignment)
    if (at.device) {
      const PassIO io{Planes::dense(S.d_org, S.d_pred, size), S.d_poc, S.d_qp, out.split ? out.split + i0 : S.d_split, out.logits ? out.logits + (size_t)i0 * nl : nullptr,
                      out.dec ? (DecisionRec *)out.dec + i0 : nullptr, out.cand ? (CandRec *)out.cand + i0 : nullptr};
      if ((rc = run_checked(dev, *st, c, io))) return rc;
      continue;   // (the stream orders this chunk's reads of the staged planes before the next chunk's gather)
    }
    const PassIO io{Planes::dense(S.d_org, S.d_pred, size), S.d_poc, S.d_qp, S.d_split, out.logits ? S.d_lg : nullptr, S.d_dec, S.d_cand};
    if ((rc = run_checked(dev, *st, c, io))) return rc;
    if (out.split) HIP_TRY(dev, hipMemcpyAsync(out.split + i0, S.d_split, (size_t)c * 4, hipMemcpyDeviceToHost, dev->stream));
    if (out.logits) HIP_TRY(dev, hipMemcpyAsync(out.logits + (size_t)i0 * nl, S.d_lg, (size_t)c * nl * 4, hipMemcpyDeviceToHost, dev->stream));
    if (out.dec) HIP_TRY(dev, hipMemcpyAsync(out.dec + i0, S.d_dec, (size_t)c * sizeof(DecisionRec), hipMemcpyDeviceToHost, dev->stream));
    if (out.cand) HIP_TRY(dev, hipMemcpyAsync(out.cand + i0, S.d_cand, (size_t)c * sizeof(CandRec), hipMemcpyDeviceToHost, dev->stream));
    HIP_TRY(dev, hipStreamSynchronize(dev->stream));   // the set is reused by the next chunk, the arrays are the caller's
  }
  return MLT_OK;
}

// predict_at_chunks for a QP sweep (host lists only): per chunk the same position upload and gather, ONE sweep pass (run_checked_sweep) into a staging set of
// n_qps slabs, then the chunk's part of every slab D2H -- element (q, i) of the caller's arrays is entry q * n_all + i; this device's CUs start at entry `first`.
static int predict_at_sweep_chunks(mlt_ctx *dev, SizeState *st, const AtPlanes &pl, int n, const int32_t *xy, const int32_t *poc, const int32_t *qps, int n_qps,
                                   const AtOut &out, size_t n_all, size_t first) {
  if (hipSetDevice(dev->device) != hipSuccess) { dev->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  const int size = st->size, nl = st->model.n_logits;
  const int cap = n < dev->chunk ? n : dev->chunk;
  const Lay::SweepStageSet lay(size, (size_t)cap, (size_t)nl, (size_t)n_qps, out.dec != nullptr, out.cand != nullptr);
  int rc;
  if ((rc = dev->stage.reserve(dev, lay.bytes() + Lay::up256((size_t)cap * 8), "staging"))) return rc;   // the set, then the chunk's positions
  const Lay::SweepStageSet::Ptrs S = lay.at(dev->stage.p);
  int32_t *d_xy = (int32_t *)(dev->stage.p + lay.bytes());
  SweepPart sw;
  sw.n_qps = n_qps; sw.slab = cap;
  std::memcpy(sw.qps, qps, (size_t)n_qps * 4);
  for (int i0 = 0; i0 < n; i0 += cap) {
    const int c = n - i0 < cap ? n - i0 : cap;
    HIP_TRY(dev, hipMemcpyAsync(d_xy, xy + 2 * (size_t)i0, (size_t)c * 8, hipMemcpyHostToDevice, dev->stream));
    HIP_TRY(dev, hipMemcpyAsync(S.d_poc, poc + i0, (size_t)c * 4, hipMemcpyHostToDevice, dev->stream));
    if ((rc = enqueue_gather(dev, GatherSrc{pl, nullptr, 0}, d_xy, nullptr, S.d_org, S.d_pred, nullptr, nullptr, c, size))) return rc;
    const PassIO io{Planes::dense(S.d_org, S.d_pred, size), S.d_poc, nullptr, S.d_split, out.logits ? S.d_lg : nullptr, S.d_dec, S.d_cand, sw};
    if ((rc = run_checked_sweep(dev, *st, c, io))) return rc;
    for (int q = 0; q < n_qps; ++q) {
      const size_t src = (size_t)q * cap, dst = (size_t)q * n_all + first + (size_t)i0;
      if (out.split) HIP_TRY(dev, hipMemcpyAsync(out.split + dst, S.d_split + src, (size_t)c * 4, hipMemcpyDeviceToHost, dev->stream));
      if (out.logits) HIP_TRY(dev, hipMemcpyAsync(out.logits + dst * nl, S.d_lg + src * nl, (size_t)c * nl * 4, hipMemcpyDeviceToHost, dev->stream));
      if (out.dec) HIP_TRY(dev, hipMemcpyAsync(out.dec + dst, (const mlt_decision *)S.d_dec + src, (size_t)c * sizeof(mlt_decision), hipMemcpyDeviceToHost, dev->stream));
      if (out.cand) HIP_TRY(dev, hipMemcpyAsync(out.cand + dst, (const mlt_candidates *)S.d_cand + src, (size_t)c * sizeof(mlt_candidates), hipMemcpyDeviceToHost, dev->stream));
    }
    HIP_TRY(dev, hipStreamSynchronize(dev->stream));   // the set is reused by the next chunk, the arrays are the caller's
  }
  return MLT_OK;
}

// What mlt_predict_at and its sweep form (and, of the pair, the one-pair tree calls) check of the picture pair and the positions before anything is enqueued
// (`who` opens the message); n > 0.
int check_at_pair(mlt_ctx *ctx, const char *who, const mlt_picture *org, const mlt_picture *pred) {
  if (!owns(ctx, org) || !owns(ctx, pred)) { ctx->err = std::string(who) + ": both pictures must belong to this context"; return MLT_ERR_ARG; }
  if (org->width != pred->width || org->height != pred->height) { ctx->err = std::string(who) + ": the two pictures differ in width or height"; return MLT_ERR_ARG; }
  return MLT_OK;
}
static int check_at_positions(mlt_ctx *ctx, const char *who, int size, const mlt_picture *org, int n, const int32_t *xy) {
  // every position, before anything is enqueued: the gather kernel trusts them
  for (int i = 0; i < n; ++i) {
    const long x = xy[2 * (size_t)i], y = xy[2 * (size_t)i + 1];
    if (x < 0 || y < 0 || x + size > org->width || y + size > org->height) {
      char msg[224];
      std::snprintf(msg, sizeof msg, "%s: position %d (x = %ld, y = %ld) puts a %d x %d CU outside the %d x %d picture", who, i, x, y, size, size, org->width, org->height);
      ctx->err = msg;
      return MLT_ERR_ARG;
    }
  }
  return MLT_OK;
}

bool owns_picture(const mlt_ctx *ctx, const mlt_picture *pic) { return owns(ctx, pic); }

void free_pictures(mlt_ctx *ctx) {
  for (mlt_picture *p : ctx->pictures) release(ctx, p);
  ctx->pictures.clear();
}

extern "C" {
#pragma GCC visibility push(default)

int mlt_picture_create(mlt_ctx *ctx, int width, int height, mlt_picture **out) {
  if (!ctx) return MLT_ERR_ARG;
  if (!out || width < kPictureMinDim || height < kPictureMinDim || width > kPictureMaxDim || height > kPictureMaxDim) { ctx->err = "mlt_picture_create: bad argument (16 <= width, height <= 16384)"; return MLT_ERR_ARG; }
  *out = nullptr;
  mlt_picture *pic = new (std::nothrow) mlt_picture();
  if (!pic) return MLT_ERR_NOMEM;
  pic->owner = ctx; pic->width = width; pic->height = height; pic->owned = true; pic->vec = true;
  pic->pitch = ((long)width + 63) / 64 * 64;
  const int G = 1 + (int)ctx->peers.size();
  pic->plane.assign((size_t)G, nullptr);
  for (int g = 0; g < G; ++g) {
    mlt_ctx *dev = device_of(ctx, g);
    hipError_t e = hipSetDevice(dev->device);
    if (e == hipSuccess) e = hipMalloc((void **)&pic->plane[(size_t)g], (size_t)height * (size_t)pic->pitch * 2);
    if (e != hipSuccess) {
      ctx->err = std::string("mlt_picture_create: ") + hipGetErrorString(e);
      release(ctx, pic);
      return e == hipErrorOutOfMemory ? MLT_ERR_NOMEM : MLT_ERR_HIP;
    }
  }
  ctx->pictures.push_back(pic);
  *out = pic;
  return MLT_OK;
}

int mlt_picture_wrap_device(mlt_ctx *ctx, const void *d_plane, int stride, int width, int height, mlt_picture **out) {
  if (!ctx) return MLT_ERR_ARG;
  if (!out || !d_plane || ((uintptr_t)d_plane & 1) || width < kPictureMinDim || height < kPictureMinDim || width > kPictureMaxDim || height > kPictureMaxDim || stride < width) {
    ctx->err = "mlt_picture_wrap_device: bad argument (2-byte aligned plane, 16 <= width, height <= 16384, stride >= width)";
    return MLT_ERR_ARG;
  }
  *out = nullptr;
  if (!ctx->peers.empty()) { ctx->err = "mlt_picture_wrap_device: a device plane lives on ONE device -- wrap it on mlt_device_ctx(ctx, i)"; return MLT_ERR_ARG; }
  mlt_picture *pic = new (std::nothrow) mlt_picture();
  if (!pic) return MLT_ERR_NOMEM;
  pic->owner = ctx; pic->width = width; pic->height = height; pic->pitch = stride; pic->owned = false;
  const uintptr_t lo = (uintptr_t)d_plane, hi = lo + (((size_t)height - 1) * (size_t)stride + (size_t)width) * 2;
  pic->vec = ((lo | hi) & 15) == 0;   // aligned 16-byte windows that hold a byte of the extent then lie inside it (mlt_picture_kernels.inc)
  pic->plane.assign(1, (int16_t *)const_cast<void *>(d_plane));
  ctx->pictures.push_back(pic);
  *out = pic;
  return MLT_OK;
}

int mlt_picture_upload(mlt_ctx *ctx, mlt_picture *pic, const int16_t *plane, int stride) {
  if (!ctx) return MLT_ERR_ARG;
  if (!pic || !plane || !owns(ctx, pic) || stride < pic->width) { ctx->err = "mlt_picture_upload: bad argument (a picture of this context, stride >= width)"; return MLT_ERR_ARG; }
  if (!pic->owned) { ctx->err = "mlt_picture_upload: a wrapped picture is the caller's memory"; return MLT_ERR_ARG; }
  const int G = (int)pic->plane.size();
  for (int g = 0; g < G; ++g) {
    mlt_ctx *dev = device_of(ctx, g);
    if (hipSetDevice(dev->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
    HIP_TRY(ctx, hipMemcpy2DAsync(pic->plane[(size_t)g], (size_t)pic->pitch * 2, plane, (size_t)stride * 2, (size_t)pic->width * 2, (size_t)pic->height, hipMemcpyHostToDevice, dev->stream));
  }
  for (int g = 0; g < G; ++g) {   // the host buffer may be reused once every copy has read it
    mlt_ctx *dev = device_of(ctx, g);
    if (hipSetDevice(dev->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
    HIP_TRY(ctx, hipStreamSynchronize(dev->stream));
  }
  return MLT_OK;
}

int mlt_picture_destroy(mlt_ctx *ctx, mlt_picture *pic) {
  if (!ctx) return MLT_ERR_ARG;
  if (!pic || !owns(ctx, pic)) { ctx->err = "mlt_picture_destroy: not a picture of this context"; return MLT_ERR_ARG; }
  for (size_t i = 0; i < ctx->pictures.size(); ++i)
    if (ctx->pictures[i] == pic) { ctx->pictures.erase(ctx->pictures.begin() + (long)i); break; }
  release(ctx, pic);   // (every call that reads a picture has synchronised before it returned; hipFree waits for the device besides)
  return MLT_OK;
}

int mlt_predict_at(mlt_ctx *ctx, int size, const mlt_picture *org, const mlt_picture *pred, int n, const int32_t *xy, const int32_t *poc, const int32_t *qp,
                   int32_t *split_mode_opt, float *logits_opt, mlt_decision *dec_opt, mlt_candidates *cand_opt) {
  if (!ctx) return MLT_ERR_ARG;
  if (n < 0 || !org || !pred || (!split_mode_opt && !logits_opt && !dec_opt && !cand_opt) || (n > 0 && (!xy || !poc || !qp))) { ctx->err = "mlt_predict_at: bad argument"; return MLT_ERR_ARG; }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if ((rc = check_at_pair(ctx, "mlt_predict_at", org, pred))) return rc;
  if (n == 0) return MLT_OK;
  if ((rc = check_at_positions(ctx, "mlt_predict_at", size, org, n, xy))) return rc;
  const AtOut out{split_mode_opt, logits_opt, dec_opt, cand_opt};
  if (!ctx->peers.empty() && n > 1)   // every device gathers from its own copy of the planes (both pictures belong to ctx: a plane per device of it)
    return run_sharded(ctx, n, [&](int g, int lo, int hi) -> int {
      mlt_ctx *dev = device_of(ctx, g);
      SizeState *sg = &dev->sz[size_index(size)];
      if (!sg->enabled || !sg->loaded) { dev->err = "CU size not enabled or weights not loaded"; return MLT_ERR_SIZE_DISABLED; }
      const AtOut o{out.split ? out.split + lo : nullptr, out.logits ? out.logits + (size_t)lo * sg->model.n_logits : nullptr, out.dec ? out.dec + lo : nullptr, out.cand ? out.cand + lo : nullptr};
      return predict_at_chunks(dev, sg, AtPlanes::of(org, pred, g), hi - lo, AtList::host(xy + 2 * (size_t)lo, poc + lo, qp + lo), o);
    });
  return predict_at_chunks(ctx, st, AtPlanes::of(org, pred, 0), n, AtList::host(xy, poc, qp), out);
}

int mlt_predict_at_sweep(mlt_ctx *ctx, int size, const mlt_picture *org, const mlt_picture *pred, int n, const int32_t *xy, const int32_t *poc,
                         const int32_t *qps, int n_qps, int32_t *split_opt, float *logits_opt, mlt_decision *dec_opt, mlt_candidates *cand_opt) {
  if (!ctx) return MLT_ERR_ARG;
  if (n < 0 || !org || !pred || !qps || n_qps < 1 || n_qps > MLT_SWEEP_MAX_QPS || (!split_opt && !logits_opt && !dec_opt && !cand_opt) || (n > 0 && (!xy || !poc))) {
    ctx->err = "mlt_predict_at_sweep: bad argument (qps, 1 <= n_qps <= 32, at least one output)";
    return MLT_ERR_ARG;
  }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if ((rc = check_at_pair(ctx, "mlt_predict_at_sweep", org, pred))) return rc;
  if (n == 0) return MLT_OK;
  if ((rc = check_at_positions(ctx, "mlt_predict_at_sweep", size, org, n, xy))) return rc;
  const AtOut out{split_opt, logits_opt, dec_opt, cand_opt};
  if (!ctx->peers.empty() && n > 1)   // every device writes its [lo, hi) range of every slab
    return run_sharded(ctx, n, [&](int g, int lo, int hi) -> int {
      mlt_ctx *dev = device_of(ctx, g);
      SizeState *sg = &dev->sz[size_index(size)];
      if (!sg->enabled || !sg->loaded) { dev->err = "CU size not enabled or weights not loaded"; return MLT_ERR_SIZE_DISABLED; }
      return predict_at_sweep_chunks(dev, sg, AtPlanes::of(org, pred, g), hi - lo, xy + 2 * (size_t)lo, poc + lo, qps, n_qps, out, (size_t)n, (size_t)lo);
    });
  return predict_at_sweep_chunks(ctx, st, AtPlanes::of(org, pred, 0), n, xy, poc, qps, n_qps, out, (size_t)n, 0);
}

int mlt_grid_positions(int width, int height, int size, int32_t *xy, int cap) {
  if (size_index(size) < 0 || width < size || height < size) return 0;
  const int cols = width / size, rows = height / size;
  const long long total = (long long)cols * rows;
  if (total > 0x7fffffff) return 0;
  for (long long i = 0; xy && i < total && i < cap; ++i) {
    xy[2 * i] = (int32_t)(i % cols) * size;
    xy[2 * i + 1] = (int32_t)(i / cols) * size;
  }
  return (int)total;
}

#pragma GCC visibility pop
}  // extern "C"
