// mlt_motion.cpp -- prediction pictures on the device (include/mltcnn.h): mlt_motion_blocks, mlt_picture_download, mlt_picture_compensate, mlt_picture_predict,
// mlt_picture_compensate_refs, mlt_picture_predict_refs.
//
// The whole-picture calls (mlt_predict_at, the tree calls and their sweeps) take an original and a PREDICTION picture; a caller that holds originals only makes the
// prediction here: an integer-sample block motion search of the current picture in a reference picture (motion_search_kernel) and quarter-sample compensation of
// the reference with the field (picture_compensate_kernel), or the compensation alone with a field of the caller's.  The field of a call lives in a grow-only
// device buffer of each device's context between the two kernels; both kernels run on every device of the context (integer arithmetic: the same bytes everywhere),
// so the result has a plane per device like an uploaded picture.  Everything is checked before anything is enqueued.
// The _refs forms: one integer search per reference (motion_search_kernel, unmodified, into slice r of the field buffer), motion_refine_kernel refines every
// reference's integer winner over the quarter-sample window and picks the block's (reference, vector), picture_compensate_kernel in its table form writes dst.
#include "mlt_runtime.h"

namespace {

struct MotionGeo { int block, block_l, bx, by; size_t blocks; };

int block_count(int width, int height, int block, int *bx, int *by) {
  if (block != 8 && block != 16 && block != 32 && block != 64) return 0;
  if (width < 1 || height < 1 || width > kPictureMaxDim || height > kPictureMaxDim) return 0;
  const int nx = (width + block - 1) / block, ny = (height + block - 1) / block;
  if (bx) *bx = nx;
  if (by) *by = ny;
  return nx * ny;   // <= 2048 x 2048
}

// what both calls check of the config and of the pictures (`search`: range and lambda count); fills geo
int check_motion(mlt_ctx *ctx, const char *who, const mlt_motion_config *cfg, bool search, const mlt_picture *cur, const mlt_picture *ref, const mlt_picture *dst, MotionGeo *geo) {
  const std::string w(who);
  if (!cfg || !ref || !dst || (search && !cur)) { ctx->err = w + ": NULL config or picture"; return MLT_ERR_ARG; }
  if (cfg->struct_size != sizeof(mlt_motion_config)) { ctx->err = w + ": mlt_motion_config.struct_size is not this library's (20)"; return MLT_ERR_ARG; }
  const int block = cfg->block == 0 ? 16 : cfg->block;
  if (block != 8 && block != 16 && block != 32 && block != 64) { ctx->err = w + ": block must be 8, 16, 32 or 64 (0: 16)"; return MLT_ERR_ARG; }
  if (cfg->flags != 0) { ctx->err = w + ": flags must be 0"; return MLT_ERR_ARG; }
  if (search && (cfg->range < 0 || cfg->range > 64 || cfg->lambda < 0 || cfg->lambda > 65535)) { ctx->err = w + ": 0 <= range <= 64 and 0 <= lambda <= 65535"; return MLT_ERR_ARG; }
  if (!owns_picture(ctx, ref) || !owns_picture(ctx, dst) || (search && !owns_picture(ctx, cur))) { ctx->err = w + ": every picture must belong to this context"; return MLT_ERR_ARG; }
  if (dst == ref || dst == cur) { ctx->err = w + ": dst must be another picture than its sources"; return MLT_ERR_ARG; }
  if (!dst->owned) { ctx->err = w + ": dst must be a picture made by mlt_picture_create (a wrapped plane is the caller's and const)"; return MLT_ERR_ARG; }
  if (ref->width != dst->width || ref->height != dst->height || (search && (cur->width != dst->width || cur->height != dst->height))) {
    ctx->err = w + ": the pictures differ in width or height";
    return MLT_ERR_ARG;
  }
  geo->block = block; geo->block_l = ilog2(block);
  geo->blocks = (size_t)block_count(dst->width, dst->height, block, &geo->bx, &geo->by);
  return MLT_OK;
}

// the field buffer of one device: [blocks][2] int16, then [blocks] uint32 (both 256-byte aligned)
struct FieldBuf {
  int16_t *mv; uint32_t *cost;
  static size_t bytes(size_t blocks) { return 2 * Lay::up256(blocks * 4); }
  static FieldBuf at(char *p, size_t blocks) { return FieldBuf{(int16_t *)p, (uint32_t *)(p + Lay::up256(blocks * 4))}; }
};

// the field buffer of the _refs calls: the winners (a FieldBuf), the reference index of every block [blocks] uint8 (256-byte aligned), then one FieldBuf per
// reference for the integer searches
struct RefsFieldBuf {
  FieldBuf win; uint8_t *ref_idx; char *slices; size_t slice_bytes;
  static size_t bytes(size_t blocks, int n_refs) { return FieldBuf::bytes(blocks) * (size_t)(1 + n_refs) + Lay::up256(blocks); }
  static RefsFieldBuf at(char *p, size_t blocks) {
    const size_t fb = FieldBuf::bytes(blocks);
    return RefsFieldBuf{FieldBuf::at(p, blocks), (uint8_t *)(p + fb), p + fb + Lay::up256(blocks), fb};
  }
  FieldBuf slice(int r, size_t blocks) const { return FieldBuf::at(slices + (size_t)r * slice_bytes, blocks); }
};

// a peer's failure is reported on the context the caller holds
int fail_on(mlt_ctx *ctx, mlt_ctx *dev, int rc) {
  if (dev != ctx) ctx->err = "device " + std::to_string(dev->device) + ": " + dev->err;
  return rc;
}

// refs_opt / d_ref_idx_opt: the table form (block b reads refs_opt[d_ref_idx_opt[b]]); without a table every block reads `ref`
int enqueue_compensate(mlt_ctx *dev, const MotionGeo &geo, const mlt_picture *ref, mlt_picture *dst, int g, const int16_t *d_mv, const mlt_picture *const *refs_opt = nullptr,
                       int n_refs = 0, const uint8_t *d_ref_idx_opt = nullptr) {
  PictureCompensateArgs ca{};
  ca.ref = ref->plane[(size_t)g]; ca.ref_pitch = ref->pitch;
  if (d_ref_idx_opt) {
    ca.ref_idx = d_ref_idx_opt;
    for (int r = 0; r < MLT_MOTION_MAX_REFS; ++r) {   // entries behind n_refs repeat refs[0]: never selected, never a wild pointer
      const mlt_picture *p = refs_opt[r < n_refs ? r : 0];
      ca.refs[r] = p->plane[(size_t)g]; ca.ref_pitches[r] = p->pitch;
    }
  }
  ca.dst = dst->plane[(size_t)g]; ca.dst_pitch = dst->pitch;
  ca.vec_dst = (((uintptr_t)ca.dst & 15) == 0 && (dst->pitch & 7) == 0) ? 1 : 0;
  ca.width = dst->width; ca.height = dst->height; ca.block_l = geo.block_l; ca.bx = geo.bx; ca.by = geo.by; ca.mv = d_mv;
  // algorithmic bytes: every sample of the reference read once and of the prediction written once, a vector per block read
  const double bytes = (double)dst->width * dst->height * 2 * 2 + (double)geo.blocks * (d_ref_idx_opt ? 5 : 4);
  PROF_LAUNCH_TRY(dev, "picture_compensate", 0.0, bytes, mlt_launch_picture_compensate(ca, dev->stream));
  return MLT_OK;
}

int enqueue_search(mlt_ctx *dev, const MotionGeo &geo, int range, int lambda, const mlt_picture *cur, const mlt_picture *ref, int g, const FieldBuf &f) {
  MotionSearchArgs sa{};
  sa.cur = cur->plane[(size_t)g]; sa.cur_pitch = cur->pitch; sa.ref = ref->plane[(size_t)g]; sa.ref_pitch = ref->pitch;
  sa.width = cur->width; sa.height = cur->height; sa.block_l = geo.block_l; sa.range = range; sa.lambda = lambda; sa.bx = geo.bx;
  sa.mv = f.mv; sa.cost = f.cost;
  // algorithmic bytes: both pictures read once, a vector and a cost per block written
  const double bytes = (double)cur->width * cur->height * 2 * 2 + (double)geo.blocks * 8;
  PROF_LAUNCH_TRY(dev, "motion_search", 0.0, bytes, mlt_launch_motion_search(sa, geo.by, dev->stream));
  return MLT_OK;
}

int enqueue_refine(mlt_ctx *dev, const MotionGeo &geo, const mlt_motion_refs_config *cfg, const mlt_picture *cur, const mlt_picture *const *refs, int n_refs, int g,
                   const RefsFieldBuf &f) {
  MotionRefineArgs ra{};
  ra.cur = cur->plane[(size_t)g]; ra.cur_pitch = cur->pitch;
  for (int r = 0; r < MLT_MOTION_MAX_REFS; ++r) {
    const mlt_picture *p = refs[r < n_refs ? r : 0];
    ra.refs[r] = p->plane[(size_t)g]; ra.ref_pitches[r] = p->pitch;
  }
  ra.n_refs = n_refs; ra.width = cur->width; ra.height = cur->height; ra.block_l = geo.block_l; ra.subpel = cfg->subpel; ra.lambda = cfg->lambda; ra.bx = geo.bx;
  ra.mv_int = f.slice(0, geo.blocks).mv; ra.mv_int_slice = f.slice_bytes / 2;
  ra.mv = f.win.mv; ra.cost = f.win.cost; ra.ref_out = f.ref_idx;
  // algorithmic bytes: the current picture and every reference read once, an integer vector per reference and block read, a vector, a cost and an index per block written
  const double bytes = (double)cur->width * cur->height * 2 * (1 + n_refs) + (double)geo.blocks * (4 * n_refs + 9);
  PROF_LAUNCH_TRY(dev, "motion_refine", 0.0, bytes, mlt_launch_motion_refine(ra, geo.by, dev->stream));
  return MLT_OK;
}

// what the _refs calls check (`search`: cur, range, lambda and subpel count): check_motion's checks for every reference; fills geo
int check_motion_refs(mlt_ctx *ctx, const char *who, const mlt_motion_refs_config *cfg, bool search, const mlt_picture *cur, const mlt_picture *const *refs, int n_refs,
                      const mlt_picture *dst, MotionGeo *geo) {
  const std::string w(who);
  if (!cfg || !refs || !dst) { ctx->err = w + ": NULL config or picture"; return MLT_ERR_ARG; }
  if (cfg->struct_size != sizeof(mlt_motion_refs_config)) { ctx->err = w + ": mlt_motion_refs_config.struct_size is not this library's (24)"; return MLT_ERR_ARG; }
  if (n_refs < 1 || n_refs > MLT_MOTION_MAX_REFS) { ctx->err = w + ": 1 <= n_refs <= MLT_MOTION_MAX_REFS (4)"; return MLT_ERR_ARG; }
  if (search && (cfg->subpel < 0 || cfg->subpel > 2)) { ctx->err = w + ": subpel must be 0, 1 or 2"; return MLT_ERR_ARG; }
  mlt_motion_config one{};
  one.struct_size = sizeof(one); one.block = cfg->block; one.range = cfg->range; one.lambda = cfg->lambda; one.flags = cfg->flags;
  for (int r = 0; r < n_refs; ++r)
    if (int rc = check_motion(ctx, who, &one, search, cur, refs[r], dst, geo)) return rc;
  return MLT_OK;
}

int sync_all(mlt_ctx *ctx, int G) {
  for (int g = 0; g < G; ++g) {
    mlt_ctx *dev = device_of(ctx, g);
    if (hipSetDevice(dev->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
    HIP_TRY(ctx, hipStreamSynchronize(dev->stream));
  }
  return MLT_OK;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int mlt_motion_blocks(int width, int height, int block, int *bx, int *by) { return block_count(width, height, block, bx, by); }

int mlt_picture_download(mlt_ctx *ctx, const mlt_picture *pic, int16_t *plane, int stride) {
  if (!ctx) return MLT_ERR_ARG;
  if (!pic || !plane || !owns_picture(ctx, pic) || stride < pic->width) { ctx->err = "mlt_picture_download: bad argument (a picture of this context, stride >= width)"; return MLT_ERR_ARG; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  HIP_TRY(ctx, hipMemcpy2DAsync(plane, (size_t)stride * 2, pic->plane[0], (size_t)pic->pitch * 2, (size_t)pic->width * 2, (size_t)pic->height, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLT_OK;
}

int mlt_picture_compensate(mlt_ctx *ctx, const mlt_picture *ref, const mlt_motion_config *cfg, const int16_t *mv, mlt_picture *dst) {
  if (!ctx) return MLT_ERR_ARG;
  MotionGeo geo;
  int rc = check_motion(ctx, "mlt_picture_compensate", cfg, false, nullptr, ref, dst, &geo);
  if (rc) return rc;
  if (!mv) { ctx->err = "mlt_picture_compensate: NULL motion field"; return MLT_ERR_ARG; }
  const int G = (int)dst->plane.size();
  for (int g = 0; g < G; ++g) {
    mlt_ctx *dev = device_of(ctx, g);
    if (hipSetDevice(dev->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
    if ((rc = dev->motion_dev.reserve(dev, FieldBuf::bytes(geo.blocks), "motion field"))) return fail_on(ctx, dev, rc);
    const FieldBuf f = FieldBuf::at(dev->motion_dev.p, geo.blocks);
    HIP_TRY(ctx, hipMemcpyAsync(f.mv, mv, geo.blocks * 4, hipMemcpyHostToDevice, dev->stream));
    if ((rc = enqueue_compensate(dev, geo, ref, dst, g, f.mv))) return fail_on(ctx, dev, rc);
  }
  for (int g = 0; g < G; ++g) {   // the field may be reused once every copy has read it
    mlt_ctx *dev = device_of(ctx, g);
    if (hipSetDevice(dev->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
    HIP_TRY(ctx, hipStreamSynchronize(dev->stream));
  }
  return MLT_OK;
}

int mlt_picture_predict(mlt_ctx *ctx, const mlt_picture *cur, const mlt_picture *ref, const mlt_motion_config *cfg, mlt_picture *dst, int16_t *mv_out_opt,
                        uint32_t *cost_out_opt) {
  if (!ctx) return MLT_ERR_ARG;
  MotionGeo geo;
  int rc = check_motion(ctx, "mlt_picture_predict", cfg, true, cur, ref, dst, &geo);
  if (rc) return rc;
  const int G = (int)dst->plane.size();
  for (int g = 0; g < G; ++g) {
    mlt_ctx *dev = device_of(ctx, g);
    if (hipSetDevice(dev->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
    if ((rc = dev->motion_dev.reserve(dev, FieldBuf::bytes(geo.blocks), "motion field"))) return fail_on(ctx, dev, rc);
    const FieldBuf f = FieldBuf::at(dev->motion_dev.p, geo.blocks);
    if ((rc = enqueue_search(dev, geo, cfg->range, cfg->lambda, cur, ref, g, f))) return fail_on(ctx, dev, rc);
    if ((rc = enqueue_compensate(dev, geo, ref, dst, g, f.mv))) return fail_on(ctx, dev, rc);
    if (g == 0) {   // every device finds the same field: the host's copy comes from devices[0]
      if (mv_out_opt) HIP_TRY(ctx, hipMemcpyAsync(mv_out_opt, f.mv, geo.blocks * 4, hipMemcpyDeviceToHost, dev->stream));
      if (cost_out_opt) HIP_TRY(ctx, hipMemcpyAsync(cost_out_opt, f.cost, geo.blocks * 4, hipMemcpyDeviceToHost, dev->stream));
    }
  }
  if (mv_out_opt || cost_out_opt)
    for (int g = 0; g < G; ++g) {
      mlt_ctx *dev = device_of(ctx, g);
      if (hipSetDevice(dev->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
      HIP_TRY(ctx, hipStreamSynchronize(dev->stream));
    }
  return MLT_OK;
}

int mlt_picture_compensate_refs(mlt_ctx *ctx, const mlt_picture *const *refs, int n_refs, const mlt_motion_refs_config *cfg, const int16_t *mv, const uint8_t *ref_idx_opt,
                                mlt_picture *dst) {
  if (!ctx) return MLT_ERR_ARG;
  MotionGeo geo;
  int rc = check_motion_refs(ctx, "mlt_picture_compensate_refs", cfg, false, nullptr, refs, n_refs, dst, &geo);
  if (rc) return rc;
  if (!mv) { ctx->err = "mlt_picture_compensate_refs: NULL motion field"; return MLT_ERR_ARG; }
  if (ref_idx_opt)
    for (size_t b = 0; b < geo.blocks; ++b)
      if (ref_idx_opt[b] >= n_refs) {
        ctx->err = "mlt_picture_compensate_refs: ref_idx of block (" + std::to_string(b % (size_t)geo.bx) + ", " + std::to_string(b / (size_t)geo.bx) + ") is " +
                   std::to_string((int)ref_idx_opt[b]) + ", n_refs is " + std::to_string(n_refs);
        return MLT_ERR_ARG;
      }
  const int G = (int)dst->plane.size();
  for (int g = 0; g < G; ++g) {
    mlt_ctx *dev = device_of(ctx, g);
    if (hipSetDevice(dev->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
    if ((rc = dev->motion_dev.reserve(dev, RefsFieldBuf::bytes(geo.blocks, 0), "motion field"))) return fail_on(ctx, dev, rc);
    const RefsFieldBuf f = RefsFieldBuf::at(dev->motion_dev.p, geo.blocks);
    HIP_TRY(ctx, hipMemcpyAsync(f.win.mv, mv, geo.blocks * 4, hipMemcpyHostToDevice, dev->stream));
    if (ref_idx_opt) HIP_TRY(ctx, hipMemcpyAsync(f.ref_idx, ref_idx_opt, geo.blocks, hipMemcpyHostToDevice, dev->stream));
    if ((rc = enqueue_compensate(dev, geo, refs[0], dst, g, f.win.mv, refs, n_refs, ref_idx_opt ? f.ref_idx : nullptr))) return fail_on(ctx, dev, rc);
  }
  return sync_all(ctx, G);   // the field and the table may be reused once every copy has read them
}

int mlt_picture_predict_refs(mlt_ctx *ctx, const mlt_picture *cur, const mlt_picture *const *refs, int n_refs, const mlt_motion_refs_config *cfg, mlt_picture *dst,
                             int16_t *mv_out_opt, uint8_t *ref_out_opt, uint32_t *cost_out_opt) {
  if (!ctx) return MLT_ERR_ARG;
  MotionGeo geo;
  if (!cur) { ctx->err = "mlt_picture_predict_refs: NULL config or picture"; return MLT_ERR_ARG; }
  int rc = check_motion_refs(ctx, "mlt_picture_predict_refs", cfg, true, cur, refs, n_refs, dst, &geo);
  if (rc) return rc;
  const int G = (int)dst->plane.size();
  for (int g = 0; g < G; ++g) {
    mlt_ctx *dev = device_of(ctx, g);
    if (hipSetDevice(dev->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
    if ((rc = dev->motion_dev.reserve(dev, RefsFieldBuf::bytes(geo.blocks, n_refs), "motion field"))) return fail_on(ctx, dev, rc);
    const RefsFieldBuf f = RefsFieldBuf::at(dev->motion_dev.p, geo.blocks);
    for (int r = 0; r < n_refs; ++r)
      if ((rc = enqueue_search(dev, geo, cfg->range, cfg->lambda, cur, refs[r], g, f.slice(r, geo.blocks)))) return fail_on(ctx, dev, rc);
    if ((rc = enqueue_refine(dev, geo, cfg, cur, refs, n_refs, g, f))) return fail_on(ctx, dev, rc);
    if ((rc = enqueue_compensate(dev, geo, refs[0], dst, g, f.win.mv, refs, n_refs, f.ref_idx))) return fail_on(ctx, dev, rc);
    if (g == 0) {   // every device finds the same field: the host's copy comes from devices[0]
      if (mv_out_opt) HIP_TRY(ctx, hipMemcpyAsync(mv_out_opt, f.win.mv, geo.blocks * 4, hipMemcpyDeviceToHost, dev->stream));
      if (ref_out_opt) HIP_TRY(ctx, hipMemcpyAsync(ref_out_opt, f.ref_idx, geo.blocks, hipMemcpyDeviceToHost, dev->stream));
      if (cost_out_opt) HIP_TRY(ctx, hipMemcpyAsync(cost_out_opt, f.win.cost, geo.blocks * 4, hipMemcpyDeviceToHost, dev->stream));
    }
  }
  if (mv_out_opt || ref_out_opt || cost_out_opt) return sync_all(ctx, G);
  return MLT_OK;
}

#pragma GCC visibility pop
}  // extern "C"
