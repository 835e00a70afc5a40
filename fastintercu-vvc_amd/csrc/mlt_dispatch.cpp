// mlt_dispatch.cpp -- the dispatcher of the host runtime: tuning switches, the activation workspace, one launch wrapper per kernel family (run_*),
// and the launch plans: what a pass launches (plan_network) and the walk that binds the workspace and enqueues it (run_network).
#include "mlt_runtime.h"

const char *tuning_env(const char *name) {
  const char *e = std::getenv("MLT_TUNING");
  return (e && e[0] == '1') ? std::getenv(name) : nullptr;
}

const Tuning &tuning() {
  static const Tuning t = [] {
    auto num = [](const char *name, long dflt) { const char *e = tuning_env(name); return e ? std::atol(e) : dflt; };
    auto on = [](const char *name) { return tuning_env(name) != nullptr; };
    auto cap = [&](const char *name) { const long v = num(name, 0); return (int)(v > 0 ? v : 256); };
    Tuning u{};
    u.debug_dump_dir = tuning_env("MLT_DEBUG_DUMP_DIR");
    u.xl_kill = (int)num("MLT_XL_KILL", 0); u.xl_kill_layer = (int)num("MLT_XL_KILL_LAYER", -1);
    u.lat_pixels = num("MLT_LAT_PIXELS", 16384L);
    u.no_exact_lat = on("MLT_NO_EXACT_LAT"); u.exact_patch_big = !on("MLT_EXACT_PATCH_64K");
    u.wg_cap = cap("MLT_WG_CAP"); u.wg_cap0 = cap("MLT_WG_CAP0"); u.wg_cap1 = cap("MLT_WG_CAP1"); u.wg_cap2 = cap("MLT_WG_CAP2");
    u.l0_mfma32 = on("MLT_L0_MFMA32"); u.l1_mfma32 = !on("MLT_L1_MFMA16");
    u.no_block_fusion = on("MLT_NO_BLOCK_FUSION");
    u.no_chain = on("MLT_NO_CHAIN") || u.no_block_fusion; u.no_chain_s2 = on("MLT_NO_CHAIN_S2"); u.no_c16 = on("MLT_NO_C16"); u.chain64 = !on("MLT_NO_CHAIN64");
    u.no_l0_s5 = on("MLT_NO_L0_S5");
    u.no_xs_handoff = on("MLT_NO_XS_HANDOFF") || u.debug_dump_dir != nullptr;   // (the layer dumps are those of the sc hand-off)
    u.no_stage256_wide = on("MLT_NO_STAGE256_WIDE");
    u.l0_stream_min = on("MLT_NO_L0_STREAM") ? 0 : (int)num("MLT_L0_STREAM_MIN", 128);
    u.l1_stream_min = on("MLT_NO_L1_STREAM") ? 0 : (int)num("MLT_L1_STREAM_MIN", 128);
    u.guard_wait_mode = on("MLT_GUARD_SPIN_WAIT") ? 1 : on("MLT_GUARD_BLOCKING_WAIT") ? 2 : 0;
    u.no_small_mix = on("MLT_NO_SMALL_MIX"); u.no_mag_guard = on("MLT_NO_MAG_GUARD");
    u.no_graph = on("MLT_NO_GRAPH") || u.debug_dump_dir != nullptr;
    return u;
  }();
  return t;
}

namespace {

int gap_slots(int hw) { return hw >= 32 ? hw / 32 : 1; }

// activation workspace (bytes per CU) for size S: 4 scratch maps of stage-0 size, one output per stage,
// fp32 GAP partial sums per head.  The stem activation is never materialised (fused into layer0.0.conv1).
size_t ws_per_cu(const mlt::Model &m, int S, bool some_exact = false) {
  const int h0 = S / 2 > 0 ? S / 2 : 1;
  const int planes = (m.exact || some_exact) ? 2 : 1;  // exact mode keeps a lo plane behind every activation
  size_t b = 4 * ((size_t)h0 * h0 * 32 * 2 * planes + 256);
  int h = S;
  for (int s = 0; s < m.n_stages; ++s) {
    h = h / 2 > 0 ? h / 2 : 1;
    b += (size_t)h * h * m.planes[s] * 2 * planes + 256;
    if (s >= 1) b += (size_t)gap_slots(h * h) * m.planes[s] * 4 + 256;
  }
  return b + 4096;
}

int ensure_ws(mlt_ctx *ctx, size_t bytes) {
  if (bytes <= ctx->ws_bytes) return MLT_OK;
  if (ctx->ws) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->ws); ctx->ws = nullptr; ctx->ws_bytes = 0; }
  ++ctx->ws_gen;
  HIP_TRY(ctx, hipMalloc((void **)&ctx->ws, bytes));
  ctx->ws_bytes = bytes;
  return MLT_OK;
}
}  // namespace
void release_ws(mlt_ctx *ctx) {  // (the caller has synchronised the stream)
  if (ctx->ws) { (void)hipFree(ctx->ws); ctx->ws = nullptr; ctx->ws_bytes = 0; }
  ++ctx->ws_gen;
}
namespace {

// MLT_DEBUG_DUMP_DIR=<dir>: after every kernel, synchronise and write the output tensor to <dir>/<seq>_<name>.bin
// (bring-up aid only; never set in production or in timed runs).
int debug_dump(mlt_ctx *ctx, const char *name, const void *dptr, size_t bytes) {
  const char *dir = tuning().debug_dump_dir;
  static int seq = 0;
  if (!dir) return MLT_OK;
  std::vector<char> host(bytes);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(host.data(), dptr, bytes, hipMemcpyDeviceToHost));
  char path[1200];
  std::snprintf(path, sizeof path, "%s/%02d_%s.bin", dir, seq++, name);
  if (FILE *f = std::fopen(path, "wb")) { std::fwrite(host.data(), 1, bytes, f); std::fclose(f); }
  return MLT_OK;
}

}  // namespace

int Launch::prof_begin(const std::string &name, double flops, double bytes, hipEvent_t &e0, hipEvent_t &e1, const char *variant) {
  if (ctx->plan) { ctx->plan->push_back(variant && variant[0] ? name + " [" + variant + "]" : name); return MLT_OK; }
  if (!ctx->profile) return MLT_OK;
  auto it = ctx->prof.find(name);
  if (it == ctx->prof.end()) { ctx->prof_order.push_back(name); it = ctx->prof.emplace(name, ProfAcc()).first; }
  it->second.launches++; it->second.flops += flops; it->second.bytes += bytes;
  HIP_TRY(ctx, hipEventCreate(&e0));
  HIP_TRY(ctx, hipEventCreate(&e1));
  it->second.ev.emplace_back(e0, e1);
  HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
  return MLT_OK;
}
int Launch::prof_end(hipEvent_t e1) {
  if (!ctx->profile) return MLT_OK;
  HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
  return MLT_OK;
}

namespace {

// plan mode with detail: append the launch's buffers to its record ("{x=ws+0x..., y=...}"; NULL pointers are left out, workspace pointers print as offsets)
void plan_note(mlt_ctx *ctx, std::initializer_list<std::pair<const char *, const void *>> ptrs, std::initializer_list<std::pair<const char *, long>> vals = {}) {
  if (!ctx->plan || !ctx->plan_detail || ctx->plan->empty()) return;
  std::string t = " {";
  char b[64];
  bool first = true;
  for (const auto &q : ptrs) {
    if (!q.second) continue;
    std::snprintf(b, sizeof b, "%s%s=0x%llx", first ? "" : " ", q.first, (unsigned long long)(uintptr_t)q.second);
    t += b; first = false;
  }
  for (const auto &q : vals) {
    std::snprintf(b, sizeof b, "%s%s=%ld", first ? "" : " ", q.first, q.second);
    t += b; first = false;
  }
  ctx->plan->back() += t + "}";
}

struct ConvIO {
  const void *x = nullptr;    // input activation (ignored when raw planes are given)
  void *y = nullptr;          // main output (may be NULL when only the GAP sums are needed)
  void *y_sc = nullptr;       // shortcut output (conv carries a shortcut)
  const void *res = nullptr;  // residual added before the ReLU
  float *gap = nullptr;       // GAP partial sums
  bool relu = false;
  bool y_c16 = false;         // main output chunk-major (ConvArgs.y_c16)
  bool ysc_c16 = false;       // shortcut output chunk-major (ConvArgs.ysc_c16)
  size_t x_lo = 0, y_lo = 0, res_lo = 0, ysc_lo = 0;  // exact mode: byte offsets hi plane -> lo plane
};

int run_conv(mlt_ctx *ctx, const mlt::PackedConv &pc, int n, int hin, const ConvIO &io, int *hout_out) {
  const int hout = hin / pc.stride > 0 ? hin / pc.stride : 1;
  *hout_out = hout;
  ConvArgs a{};
  a.x = io.x; a.y = io.y; a.w = pc.d_w; a.bias = pc.d_bias; a.res = io.res; a.n = n; a.relu = io.relu ? 1 : 0;
  a.y_sc = io.y_sc; a.bias_sc = pc.d_bias_sc; a.acc_scale = pc.acc_scale; a.y_c16 = io.y_c16 ? 1 : 0; a.ysc_c16 = io.ysc_c16 ? 1 : 0;
  a.hin_l = ilog2(hin); a.hout_l = ilog2(hout);
  a.x_lo_off = io.x_lo; a.y_lo_off = io.y_lo; a.res_lo_off = io.res_lo; a.ysc_lo_off = io.ysc_lo; a.w_lo_off = pc.plane_halves * 2;
  a.lo8_scale = 0x01010101 * ((127 - pc.lo8_exp) & 0xFF);
  a.xl_sa0 = 0x01010101 * ((127 - pc.xl_ewl) & 0xFF); a.xl_sa1 = 0x01010101 * ((127 - pc.xl_ewh) & 0xFF); a.xl_sb1 = 0x01010101 * (127 - 12);  // (12 = MLT_XL_LO_EXP, mlt_kernels.hip)
  { const int kill = tuning().xl_kill, only = tuning().xl_kill_layer;  // bring-up: E8M0 byte 0 = 2^-127 silences a K block (of one layer: cin * 1000 + cout)
    if (only < 0 || only == pc.cin * 1000 + pc.cout) { if (kill & 1) a.xl_sa0 = 0; if (kill & 2) a.xl_sb1 = 0; } }
  // LDS-DMA staging variants (fast arithmetic): resident weights on maps >= 16 x 16, weight ring on maps >= 8 x 8
  // Small batches (the encoder's one-CU-per-call use): the throughput tiling would put a whole layer on 1-4 workgroups
  // that stream all its weights through their LDS one after the other.  The latency variants cut the couts into 32-channel
  // tiles (4x more workgroups, 4x fewer weight bytes each) on the same packed weights.
  const long lat_px = tuning().lat_pixels;  // output pixels of the launch; measured crossover 13-33 k per layer; 0 disables
  // hi+lo weights on the fast tiling (MLT_MODEL_W2): its stride-1 layers with >= 64 channels have ONE per-conv form, the 32-cout x 128-pixel
  // variant (large launches of those layers go through chain_kernel<..., W2>; this is the bit-identical small-launch / fallback form)
  // (its stride-2 and 32-channel layers have ONE row on their fast tiling, DEFAULT, at any launch size)
  const bool no_exact_lat = tuning().no_exact_lat;
  const bool lat = !(pc.exact && no_exact_lat) && pc.lat && hout >= 8 && (pc.w2 ? pc.stride == 1 : (long)n * hout * hout <= lat_px);
  const int dma = (pc.exact || pc.w2 || lat) ? 0 : (pc.dma == 1 && hout >= 16) ? 1 : (pc.dma == 2 && hout >= 8) ? 2 : 0;
  const int MT = lat ? 128 : dma == 2 ? pc.mt_dma : pc.mt;
  const int nsplit = pc.xl ? 6 : pc.exact ? 2 : pc.w2 ? 4 : 1;  // (mlt_launch_conv; 6 = exact-lite: the exact arithmetic's geometry, FP8 cross terms)
  const int act_planes = (nsplit == 2 || nsplit == 6) ? 2 : 1;
  int tw = hout < 32 ? hout : 32;
  int th = MT / tw < hout ? MT / tw : hout;
  int spw = MT / (tw * th);
  const int halo = pc.taps == 9 ? 3 : 1;
  const int PS = pc.kc * 2 + 16;
  const int ph = (th - 1) * pc.stride + halo, pw = (tw - 1) * pc.stride + halo;
  // row pitch (pixels): stride 2 keeps even / odd columns in two halves; 8-wide maps need RP = 2 (mod 4) so that the
  // two rows a ds_read_b128 lane group reads sit 8 (mod 16) pixels apart (mlt_kernels.hip, lane ranking)
  int half = pc.stride == 2 ? (pw + 1) / 2 : 0;
  if (pc.stride == 2 && tw == 8 && (2 * half) % 4 != 2) ++half;
  int rp = pc.stride == 2 ? 2 * half : pw;
  if (pc.stride == 1 && tw == 8) while (rp % 4 != 2) ++rp;
  // LDS budget of the patch planes: 64 KiB -- or, for the exact arithmetic (two planes), what the two-deep weight ring of the tiling leaves of the
  // 160 KiB (round 4: the 128 -> 256 stride-2 layer on 8 x 8 maps needs 96 KiB for TWO samples per tile; with one, half of the tile's waves idled)
  size_t patch_budget = 64 * 1024;
  if (nsplit == 2 || nsplit == 6) {
    // (of the layer's throughput tiling, whose ring is the largest: the latency variants cut the same tiles, so that both compute a CU in the same tile)
    const int ring = mlt_conv_ring_bytes(pc.cin, pc.cout, pc.stride, nsplit, pc.taps == 1 ? MLT_CONV_CENTRE : MLT_CONV_DEFAULT);
    const bool big = tuning().exact_patch_big;
    if (big && ring >= 0 && ring + 64 * 1024 < 160 * 1024) patch_budget = 160 * 1024 - (size_t)ring;   // (ring < 0: no kernel for the key -- the launch below reports it)
  }
  while (spw > 1 && (((size_t)spw * ph * rp * PS + 1023) / 1024 * 1024) * act_planes > patch_budget) spw /= 2;
  a.tw_l = ilog2(tw); a.th_l = ilog2(th); a.spw_l = ilog2(spw);
  a.ph = ph; a.pw = pw; a.rp = rp; a.half = half;
  auto magic = [](int d) { return d < 2 ? 0u : (uint32_t)((0x100000000ull + d - 1) / d); };  // 0 encodes d == 1 (1x1 convs on 1x1 maps)
  a.pw_magic = magic(pw); a.ph_magic = magic(ph);
  a.patch_bytes = (int)((((size_t)spw * ph * rp * PS) + 1023) / 1024 * 1024);
  if (dma) {  // two unpadded, swizzled patch buffers; the row pitch keeps the rules above
    a.patch_bytes = (int)((((size_t)spw * ph * rp * pc.kc * 2) + 1023) / 1024 * 1024);
    a.rp_magic = magic(rp);
    a.zero = ctx->zero_page;
  }
  const int hw = hout * hout;
  a.gap = io.gap; a.gap_slots = gap_slots(hw); a.gap_l = hw >= 32 ? 5 : ilog2(hw);
  a.ntiles = ((n + spw - 1) / spw) * (hout / th) * (hout / tw);
  // persistent workgroups: at most MLT_WG_PER_CU (default 2) x 256 CUs per cout tile, each looping over tiles
  const int wg_cap = tuning().wg_cap;
  // only the weights-resident kernels (single weight step, single channel chunk) are persistent (mlt_kernels.hip PERSIST)
  const int gt = (nsplit == 4 && !lat) ? pc.gt_w2 : pc.gt;  // the hi+lo-weights tier has its own taps-per-step (mlt_conv_cfg)
  const bool persistent = (gt == pc.taps + (pc.has_sc ? 1 : 0) && pc.cin == pc.kc) || dma == 2;
  // ring-DMA: one 16-wave or two 8-wave workgroups per CU, counted over all cout tiles
  const int cap = dma == 2 ? wg_cap * ((pc.mt_dma >= 256 || pc.stride == 2) ? 1 : 2) / (pc.cout / pc.ct) : wg_cap;  // stride 2: LDS fits one
  const int grid_x = (persistent && a.ntiles > cap) ? cap : a.ntiles;
  char name[48];
  std::snprintf(name, sizeof name, "conv3x3_s%d_%dto%d_h%d%s", pc.stride, pc.cin, pc.cout, hout, pc.has_sc ? "+sc" : "");
  const double px = (double)n * hw;
  const double flops = 2.0 * px * pc.cout * pc.cin * (pc.taps + (pc.has_sc ? 1 : 0));
  const double in_bytes = (double)n * hin * hin * pc.cin * 2;
  const double bytes = in_bytes + px * pc.cout * 2 * ((io.y ? 1 : 0) + (io.y_sc ? 1 : 0) + (io.res ? 1 : 0)) + (double)pc.w.size() * 2;
  Launch L{ctx};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  char variant[96];
  std::snprintf(variant, sizeof variant, "%s%s%s%s%s", nsplit == 1 ? "single pass" : nsplit == 2 ? "exact" : nsplit == 4 ? "hi+lo weights" : nsplit == 6 ? "exact-lite" : "?",
                pc.taps == 1 ? ", centre tap" : lat ? ", latency tiles" : dma == 1 ? ", resident weights + LDS-DMA patches" : dma == 2 ? ", weight ring + LDS-DMA" : "",
                io.y_c16 ? ", y chunk-major" : "", io.ysc_c16 ? ", sc chunk-major" : "", io.gap ? ", GAP" : "");
  int rc = L.prof_begin(name, flops, bytes, e0, e1, variant);
  if (rc) return rc;
  plan_note(ctx, {{"x", io.x}, {"y", io.y}, {"y_sc", io.y_sc}, {"res", io.res}, {"gap", io.gap}},
            {{"x_lo", (long)io.x_lo}, {"y_lo", (long)io.y_lo}, {"res_lo", (long)io.res_lo}, {"ysc_lo", (long)io.ysc_lo}, {"relu", io.relu}, {"grid", grid_x}});
  LAUNCH_TRY(ctx, mlt_launch_conv(pc.cin, pc.cout, pc.stride, nsplit, pc.taps == 1 ? MLT_CONV_CENTRE : lat ? MLT_CONV_LATENCY : dma ? MLT_CONV_DMA : MLT_CONV_DEFAULT, a, grid_x, ctx->stream));
  if ((rc = L.prof_end(e1))) return rc;
  if (io.y && (rc = debug_dump(ctx, name, io.y, (size_t)px * pc.cout * 2))) return rc;
  if (io.y_sc && (rc = debug_dump(ctx, (std::string(name) + "_sc").c_str(), io.y_sc, (size_t)px * pc.cout * 2))) return rc;
  return MLT_OK;
}

// First layer: raw Pel planes -> t = relu(bn1(conv1(stem x))) and sc = bn(shortcut(stem x)) in one composed kernel.
int run_stem5(mlt_ctx *ctx, const mlt::PackedConv &pc, int n, int S, const Planes &pl, void *y, void *y_sc, size_t lo_off) {
  const int hout = S / 2;
  Stem5Args a{};
  pl.fill(a);
  a.w = pc.d_w; a.bias = pc.d_bias; a.bias_sc = pc.d_bias_sc; a.y = y; a.y_sc = y_sc;
  a.y_lo_off = lo_off; a.ysc_lo_off = lo_off; a.w_lo_off = pc.plane_halves * 2; a.acc_scale = pc.acc_scale;
  a.n = n; a.s_l = ilog2(S); a.hout_l = ilog2(hout);
  const int MT = 256;
  const int tw = hout < 32 ? hout : 32;
  const int th = MT / tw < hout ? MT / tw : hout;
  const int spw = MT / (tw * th);
  a.tw_l = ilog2(tw); a.th_l = ilog2(th); a.spw_l = ilog2(spw);
  a.rh = 2 * th + 3; a.rw = 2 * tw + 3; a.halfw = (a.rw + 1) / 2;
  a.rw_magic = (uint32_t)((0x100000000ull + a.rw - 1) / a.rw);
  a.rh_magic = (uint32_t)((0x100000000ull + a.rh - 1) / a.rh);
  const int lds = spw * a.rh * 2 * a.halfw * 4;
  const int grid_x = ((n + spw - 1) / spw) * (hout / th) * (hout / tw);
  char name[48];
  std::snprintf(name, sizeof name, "stem5x5_s2_2to32_h%d+sc", hout);
  const double px = (double)n * hout * hout;
  Launch L{ctx};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = L.prof_begin(name, 2.0 * px * 32 * (50 + 18), (double)n * S * S * 4 + px * 32 * 2 * 2, e0, e1, pc.xl ? "exact-lite" : pc.exact ? "exact" : pc.w2 ? "hi+lo weights" : "single pass");
  if (rc) return rc;
  plan_note(ctx, {{"y", y}, {"y_sc", y_sc}}, {{"lo", (long)lo_off}, {"grid", grid_x}});
  LAUNCH_TRY(ctx, mlt_launch_stem5(a, pc.exact ? 2 : pc.w2 ? 3 : 1, grid_x, lds, ctx->stream));
  if ((rc = L.prof_end(e1))) return rc;
  if ((rc = debug_dump(ctx, name, y, (size_t)px * 32 * 2))) return rc;
  return debug_dump(ctx, (std::string(name) + "_sc").c_str(), y_sc, (size_t)px * 32 * 2);
}

// Whole layer0.0 (composed first layer + conv2 + shortcut + relu) from the raw planes in one kernel (fast, H >= 32).
int run_stem_block(mlt_ctx *ctx, const mlt::Model &m, int n, int S, const Planes &pl, void *y, int32_t *d_flat, bool flat_is_clear) {
  const int h = S / 2;
  const mlt::PackedConv &c2 = m.blocks[0][0].conv2;
  StemBlockArgs a{};
  pl.fill(a);
  a.w = m.stem_b.d_w; a.w2 = c2.d_w; a.bias = m.stem.d_bias; a.bias_sc = m.stem.d_bias_sc; a.bias2 = c2.d_bias; a.y = y;
  a.flat = d_flat;
  a.w_lo_off = m.stem_b.plane_halves * 2; a.w2_lo_off = c2.plane_halves * 2; a.scale2 = c2.acc_scale;
  if (d_flat && !flat_is_clear) LAUNCH_TRY(ctx, hipMemsetAsync(d_flat, 0, (size_t)n * 4, ctx->stream));  // (flat_is_clear: the consumer of the previous call left it zero)
  a.acc_scale = m.stem.acc_scale; a.n = n; a.hout_l = ilog2(h); a.ntiles = n * (h / 16) * (h / 32);
  const int wg_cap = tuning().wg_cap2;  // one (pipelined) workgroup per CU
  const int grid_x = a.ntiles > wg_cap ? wg_cap : a.ntiles;
  char name[48];
  std::snprintf(name, sizeof name, "stem+block_s2_2to32_h%d(layer0.0)", h);
  const double px = (double)n * h * h;
  Launch L{ctx};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = L.prof_begin(name, 2.0 * px * 32 * (50 + 18 + 288), (double)n * S * S * 4 + px * 32 * 2, e0, e1, m.w2 ? "hi+lo weights" : "single pass");
  if (rc) return rc;
  plan_note(ctx, {{"y", y}, {"flat", d_flat}}, {{"flat_is_clear", flat_is_clear}, {"grid", grid_x}});
  LAUNCH_TRY(ctx, mlt_launch_stem_block(a, m.w2, grid_x, ctx->stream));
  if ((rc = L.prof_end(e1))) return rc;
  return debug_dump(ctx, name, y, (size_t)px * 32 * 2);
}

// All of layer0 of 128 x 128 CUs in one launch (layer0_stream_kernel): bit-identical to run_stem_block + run_block32, b0 never reaches HBM.
// c5 != nullptr: layer1.0.conv1 + shortcut ride along as a fifth stage (layer0_stream_kernel<true>): y is not written, t -> y_t (NHWC), sc -> y_sc (chunk-major)
// xs (with c5, when run_layer1_stream(..., c5) follows): layer0_stream_xs_kernel -- y_sc receives the shortcut's input [n][32][32][32] instead, half the bytes
int run_layer0_stream(mlt_ctx *ctx, const mlt::Model &m0, const mlt::Model &m1, int n, const Planes &pl, void *y, int32_t *d_flat, bool flat_is_clear,
                      const mlt::PackedConv *c5, void *y_t, void *y_sc, bool xs) {
  const mlt::PackedConv &c2 = m0.blocks[0][0].conv2;
  const mlt::Block &B1 = m1.blocks[0][1];
  Layer0Args a{};
  pl.fill(a);
  a.w = m0.stem_b.d_w; a.w2 = c2.d_w; a.w3 = B1.conv1.d_w; a.w4 = B1.conv2.d_w;
  a.bias = m0.stem.d_bias; a.bias_sc = m0.stem.d_bias_sc; a.bias2 = c2.d_bias; a.bias3 = B1.conv1.d_bias; a.bias4 = B1.conv2.d_bias;
  a.y = y; a.flat = d_flat; a.acc_scale = m0.stem.acc_scale; a.n = n;
  if (c5) { a.w5 = c5->d_w; a.bias5 = c5->d_bias; a.bias5_sc = c5->d_bias_sc; a.scale5 = c5->acc_scale; a.y_t = y_t; a.y_sc = y_sc; }
  if (d_flat && !flat_is_clear) LAUNCH_TRY(ctx, hipMemsetAsync(d_flat, 0, (size_t)n * 4, ctx->stream));
  const int wg_cap = tuning().wg_cap0;
  const int grid_x = n > wg_cap ? wg_cap : n;
  const double px = (double)n * 64 * 64;
  Launch L{ctx};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = c5 ? L.prof_begin("layer0_stream_h64(stem+layer0+layer1.0.conv1+sc)", 2.0 * px * 32 * (50 + 18 + 3 * 288) + 2.0 * (px / 4) * 64 * (288 + (xs ? 0 : 32)),
                             (double)n * 128 * 128 * 4 + (px / 4) * (64 + (xs ? 32 : 64)) * 2, e0, e1, xs ? "xs hand-off" : nullptr)
              : L.prof_begin("layer0_stream_h64(stem+layer0.0+layer0.1)", 2.0 * px * 32 * (50 + 18 + 3 * 288), (double)n * 128 * 128 * 4 + px * 32 * 2, e0, e1);
  if (rc) return rc;
  const bool mfma32 = tuning().l0_mfma32;   // round 5's MFMA shape (A/B; the results are the same bits)
  plan_note(ctx, {{"y", c5 ? nullptr : y}, {"y_t", c5 ? y_t : nullptr}, {"y_sc", c5 ? y_sc : nullptr}, {"flat", d_flat}}, {{"flat_is_clear", flat_is_clear}, {"grid", grid_x}});
  LAUNCH_TRY(ctx, mlt_launch_layer0_stream(a, c5 != nullptr, mfma32, xs, grid_x, ctx->stream));
  if ((rc = L.prof_end(e1))) return rc;
  if (c5) {
    if ((rc = debug_dump(ctx, "conv3x3_s2_32to64_h32+sc", y_t, (size_t)(px / 4) * 64 * 2))) return rc;
    return debug_dump(ctx, "conv3x3_s2_32to64_h32+sc_sc", y_sc, (size_t)(px / 4) * 64 * 2);
  }
  return debug_dump(ctx, "block_s1_32_h64(conv1+conv2)", y, (size_t)px * 32 * 2);  // (the dump carries the two-launch form's name: same tensor)
}

// Fused identity BasicBlock of the 32-channel stage (fast arithmetic, H >= 32): conv1 -> LDS -> conv2 + residual.
int run_block32(mlt_ctx *ctx, const mlt::Block &B, int n, int h, const void *x, void *y) {
  Block32Args a{};
  const bool w2 = B.conv1.w2;  // hi+lo weights: 8 x 32 tiles (four resident weight planes)
  a.x = x; a.y = y; a.w1 = B.conv1.d_w; a.w2 = B.conv2.d_w; a.bias1 = B.conv1.d_bias; a.bias2 = B.conv2.d_bias;
  a.w1_lo_off = B.conv1.plane_halves * 2; a.w2_lo_off = B.conv2.plane_halves * 2; a.scale1 = B.conv1.acc_scale; a.scale2 = B.conv2.acc_scale;
  a.n = n; a.h_l = ilog2(h); a.ntiles = n * (h / (w2 ? 8 : 16)) * (h / 32);
  const int wg_cap = tuning().wg_cap;
  const int grid_x = a.ntiles > wg_cap ? wg_cap : a.ntiles;
  char name[48];
  std::snprintf(name, sizeof name, "block_s1_32_h%d(conv1+conv2)", h);
  const double px = (double)n * h * h;
  Launch L{ctx};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = L.prof_begin(name, 2.0 * px * 32 * 32 * 9 * 2, px * 32 * 2 * 2 + 2.0 * 18 * 1024, e0, e1, w2 ? "hi+lo weights" : "single pass");
  if (rc) return rc;
  plan_note(ctx, {{"x", x}, {"y", y}}, {{"grid", grid_x}});
  LAUNCH_TRY(ctx, mlt_launch_block32(a, w2, grid_x, ctx->stream));
  if ((rc = L.prof_end(e1))) return rc;
  return debug_dump(ctx, name, y, (size_t)px * 32 * 2);
}

// BasicBlock tail of a stage as ONE launch (chain_kernel): b0 = relu(bn2(conv2 t) + sc); t1 = relu(bn1(conv1 b0));
// out = relu(bn2(conv2 t1) + b0) (+ GAP).  Fast arithmetic, stages whose whole sample fits the LDS (128 channels @ 16 x 16).
// s2_in != NULL: the stage's stride-2 conv + shortcut run inside the same launch from the stage input s2_in ([n][2h][2h][c/2]);
// t / sc are then unused.  wide (the whole 256-channel stage): stage256_wide_kernel, same launch name, same bits.
int run_chain3(mlt_ctx *ctx, const mlt::Block &B0, const mlt::Block &B1, int n, int h, const void *t, const void *sc, void *y, float *gap,
               const void *s2_in, bool x_c16, bool y_c16, void *b0_hbm, bool sc_c16, bool wide) {
  const int c = B0.conv2.cout;
  ChainArgs a{};
  a.x = s2_in ? s2_in : t; a.nconv = 3; a.y = y; a.gap = gap; a.n = n; a.zero = ctx->zero_page;
  a.x_c16 = x_c16 ? 1 : 0; a.y_c16 = y_c16 ? 1 : 0; a.res0_c16 = sc_c16 ? 1 : 0;
  const mlt::PackedConv *pcs[3] = {&B0.conv2, &B1.conv1, &B1.conv2};
  const bool w2 = B0.conv2.w2;  // hi+lo weights: chain_kernel<..., W2> (two planes per ring step)
  for (int k = 0; k < 3; ++k) {
    a.cv[k].w = pcs[k]->d_w; a.cv[k].bias = pcs[k]->d_bias; a.cv[k].acc_scale = pcs[k]->acc_scale; a.cv[k].relu = 1;
    a.cv[k].w_lo_off = pcs[k]->plane_halves * 2;
    a.cv[k].lo8_scale = 0x01010101 * ((127 - pcs[k]->lo8_exp) & 0xFF);  // E8M0 byte of the FP8 lo plane's scale (2^-lo8_exp), all four bytes
  }
  a.cv[0].res_mode = s2_in ? 2 : 1; a.cv[0].res = sc; a.cv[0].save = 1; a.cv[2].res_mode = 2;
  if (c == 64) {  // no room for b0 in registers: conv 0 writes it to HBM (b0_hbm), the last conv reads it back as its residual
    a.cv[0].save = 0; a.cv[0].y = b0_hbm; a.cv[2].res_mode = 1; a.cv[2].res = b0_hbm;
  }
  if (s2_in) {
    const mlt::PackedConv &p2 = B0.conv1_s2c;
    a.s2_w = p2.d_w; a.s2_bias = p2.d_bias; a.s2_bias_sc = p2.d_bias_sc; a.s2_scale = p2.acc_scale;
  }
  const int hw = h * h;
  a.gap_slots = gap_slots(hw); a.gap_l = hw >= 32 ? 5 : ilog2(hw);
  const int wg_cap = tuning().wg_cap;
  const int spw = c == 256 ? 2 : 1;            // samples per workgroup (64 KiB of activations)
  const int ntiles = (n + spw - 1) / spw;
  const int grid_x = ntiles > wg_cap ? wg_cap : ntiles;  // one workgroup per CU (its LDS is full), persistent over tiles
  char name[48];
  std::snprintf(name, sizeof name, s2_in ? "stage_%d_h%d(s2+sc,conv2,conv1,conv2)" : "chain3_s1_%d_h%d(conv2+conv1+conv2)", c, h);
  const double px = (double)n * hw;
  const double flops = 3.0 * 2.0 * px * c * c * 9 + (s2_in ? 2.0 * px * c * (c / 2) * 10 : 0.0);
  const double bytes = (s2_in ? px * 4 * (c / 2) * 2 : px * c * 2 * 2) + (y ? px * c * 2 : 0.0) + 3.0 * (double)B0.conv2.w.size() * 2 +
                       (s2_in ? (double)B0.conv1_s2c.w.size() * 2 : 0.0);
  Launch L{ctx};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  char variant[96];
  std::snprintf(variant, sizeof variant, "%s%s%s%s%s%s", wide ? "both cout passes per wave, " : "", w2 ? "hi+lo weights" : "single pass", x_c16 ? ", x chunk-major" : "", sc_c16 ? ", sc chunk-major" : "", y_c16 ? ", y chunk-major" : "",
                gap ? ", GAP" : "");
  int rc = L.prof_begin(name, flops, bytes, e0, e1, variant);
  if (rc) return rc;
  plan_note(ctx, {{"x", a.x}, {"sc", s2_in ? nullptr : sc}, {"y", y}, {"gap", gap}, {"b0", c == 64 ? b0_hbm : nullptr}}, {{"grid", grid_x}});
  if (wide) {  // (plan_network: the single-pass whole-stage launch of the 256 stage on a device that passed the LDS probe)
    LAUNCH_TRY(ctx, c == 256 && h == 8 && s2_in && !w2 && ctx->lds_oob_zero ? mlt_launch_stage256_wide(a, grid_x, ctx->stream) : hipErrorInvalidValue);
  } else {
    LAUNCH_TRY(ctx, mlt_launch_chain(c, h, s2_in != nullptr, ctx->lds_oob_zero, w2, a, grid_x, ctx->stream));
  }
  if ((rc = L.prof_end(e1))) return rc;
  if (y && (rc = debug_dump(ctx, name, y, (size_t)px * c * 2))) return rc;
  return MLT_OK;
}

// The three stride-1 convs of layer1 (64 channels at 32 x 32) as ONE streaming launch (layer1_stream_kernel): bit-identical to run_chain3's
// 64-channel chain, weights resident in registers, b0 never in HBM.  t NHWC, sc chunk-major (what layer0_stream_kernel<true> / the stride-2 launch write).
// c5xs != nullptr (behind run_layer0_stream(..., xs)): layer1_stream_xs_kernel -- `sc` holds the shortcut's input and the launch computes the shortcut from
// layer1.0.conv1's packed weights (tap 9), its shortcut biases and its accumulator scale
int run_layer1_stream(mlt_ctx *ctx, const mlt::Block &B0, const mlt::Block &B1, int n, const void *t, const void *sc, void *y, float *gap, bool y_c16, const mlt::PackedConv *c5xs) {
  Layer1Args a{};
  const bool xs = c5xs != nullptr;
  if (xs) { a.w_sc = c5xs->d_w; a.bias_sc = c5xs->d_bias_sc; a.scale_sc = c5xs->acc_scale; }
  a.t = t; a.sc = sc; a.y = y; a.y_c16 = y_c16 ? 1 : 0; a.gap = gap; a.gap_slots = gap_slots(32 * 32); a.n = n;
  const mlt::PackedConv *pcs[3] = {&B0.conv2, &B1.conv1, &B1.conv2};
  for (int k = 0; k < 3; ++k) { a.w[k] = pcs[k]->d_w; a.bias[k] = pcs[k]->d_bias; a.scale[k] = pcs[k]->acc_scale; }
  const int wg_cap = tuning().wg_cap1;
  const int grid_x = n > wg_cap ? wg_cap : n;
  const double px = (double)n * 32 * 32;
  Launch L{ctx};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = L.prof_begin("layer1_stream_h32(conv2+conv1+conv2)", 3.0 * 2.0 * px * 64 * 64 * 9 + (xs ? 2.0 * px * 64 * 32 : 0.0), px * (64 * 2 + (xs ? 32 : 64)) * 2 + 3.0 * 72 * 1024 + (xs ? 4096.0 : 0.0), e0, e1,
                        xs ? (y_c16 ? "xs hand-off, single pass, y chunk-major, GAP" : "xs hand-off, single pass, GAP") : y_c16 ? "single pass, y chunk-major, GAP" : "single pass, GAP");
  if (rc) return rc;
  // round 6: the 16x16x32 MFMA form exists (same bits) but measures 2 % SLOWER here than round 5's 32x32x16 form (0.882 against 0.863 ms, same box, alternating:
  // profiles/r06e_mfma16_ab.txt) -- the bare loop's +11 % is a clock effect at 1.6 GHz, this kernel already holds ~2.1 GHz and pays for twice the MFMA issue
  // slots and 8-byte epilogue accesses: it stays on 32x32x16 (MLT_TUNING=1 MLT_L1_MFMA16=1 selects the other form)
  const bool mfma32 = tuning().l1_mfma32;
  plan_note(ctx, {{"t", t}, {"sc", sc}, {"y", y}, {"gap", gap}}, {{"grid", grid_x}});
  LAUNCH_TRY(ctx, mlt_launch_layer1_stream(a, mfma32, xs, grid_x, ctx->stream));
  if ((rc = L.prof_end(e1))) return rc;
  return debug_dump(ctx, "chain3_s1_64_h32(conv2+conv1+conv2)", y, (size_t)px * 64 * 2);
}

// the batch class: everything about a CALL that the choice of launches depends on
enum : unsigned { CLS_QUADS = 1u, CLS_FLAT = 2u, CLS_L0_STREAM = 4u, CLS_L1_STREAM = 8u, CLS_CHAIN0 = 16u /* << s: stage s is large enough for a whole-stage launch */ };
unsigned batch_class(const NetCfg &c, int n, const Planes &pl, bool has_flat) {
  const Tuning &tn = tuning();
  unsigned cls = 0;
  if (pl.aligned8()) cls |= CLS_QUADS;
  if (has_flat) cls |= CLS_FLAT;
  // round 5: batches of 128 x 128 CUs run ALL of layer0 in one streaming launch; round 6: from 128 CUs on -- the measured crossover (docs/KERNEL_NOTES.md,
  // "Where the streaming launches start to pay": 128 CUs +3 %, 192 CUs +12 %); the same for layer1's three stride-1 convs
  if (tn.l0_stream_min > 0 && n >= tn.l0_stream_min) cls |= CLS_L0_STREAM;
  if (tn.l1_stream_min > 0 && n >= tn.l1_stream_min) cls |= CLS_L1_STREAM;
  for (int s = 1; s < c.m->n_stages; ++s) {   // small launches keep the per-conv latency variants: a chain runs its convs one after the other on n workgroups
    const int h = c.h_in(s), ho = h / 2 > 0 ? h / 2 : 1;
    if ((long)n * ho * ho > tn.lat_pixels) cls |= CLS_CHAIN0 << s;
  }
  return cls;
}


NetPlan plan_network(const mlt_ctx *ctx, const NetCfg &c, unsigned cls) {
  const Tuning &tn = tuning();
  const mlt::Model &m = *c.m;
  NetPlan P;
  auto add = [&](PlanStep::Kind k, int s) -> PlanStep & { PlanStep st{}; st.kind = k; st.s = (int8_t)s; P.push_back(st); return P.back(); };
  // Which stages run as chain / whole-stage launches (fast arithmetic, large launches).  Asked for stage s AND for stage s + 1: a stage whose successor
  // is a whole-stage kernel writes its output chunk-major (ConvArgs.y_c16).
  auto wants_chain = [&](int s) -> bool {
    if (s <= 0 || s >= m.n_stages || tn.no_chain || !(cls & (CLS_CHAIN0 << s))) return false;
    const mlt::Model &mm = c.model_of(s, 1);
    if (mm.exact || (mm.w2 && !ctx->lds_oob_zero)) return false;  // (the hi+lo-weights chains exist in the padding-from-beyond-the-LDS form only)
    const int h = c.h_in(s), ho = h / 2 > 0 ? h / 2 : 1;
    const mlt::PackedConv &c2 = mm.blocks[s][0].conv2;
    // The 64-channel chain (a 128 KiB sample per workgroup, 8 accumulators per wave; b0 through HBM): 1.19 ms against 3 x 0.40 ms
    // for the launch itself, but the step gains 4 % (less HBM traffic -> the power-limited chip clocks the other kernels higher).
    const bool packing_ok = (m.planes[s] == 64 ? (c2.ct == 64 && c2.gt == 9 && tn.chain64) : (c2.ct == 128 && c2.gt == 3)) && (!mm.w2 || c2.lo8 || m.planes[s] == 64);  // what chain_kernel<C> streams
    return mlt_chain_supported(m.planes[s], ho) && c2.taps == 9 && c2.kc == 64 && packing_ok;
  };
  // (the whole-stage form -- stride-2 conv + shortcut inside the launch -- exists for the single pass only: both units of the stage on `m`)
  auto wants_s2 = [&](int s) -> bool {
    if (!wants_chain(s) || tn.no_chain_s2 || c.model_of(s, 0).w2 || c.model_of(s, 1).w2) return false;
    const mlt::PackedConv &p2 = c.model_of(s, 0).blocks[s][0].conv1_s2c;
    return ctx->plan ? !p2.w.empty() : p2.d_w != nullptr;
  };
  bool cur_c16 = false;    // layout of the stage input
  bool l0_front = false;   // the layer0 streaming launch carried layer1.0.conv1 + shortcut
  int l0_front_step = -1;  // ... and its place in the plan
  for (int s = 0; s < m.n_stages; ++s) {
    const bool last = s == m.n_stages - 1;
    const mlt::Model &ms = c.model_of(s, 0);  // first launch unit: layer0.0 / the stride-2 conv + shortcut
    const mlt::Model &mt = c.model_of(s, 1);  // second unit: layer0.1, or conv2 of block 0 + block 1 of the later stages
    const int h = c.h_in(s), ho = h / 2 > 0 ? h / 2 : 1;
    const bool fused_b0 = s == 0 && !ms.exact && ho >= 32 && !tn.no_block_fusion && (cls & CLS_QUADS);
    if (s == 0 && (cls & CLS_FLAT) && !fused_b0) add(PlanStep::FLAT_STAT, 0);
    if (fused_b0 && ho == 64 && !ms.w2 && !mt.exact && !mt.w2 && (cls & CLS_L0_STREAM)) {
      // ... and with it the stride-2 conv + shortcut that open layer1, when the 64-channel chain follows (it wants sc chunk-major) and layer1's first
      // unit runs the single pass too: layer0's output then never reaches HBM
      const mlt::Model &m10 = c.model_of(1, 0);
      const mlt::PackedConv &c5 = m10.blocks[1][0].conv1;
      l0_front = !tn.no_l0_s5 && m.n_stages > 1 && !m10.exact && !m10.w2 && wants_chain(1) && !wants_s2(1) && m.planes[1] == 64 && !tn.no_c16 &&
                 c5.has_sc && c5.taps == 9 && c5.kc == 32 && c5.ct == 64 && c5.cin == 32 && c5.cout == 64 && c5.stride == 2;
      add(PlanStep::LAYER0_STREAM, 0).front = l0_front;
      if (l0_front) l0_front_step = (int)P.size() - 1;
      continue;
    }
    if (fused_b0) add(PlanStep::STEM_BLOCK, 0);   // raw planes -> b0 in ONE kernel (t and sc never leave the chip)
    else {
      const bool chain = wants_chain(s), chain_s2 = wants_s2(s);   // chain_s2: the stride-2 conv + shortcut join the launch
      bool sc_c16 = false;
      if (s == 0) add(PlanStep::STEM5, 0);
      else if (chain_s2) {}
      else if (s == 1 && l0_front) sc_c16 = true;   // layer0_stream_kernel<true> wrote t (pool0) and sc (pool1, chunk-major) already
      else {
        // the 64-channel chain reads sc as a residual in accumulator order: chunk-major makes that one cache line per lane quad
        // (t -- the chain's input, fetched by LDS-DMA -- stays NHWC: chunk-major, the stride-2 kernel's stores gained what the chain's
        // DMA lost, 0.455 -> 0.438 ms against 1.06 -> 1.08 ms)
        sc_c16 = chain && m.planes[s] == 64 && !tn.no_c16 && !ms.exact;  // (the exact kernels write NHWC)
        add(PlanStep::CONV_S2, s).sc_c16 = sc_c16;
      }
      if (chain) {  // rest of the stage (or all of it) in one launch: activations stay in LDS, b0 in registers
        const bool out_c16 = !last && !tn.no_c16 && wants_s2(s + 1);
        // round 5: large batches run the 64-channel stage's three stride-1 convs as a streaming launch (same bits as the chain)
        const mlt::PackedConv &q2 = mt.blocks[s][0].conv2;
        const bool stream = s == 1 && !chain_s2 && m.planes[s] == 64 && ho == 32 && sc_c16 && !mt.w2 && !mt.exact && (cls & CLS_L1_STREAM) &&
                            q2.taps == 9 && q2.kc == 64 && q2.ct == 64 && !last;
        PlanStep &st = add(stream ? PlanStep::LAYER1_STREAM : PlanStep::CHAIN, s);
        st.inside_s2 = chain_s2; st.x_c16 = cur_c16; st.sc_c16 = sc_c16; st.y_c16 = out_c16;
        // the whole 256-channel stage: both cout passes per wave (padding from beyond the LDS only: devices that fail the probe keep chain_kernel)
        st.wide = chain_s2 && m.planes[s] == 256 && ho == 8 && ctx->lds_oob_zero && !tn.no_stage256_wide;
        // the five-stage front followed by layer1's streaming launch, both in their shipped MFMA shapes: the front hands over the shortcut's INPUT (half
        // the bytes) and layer1's loader waves compute the shortcut (layer0_stream_xs_kernel -> layer1_stream_xs_kernel; same bits).  Every other
        // consumer of the front's sc -- the 64-channel chain -- and every other producer of layer1's sc -- the stride-2 launch -- keeps the sc hand-off.
        if (stream && l0_front && l0_front_step >= 0 && !tn.no_xs_handoff && !tn.l0_mfma32 && tn.l1_mfma32) st.xs = P[(size_t)l0_front_step].xs = true;
        cur_c16 = out_c16;
        continue;
      }
      add(PlanStep::CONV_B0C2, s);   // b0 = relu(bn2(conv2 t) + sc)
    }
    // block 1 (identity shortcut)
    if (s == 0 && !mt.exact && ho >= 32 && !tn.no_block_fusion) { add(PlanStep::BLOCK32, 0); continue; }  // 32-channel identity block in ONE kernel
    add(PlanStep::CONV_B1C1, s);
    PlanStep &st = add(PlanStep::CONV_B1C2, s);
    st.y_c16 = !last && !tn.no_c16 && wants_s2(s + 1);
    cur_c16 = st.y_c16;
  }
  add(PlanStep::HEADS, m.n_stages - 1);
  return P;
}

}  // namespace

// One pass of the network for n CUs in the arithmetic of `c` (NetCfg, mlt_runtime.h: the launch units of back_mask run `mback` -- the hi+lo-weights model; same
// single fp16 activation planes, so the two models' units compose freely -- those of x_units run `mx`, the EXACT arithmetic's per-conv kernels with a lo plane behind
// every tensor such a unit writes; a unit that reads a single-plane producer's output takes its lo part as zero; every other unit runs `m`).
// `go`: what the pass produces for the guards besides its results.
int run_network(mlt_ctx *ctx, SizeState &st, const NetCfg &c, int n, const PassIO &io, const GuardOut &go) {
  const int S = st.size;
  mlt::Model &m = *c.m;
  const unsigned cls = batch_class(c, n, io.pl, go.d_flat != nullptr);
  // the plan: cached per (models, unit masks, batch class) once the size is loaded -- while a load is in flight (the calibration prices candidate tiers and
  // rebuilds models in place) it is built per call
  NetPlan fresh;
  const NetPlan *plan;
  if (st.loaded && !ctx->plan) {
    const PlanKey key{c.m, c.mback, c.mx, c.back_mask, c.x_units, cls};
    auto it = st.plans.find(key);
    if (it == st.plans.end()) it = st.plans.emplace(key, plan_network(ctx, c, cls)).first;
    plan = &it->second;
  } else {
    fresh = plan_network(ctx, c, cls);
    plan = &fresh;
  }
  int rc = ctx->plan ? MLT_OK : ensure_ws(ctx, ws_per_cu(m, S, c.x_units != 0) * (size_t)n);   // (plan mode: the workspace is carved from a fake base and never touched)
  if (rc) return rc;
  // carve the workspace
  char *p = ctx->ws;
  auto carve = [&](size_t bytes) { char *r = p; p += (bytes + 255) / 256 * 256; return (void *)r; };
  const int h0 = S / 2 > 0 ? S / 2 : 1;
  // a lo plane behind every activation (x_units: room for one behind every buffer, used by the units of the mask only)
  const int nplanes = (m.exact || c.x_units) ? 2 : 1;
  void *pool[4];
  for (int i = 0; i < 4; ++i) pool[i] = carve((size_t)n * h0 * h0 * 32 * 2 * nplanes);
  void *outs[5];
  float *gaps[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  {
    int h = S;
    for (int s = 0; s < m.n_stages; ++s) {
      h = h / 2 > 0 ? h / 2 : 1;
      outs[s] = carve((size_t)n * h * h * m.planes[s] * 2 * nplanes);
      if (s >= 1) gaps[s] = (float *)carve((size_t)n * gap_slots(h * h) * m.planes[s] * 4);
    }
  }
  Launch L{ctx};
  const bool quad_ok = (cls & CLS_QUADS) != 0;
  for (const PlanStep &ps : *plan) {
    const int s = ps.s;
    const bool last = s == m.n_stages - 1;
    mlt::Model &ms = c.model_of(s, 0), &mt = c.model_of(s, 1);
    const int h = c.h_in(s), ho = h / 2 > 0 ? h / 2 : 1;
    const void *cur = s > 0 ? outs[s - 1] : nullptr;   // the stage input
    // (exact units, round 4: a unit in the exact arithmetic keeps a lo plane behind the tensors it writes and expects one behind those it
    // reads -- a plane of zeros when the producer is a single-plane unit; single-plane units read the hi planes and ignore the offsets)
    const bool ex0 = ms.exact, ex1 = mt.exact;
    const size_t lo_in = ex0 ? (size_t)n * h * h * (s == 0 ? 32 : m.planes[s - 1]) * 2 : 0;  // plane bytes of the stage input
    const size_t lo_st = (ex0 || ex1) ? (size_t)n * ho * ho * m.planes[s] * 2 : 0;             // plane bytes inside the stage
    // an exact unit behind a single-plane unit: its input has no lo part (the producer wrote fp16 values): lo offset 0 = "no lo plane, read
    // zeros" (ConvArgs.x_lo_off / res_lo_off)
    const bool in_has_lo = s > 0 && c.model_of(s - 1, 1).exact;
    const bool b0_has_lo = s == 0 ? ex0 : ex1;  // (b0 = pool2 is written by unit 0 of layer0, by unit 1 of the later stages)
    int hh = 0;
    ConvIO cv;
    switch (ps.kind) {
    case PlanStep::FLAT_STAT: {
      FlatStatArgs fa{};
      io.pl.fill(fa);
      fa.flat = go.d_flat; fa.n = n; fa.s_l = ilog2(S);
      hipEvent_t e0 = nullptr, e1 = nullptr;
      if ((rc = L.prof_begin("guard_flat_stat", 0.0, (double)n * S * S * 4, e0, e1))) return rc;
      plan_note(ctx, {{"flat", go.d_flat}}, {{"quads", quad_ok}});
      LAUNCH_TRY(ctx, mlt_launch_flat_stat(fa, quad_ok, ctx->stream));
      rc = L.prof_end(e1);
      break;
    }
    case PlanStep::LAYER0_STREAM:
      rc = run_layer0_stream(ctx, ms, mt, n, io.pl, outs[0], go.d_flat, go.flat_is_clear,
                             ps.front ? &c.model_of(1, 0).blocks[1][0].conv1 : nullptr, pool[0], pool[1], ps.front && ps.xs);
      break;
    case PlanStep::STEM_BLOCK:
      rc = run_stem_block(ctx, ms, n, S, io.pl, pool[2], go.d_flat, go.flat_is_clear);
      break;
    case PlanStep::STEM5:
      // block 0 (stride 2): ONE kernel gives t = relu(bn1(conv1 x)) and sc = bn(conv1x1 x) (arch:44-55); for s == 0 the same kernel also
      // computes x = stem(raw planes) on the fly (arch:277-278, EncCu.cpp:810-877)
      rc = run_stem5(ctx, ms.stem, n, S, io.pl, pool[0], pool[1], lo_st);
      break;
    case PlanStep::CONV_S2:
      cv.x = cur; cv.y = pool[0]; cv.y_sc = pool[1]; cv.relu = true;
      cv.x_lo = in_has_lo ? lo_in : 0; cv.y_lo = lo_st; cv.ysc_lo = lo_st;
      cv.ysc_c16 = ps.sc_c16;
      rc = run_conv(ctx, ms.blocks[s][0].conv1, n, h, cv, &hh);
      break;
    case PlanStep::CHAIN:
      rc = run_chain3(ctx, mt.blocks[s][0], mt.blocks[s][1], n, ho, pool[0], pool[1], last ? nullptr : outs[s], gaps[s], ps.inside_s2 ? cur : nullptr,
                      ps.x_c16, ps.y_c16, pool[2], ps.sc_c16, ps.wide);
      break;
    case PlanStep::LAYER1_STREAM:
      rc = run_layer1_stream(ctx, mt.blocks[s][0], mt.blocks[s][1], n, pool[0], pool[1], outs[s], gaps[s], ps.y_c16, ps.xs ? &c.model_of(1, 0).blocks[1][0].conv1 : nullptr);
      break;
    case PlanStep::CONV_B0C2:
      cv.x = pool[0]; cv.y = pool[2]; cv.res = pool[1]; cv.relu = true;  // b0 = relu(bn2(conv2 t) + sc)
      cv.x_lo = cv.y_lo = cv.res_lo = lo_st;
      if (s > 0 && ex1 && !ex0) cv.x_lo = cv.res_lo = 0;  // t and sc came from a single-plane unit
      rc = run_conv(ctx, (s == 0 ? ms : mt).blocks[s][0].conv2, n, ho, cv, &hh);
      break;
    case PlanStep::BLOCK32:
      rc = run_block32(ctx, mt.blocks[0][1], n, ho, pool[2], outs[0]);
      break;
    case PlanStep::CONV_B1C1:
      cv.x = pool[2]; cv.y = pool[3]; cv.relu = true;
      cv.x_lo = cv.y_lo = lo_st;
      if (!b0_has_lo) cv.x_lo = 0;
      rc = run_conv(ctx, mt.blocks[s][1].conv1, n, ho, cv, &hh);
      break;
    case PlanStep::CONV_B1C2:
      cv.x = pool[3]; cv.y = last ? nullptr : outs[s]; cv.res = pool[2]; cv.relu = true; cv.gap = gaps[s];
      cv.x_lo = cv.y_lo = cv.res_lo = lo_st;
      if (!b0_has_lo) cv.res_lo = 0;
      cv.y_c16 = ps.y_c16;
      rc = run_conv(ctx, mt.blocks[s][1].conv2, n, ho, cv, &hh);
      break;
    case PlanStep::HEADS: {
      HeadArgs ha{};
      for (int t = 1; t < m.n_stages; ++t) {   // head t - 1 pools stage t's output
        const int hd = t - 1, hs = c.h_in(t + 1);
        ha.gap[hd] = gaps[t]; ha.slots[hd] = gap_slots(hs * hs); ha.w[hd] = m.heads[hd].d_w; ha.b[hd] = m.heads[hd].d_b;
        ha.c[hd] = m.planes[t]; ha.hw[hd] = hs * hs; ha.classes[hd] = m.heads[hd].classes;
      }
      ha.n_heads = m.n_heads; ha.decision_head = st.head_index; ha.poc = io.poc; ha.qp = io.qp; ha.logits = io.logits; ha.split = io.split;
      ha.mag = go.d_mag;
      ha.dec = io.dec; ha.min_conf = st.min_conf;
      ha.cand = io.cand; ha.cand_cov = st.cand_cov; ha.cand_max = st.cand_max;
      const GuardTail *tail = go.tail;
      if (tail && (n == 1 || tail->next)) {
        ha.rule = tail->rule;
        ha.g_count = tail->count; ha.g_idx = tail->idx; ha.g_flat = tail->flat;
        ha.g_next = tail->next;   // (NULL: mlt_predict's slot -- one CU, the count is set outright)
      }
      hipEvent_t e0 = nullptr, e1 = nullptr;
      if (io.sweep.n_qps > 0) {   // QP sweep: the same arguments, the heads under every point (fix-up mode: io.sweep.idx)
        HeadSweepArgs sa{};
        sa.h = ha; sa.h.mag = nullptr;   // (ha.qp: NULL, or the CUs' offsets to every point)
        sa.n_qps = io.sweep.n_qps; sa.slab = io.sweep.slab; sa.fix_idx = io.sweep.idx; sa.mask = io.sweep.mask; sa.active = io.sweep.idx ? nullptr : io.sweep.active;
        std::memcpy(sa.qps, io.sweep.qps, sizeof sa.qps);
        if ((rc = L.prof_begin("heads_sweep", 0.0, 0.0, e0, e1))) return rc;
        LAUNCH_TRY(ctx, mlt_launch_heads_sweep(sa, n, ctx->stream));
        rc = L.prof_end(e1);
        break;
      }
      if ((rc = L.prof_begin("heads", 0.0, 0.0, e0, e1))) return rc;
      plan_note(ctx, {{"gap0", ha.gap[0]}, {"gap1", ha.gap[1]}, {"gap2", ha.gap[2]}, {"gap3", ha.gap[3]}},
                {{"slots0", ha.slots[0]}, {"slots1", ha.slots[1]}, {"slots2", ha.slots[2]}, {"slots3", ha.slots[3]}, {"c0", ha.c[0]}, {"c1", ha.c[1]}, {"c2", ha.c[2]}, {"c3", ha.c[3]},
                 {"hw0", ha.hw[0]}, {"hw1", ha.hw[1]}, {"hw2", ha.hw[2]}, {"hw3", ha.hw[3]}, {"heads", ha.n_heads}});
      LAUNCH_TRY(ctx, mlt_launch_heads(ha, n, ctx->stream));
      rc = L.prof_end(e1);
      break;
    }
    }
    if (rc) return rc;
  }
  return MLT_OK;
}

extern "C" {
#pragma GCC visibility push(default)

// Host-only hook (not part of include/mltcnn.h; no HIP call, no device): the LAUNCH PLAN of one batch -- what run_network would enqueue for n CUs of `size`
// with hi+lo weights in the launch units of w2_units and the exact arithmetic in those of x_units (tier: 0 the fp16 tiers as given by the two masks, 1 exact
// everywhere, 5 exact-lite everywhere), planes 8-byte aligned or not.  The models are built from the blob on the host exactly as mlt_load_weights builds them;
// the dispatcher then runs in plan mode (mlt_ctx::plan).  One launch per line: "name [variant, layouts]".  Returns the number of launches, or -1.
int mlt_plan_describe(const void *blob, size_t bytes, int size, int n, int tier, unsigned w2_units, unsigned x_units, int aligned, char *out, size_t cap) {
  const int si = size_index(size);
  if (!blob || !out || cap == 0 || si < 0 || n <= 0) return -1;
  mlt_ctx ctx;
  std::vector<std::string> plan;
  ctx.plan = &plan;
  ctx.plan_detail = (aligned & 2) != 0;   // (bit 1 of `aligned`: every record also lists the launch's buffers -- the hand-offs between launches)
  ctx.lds_oob_zero = true;    // (what every gfx950 device reports: mlt_probe_lds_oob)
  SizeState &st = ctx.sz[si];
  st.size = size; st.enabled = st.loaded = true;
  st.head_index = size == 128 ? 2 : 0;
  std::string err;
  const bool whole_exact = tier == 1 || tier == 5;
  if (!mlt::build_model(blob, bytes, tier == 5 ? mlt::MLT_MODEL_XLITE : tier == 1 ? mlt::MLT_MODEL_EXACT : mlt::MLT_MODEL_FAST, size, st.model, err)) return -1;
  if (!whole_exact && w2_units && !mlt::build_model(blob, bytes, mlt::MLT_MODEL_W2, size, st.model_w2, err)) return -1;
  if (!whole_exact && x_units && !mlt::build_model(blob, bytes, mlt::MLT_MODEL_EXACT, size, st.model_exact, err)) return -1;
  st.exact = whole_exact;
  st.w2 = !whole_exact && w2_units != 0; st.w2_units = st.w2 ? w2_units : 0; st.x_units = whole_exact ? 0 : x_units;
  const int16_t *planes = (const int16_t *)(uintptr_t)((aligned & 1) ? 0x1000 : 0x1002);   // never dereferenced: only the alignment is looked at
  int32_t *const flat_fake = (int32_t *)(uintptr_t)0x2000;   // (never dereferenced in plan mode; a constant so that the detailed records are reproducible)
  ctx.ws = (char *)(uintptr_t)0x100000000ull;   // (never touched in plan mode: a base that tells a workspace offset from a NULL pointer in the detailed records)
  GuardOut go;
  go.d_flat = whole_exact ? nullptr : flat_fake;
  const int rc = run_network(&ctx, st, st.main_cfg(), n, PassIO{Planes::dense(planes, planes, size), nullptr, nullptr, nullptr, nullptr, nullptr}, go);
  ctx.ws = nullptr;
  if (rc) return -1;
  size_t pos = 0;
  for (const std::string &l : plan) {
    if (pos + l.size() + 2 > cap) return -1;
    std::memcpy(out + pos, l.data(), l.size());
    pos += l.size();
    out[pos++] = '\n';
  }
  out[pos] = 0;
  return (int)plan.size();
}

#pragma GCC visibility pop
}  // extern "C"
