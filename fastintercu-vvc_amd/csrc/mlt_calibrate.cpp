// mlt_calibrate.cpp -- loading a size's weights: model upload, the calibration sets and session that price candidate tiers on the device (the search itself is
// mlt_tier_search.h), load_one / load_all, and the entry points around them (mlt_load_weights, mlt_calibrate, mlt_arithmetic).
#include "mlt_runtime.h"

namespace {

int upload_model(mlt_ctx *ctx, mlt::Model &m) {
  auto up = [&](mlt::PackedConv &pc) -> int {
    if (pc.w.empty()) return MLT_OK;  // layer0.0.conv1: folded into the composed first layer
    HIP_TRY(ctx, hipMalloc(&pc.d_w, pc.w.size() * 2));
    HIP_TRY(ctx, hipMemcpy(pc.d_w, pc.w.data(), pc.w.size() * 2, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMalloc((void **)&pc.d_bias, pc.bias.size() * 4));
    HIP_TRY(ctx, hipMemcpy(pc.d_bias, pc.bias.data(), pc.bias.size() * 4, hipMemcpyHostToDevice));
    if (pc.has_sc) {
      HIP_TRY(ctx, hipMalloc((void **)&pc.d_bias_sc, pc.bias_sc.size() * 4));
      HIP_TRY(ctx, hipMemcpy(pc.d_bias_sc, pc.bias_sc.data(), pc.bias_sc.size() * 4, hipMemcpyHostToDevice));
    }
    return MLT_OK;
  };
  int rc;
  if ((rc = up(m.stem))) return rc;
  if ((rc = up(m.stem_b))) return rc;
  for (int s = 0; s < m.n_stages; ++s)
    for (int b = 0; b < 2; ++b) {
      if ((rc = up(m.blocks[s][b].conv1))) return rc;
      if ((rc = up(m.blocks[s][b].conv2))) return rc;
      if ((rc = up(m.blocks[s][b].conv1_s2c))) return rc;
    }
  for (int h = 0; h < m.n_heads; ++h) {
    mlt::Head &H = m.heads[h];
    HIP_TRY(ctx, hipMalloc((void **)&H.d_w, H.w.size() * 4));
    HIP_TRY(ctx, hipMemcpy(H.d_w, H.w.data(), H.w.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMalloc((void **)&H.d_b, H.b.size() * 4));
    HIP_TRY(ctx, hipMemcpy(H.d_b, H.b.data(), H.b.size() * 4, hipMemcpyHostToDevice));
  }
  m.on_device = true;
  return MLT_OK;
}

}  // namespace

void free_model(mlt::Model &m) {
  auto fr = [](mlt::PackedConv &pc) {
    if (pc.d_w) (void)hipFree(pc.d_w);
    if (pc.d_bias) (void)hipFree(pc.d_bias);
    if (pc.d_bias_sc) (void)hipFree(pc.d_bias_sc);
    pc.d_w = nullptr; pc.d_bias = pc.d_bias_sc = nullptr;
  };
  fr(m.stem);
  fr(m.stem_b);
  for (int s = 0; s < 5; ++s)
    for (int b = 0; b < 2; ++b) { fr(m.blocks[s][b].conv1); fr(m.blocks[s][b].conv2); fr(m.blocks[s][b].conv1_s2c); }
  for (int h = 0; h < 4; ++h) { if (m.heads[h].d_w) (void)hipFree(m.heads[h].d_w); if (m.heads[h].d_b) (void)hipFree(m.heads[h].d_b); m.heads[h].d_w = m.heads[h].d_b = nullptr; }
  m.on_device = false;
}

namespace {

// ---- load-time calibration of the fast arithmetic against the exact one (include/mltcnn.h: mlt_load_weights) ----
// Calibration set (round 3): NOT only the bench's texture distribution.  Seeded CUs in five content classes -- the classes the
// flat-content guard does NOT re-evaluate exactly, because admission must be decided on what the fast arithmetic will really see:
//   0 texture (blocky base + texture +-48, pred = org + noise +-40)      1 i.i.d. uniform org and pred (large residuals)
//   2 constant org / textured pred    3 textured org / constant pred   4 texture with a constant band over 10-12 % of the
//   quads, just under the guard's 1/8 for exactly flat quads   5 (round 4) texture with a NEAR-flat band (+-1 LSB dither or amplitude-4
//   texture on constants, alternating) over 40-48 % of the rows, just under the guard's 1/2 for near-flat quads
// (content the guard catches -- constant, dithered, low-contrast, ramps -- is evaluated with the exact arithmetic anyway).
// Round 4: 560 CUs (160 + 5 x 80; round 3: 96) = 5040 logits of the 128 model, so that the LARGEST error seen is a statistic with some power:
// a Gaussian sample of that size peaks at 3.9 sigma, the round-3 tail probe found weight sets whose worst error sits at 6.5 x their rms.
constexpr int kCalibClasses = 6;          // synthetic content classes; class kCalibClasses = the caller's own CUs (mlt_calibrate)
constexpr int kCalibCount[kCalibClasses] = {160, 80, 80, 80, 80, 80};
constexpr int kCalibN = 560;
constexpr int kCalibCallerMax = 4096;     // caller-supplied CUs per mlt_calibrate call (64 KiB of planes each at S = 128)

struct CalibInputs { std::vector<int16_t> org, pred; std::vector<int32_t> poc, qp; std::vector<int> cls; };

// (generated once per process and CU size: 31 MB of planes for S = 128, ~0.1 s of host time)
const CalibInputs &calibration_set(int S) {
  static std::mutex mu;
  static std::map<int, CalibInputs> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(S);
  if (it != cache.end()) return it->second;
  CalibInputs &ci = cache[S];
  const size_t cs = (size_t)S * S;
  ci.org.assign(cs * kCalibN, 0); ci.pred.assign(cs * kCalibN, 0); ci.poc.assign(kCalibN, 0); ci.qp.assign(kCalibN, 0); ci.cls.assign(kCalibN, 0);
  uint64_t z = 0x9E3779B97F4A7C15ull;  // splitmix64
  auto next = [&]() { z += 0x9E3779B97F4A7C15ull; uint64_t x = z; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); };
  auto clip = [](int v) { return v < 0 ? 0 : v > 1023 ? 1023 : v; };
  const int nb = S / 16 > 0 ? S / 16 : 1, bs = S / nb;
  int i = 0;
  for (int c = 0; c < kCalibClasses; ++c)
    for (int k = 0; k < kCalibCount[c]; ++k, ++i) {
      ci.cls[i] = c;
      int16_t *o = &ci.org[(size_t)i * cs], *q = &ci.pred[(size_t)i * cs];
      std::vector<int> base((size_t)nb * nb);
      for (int &b : base) b = 64 + (int)(next() % 896);
      const int co = (int)(next() % 1024), cp = (int)(next() % 1024);
      int band_h = (S * (10 + k % 3)) / 100;
      if (band_h * 8 >= S) band_h = S / 8 - 1;
      if (band_h < 1) band_h = 1;
      if (c == 5) band_h = (S * (40 + 4 * (k % 3))) / 100;
      const int band_y = (int)(next() % (uint64_t)(S - band_h + 1));
      const int amp = (k & 1) ? 4 : 1;  // class 5: low contrast / dither
      for (int y = 0; y < S; ++y)
        for (int x = 0; x < S; ++x) {
          int vo, vp;
          if (c == 1) { vo = (int)(next() % 1024); vp = (int)(next() % 1024); }
          else {
            vo = clip(base[(size_t)(y / bs) * nb + x / bs] + (int)(next() % 97) - 48);
            vp = clip(vo + (int)(next() % 81) - 40);
            if (c == 2) vo = co;
            if (c == 3) vp = cp;
            if (c == 4 && y >= band_y && y < band_y + band_h) { vo = co; vp = cp; }
            if (c == 5 && y >= band_y && y < band_y + band_h) {
              vo = clip(8 + co % 1008 + (int)(next() % (uint64_t)(2 * amp + 1)) - amp);
              vp = clip(8 + cp % 1008 + (int)(next() % (uint64_t)(2 * amp + 1)) - amp);
            }
          }
          o[(size_t)y * S + x] = (int16_t)vo;
          q[(size_t)y * S + x] = (int16_t)vp;
        }
      ci.poc[i] = (int32_t)(next() % 601);
      ci.qp[i] = 17 + (int32_t)(next() % 31);
    }
  return ci;
}

// Round 6: the IN-DISTRIBUTION set behind the magnitude guard.  A configuration admitted behind that guard runs only CUs of ordinary logit
// magnitude in the non-exact arithmetic -- for a trained-like weight set that leaves ~200 of the 560 synthetic CUs (the texture class and parts of
// the band classes), too few for the statistical admission rule, and none of them has the statistics of natural scenes, the content on which
// such a set's WEIGHT rounding error is largest (smooth activations: the error of a weight is the same at every pixel and survives the pooling;
// tools/attribute_error.py).  So the guarded figures are taken over the synthetic CUs below the threshold PLUS this set: 160 further CUs of the
// texture class (class 0) and 160 "1/f scenes" (class kClassScenes): a random-phase field of 48 plane waves with log-uniform spatial frequency
// (equal power per octave = the 1/f^2 power law of natural images: fastintercu-vvc_amd/synth.py natural_patches, without the FFT), contrast
// log-uniform 6 ... 160 ten-bit steps around a mean of 120 ... 900, +-1 step of sensor noise; prediction = the scene displaced by a motion vector
// in [-2, 2]^2, smoothed by [1 2 1]^2 / 16 with probability 1/2, + noise of amplitude 0 ... 6.  Only priced for configurations the plain rule
// rejects; generated once per process (~0.2 s).
constexpr float kMagRange = 1.5f;   // range guard: a plain-admitted tier is trusted up to this multiple of the largest logit magnitude of its calibration CUs
constexpr int kClassScenes = kCalibClasses + 1;   // content class ids: 0 .. 5 synthetic, kCalibClasses = the caller's, kClassScenes = the 1/f scenes
constexpr int kCalibExtraTexture = 160, kCalibExtraScenes = 160, kCalibExtraN = kCalibExtraTexture + kCalibExtraScenes;

const CalibInputs &calibration_extra_set(int S) {
  static std::mutex mu;
  static std::map<int, CalibInputs> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(S);
  if (it != cache.end()) return it->second;
  CalibInputs &ci = cache[S];
  const size_t cs = (size_t)S * S;
  ci.org.assign(cs * kCalibExtraN, 0); ci.pred.assign(cs * kCalibExtraN, 0); ci.poc.assign(kCalibExtraN, 0); ci.qp.assign(kCalibExtraN, 0); ci.cls.assign(kCalibExtraN, 0);
  uint64_t z = 0xD1B54A32D192ED03ull;  // splitmix64, another stream than calibration_set's
  auto next = [&]() { z += 0x9E3779B97F4A7C15ull; uint64_t x = z; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); };
  auto unif = [&]() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); };
  auto clip = [](int v) { return v < 0 ? 0 : v > 1023 ? 1023 : v; };
  const int nb = S / 16 > 0 ? S / 16 : 1, bs = S / nb;
  for (int i = 0; i < kCalibExtraTexture; ++i) {   // the texture class of calibration_set (class 0)
    int16_t *o = &ci.org[(size_t)i * cs], *q = &ci.pred[(size_t)i * cs];
    std::vector<int> base((size_t)nb * nb);
    for (int &b : base) b = 64 + (int)(next() % 896);
    for (int y = 0; y < S; ++y)
      for (int x = 0; x < S; ++x) {
        const int vo = clip(base[(size_t)(y / bs) * nb + x / bs] + (int)(next() % 97) - 48);
        o[(size_t)y * S + x] = (int16_t)vo;
        q[(size_t)y * S + x] = (int16_t)clip(vo + (int)(next() % 81) - 40);
      }
    ci.poc[i] = (int32_t)(next() % 601);
    ci.qp[i] = 17 + (int32_t)(next() % 31);
  }
  const int m = S + 8, K = 48;
  std::vector<float> field((size_t)m * m);
  std::vector<int> scene((size_t)m * m), ref((size_t)m * m);
  for (int i = kCalibExtraTexture; i < kCalibExtraN; ++i) {
    ci.cls[i] = kClassScenes;
    std::fill(field.begin(), field.end(), 0.f);
    for (int k = 0; k < K; ++k) {
      const double f = std::exp(std::log(1.0 / m) + unif() * (std::log(0.5) - std::log(1.0 / m)));   // cycles per pixel, log-uniform in [1 / m, 1 / 2]
      const double th = unif() * 6.283185307179586, ph = unif() * 6.283185307179586;
      const double wx = 6.283185307179586 * f * std::cos(th), wy = 6.283185307179586 * f * std::sin(th);
      const double cb = std::cos(wx), sb = std::sin(wx);
      for (int y = 0; y < m; ++y) {   // cos(ph + wy y + wx x) along x by rotation
        double c = std::cos(ph + wy * y), sn = std::sin(ph + wy * y);
        float *row = &field[(size_t)y * m];
        for (int x = 0; x < m; ++x) { row[x] += (float)c; const double c2 = c * cb - sn * sb; sn = sn * cb + c * sb; c = c2; }
      }
    }
    double mean = 0.0, var = 0.0;
    for (float v : field) mean += v;
    mean /= (double)field.size();
    for (float v : field) var += (v - mean) * (v - mean);
    const double sd_f = std::sqrt(var / (double)field.size()) + 1e-12;
    const double u0 = unif(), u1 = unif(), u2 = unif(), u3 = unif();
    const double sd = 6.0 * std::exp(u0 * std::log(160.0 / 6.0)), mu_s = 120.0 + 780.0 * u1;
    for (size_t j = 0; j < field.size(); ++j) scene[j] = clip((int)std::lrint(mu_s + sd * (field[j] - mean) / sd_f) + (int)(next() % 3) - 1);
    ref = scene;
    if (u3 < 0.5)
      for (int y = 1; y < m - 1; ++y)
        for (int x = 1; x < m - 1; ++x) {
          const int *r0 = &scene[(size_t)(y - 1) * m + x], *r1 = r0 + m, *r2 = r1 + m;
          ref[(size_t)y * m + x] = (r0[-1] + 2 * r0[0] + r0[1] + 2 * r1[-1] + 4 * r1[0] + 2 * r1[1] + r2[-1] + 2 * r2[0] + r2[1] + 8) / 16;
        }
    const int my = (int)(next() % 5) - 2, mx = (int)(next() % 5) - 2, a = (int)(u2 * 7.0);
    int16_t *o = &ci.org[(size_t)i * cs], *q = &ci.pred[(size_t)i * cs];
    for (int y = 0; y < S; ++y)
      for (int x = 0; x < S; ++x) {
        o[(size_t)y * S + x] = (int16_t)scene[(size_t)(y + 4) * m + x + 4];
        q[(size_t)y * S + x] = (int16_t)clip(ref[(size_t)(y + 4 + my) * m + x + 4 + mx] + (a ? (int)(next() % (uint64_t)(2 * a + 1)) - a : 0));
      }
    ci.poc[i] = (int32_t)(next() % 601);
    ci.qp[i] = 17 + (int32_t)(next() % 31);
  }
  return ci;
}

// The caller's own content for the calibration (mlt_calibrate): n dense CUs in HOST memory, appended to the synthetic set or replacing it.
struct CalibExtra { const int16_t *org, *pred; const int32_t *poc, *qp; int n; bool replace; };

// One calibration session: the calibration CUs resident on the device (the synthetic set, the caller's CUs, or both), their exact logits
// (computed ONCE, 96 CUs at a time: the exact workspace is 5.6 MiB per 128x128 CU), and price(w2 units, exact units) = the set through
// `model` with hi+lo weights / the exact arithmetic in those launch units (0: single pass everywhere), leaving in st.calib_rms the WORST
// pooled rms |dlogit| over {each content class, each head}, in st.calib_max the overall maximum and in tail_ratio max / (rms pooled over
// everything).  Caller CUs the flat-content guard would re-evaluate exactly anyway (same statistic, same thresholds) do not count: the
// admission is about what the non-exact arithmetic will really see.
struct CalibSession {
  mlt_ctx *ctx; SizeState &st;
  const CalibExtra *extra;
  // one resident set of CUs: the synthetic calibration set (+ the caller's), or the in-distribution set behind the magnitude guard
  struct Set {
    int n = 0;
    char *d = nullptr;
    int16_t *d_org = nullptr, *d_pred = nullptr;
    int32_t *d_poc = nullptr, *d_qp = nullptr, *d_split = nullptr;
    float *d_lg = nullptr, *d_mag = nullptr;
    std::vector<int> cls;
    std::vector<char> use;
    std::vector<float> le, lf, mag;   // exact logits, the candidate's logits, logit magnitude (HeadArgs.mag of the exact pass)
  };
  Set main, xtra;
  int n = 0, n_syn = 0, n_used = 0, n_caller_used = 0;
  float tail_ratio = 0.f;
  bool want_mag = false;   // the size may run behind the magnitude guard: the exact pass also delivers the magnitudes
  static constexpr int kSub = 96;
  CalibSession(mlt_ctx *c, SizeState &s, const CalibExtra *e = nullptr) : ctx(c), st(s), extra(e) {}
  ~CalibSession() {
    if (main.d) (void)hipFree(main.d);
    if (xtra.d) (void)hipFree(xtra.d);
    // the workspace grew to 96 exact CUs (540 MiB at S = 128): release it, the first real call sizes it for its own batch (a max_batch = 1
    // encoder context would otherwise carry it for life); captured graphs of every size that baked the old workspace in are dropped
    // with it (a later allocation may return the same address with fewer bytes behind it)
    (void)hipStreamSynchronize(ctx->stream);
    release_ws(ctx);
  }
  int alloc(Set &t, int count) {
    const int S = st.size, nl = st.model.n_logits;
    const size_t cs = (size_t)S * S, plane = cs * 2 * (size_t)count;
    t.n = count;
    HIP_TRY(ctx, hipMalloc((void **)&t.d, 2 * plane + 4 * (size_t)count * 4 + (size_t)count * nl * 4));
    t.d_org = (int16_t *)t.d; t.d_pred = (int16_t *)(t.d + plane);
    t.d_poc = (int32_t *)(t.d + 2 * plane); t.d_qp = t.d_poc + count; t.d_split = t.d_qp + count;
    t.d_mag = (float *)(t.d_split + count);
    t.d_lg = t.d_mag + count;
    return MLT_OK;
  }
  // which CUs of t[first ..) the flat-content guard re-evaluates exactly at run time (flat_stat_kernel's statistic under the flat test of guard_rule,
  // mlt_tail_kernels.inc -- its one host-side restatement, at the thresholds of guard_thresholds): those never see the arithmetic being priced
  int drop_flat(Set &t, int first, int div = 8, std::vector<char> *mask = nullptr) {
    const int S = st.size, cnt = t.n - first;
    const size_t cs = (size_t)S * S;
    if (!st.cfg_flat_guard || cnt <= 0) return MLT_OK;
    FlatStatArgs fa{};
    Planes::dense(t.d_org + cs * first, t.d_pred + cs * first, S).fill(fa);
    fa.flat = t.d_split; fa.n = cnt; fa.s_l = ilog2(S);
    HIP_TRY(ctx, mlt_launch_flat_stat(fa, true, ctx->stream));
    std::vector<int32_t> fl((size_t)cnt);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(fl.data(), t.d_split, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    const int flat_thr = (S * S / 4) / div, near_thr = (S * S / 4) / 2;
    std::vector<char> &u = mask ? *mask : t.use;
    for (int i = 0; i < cnt; ++i)
      if ((fl[(size_t)i] >> MLT_FLAT_EXACT_SHIFT) >= flat_thr || (fl[(size_t)i] & 0xFFFF) >= near_thr) u[(size_t)(first + i)] = 0;
    return MLT_OK;
  }
  // the arithmetic being priced: `whole` everywhere, or `model` with hi+lo weights in the launch units of mask and the exact arithmetic in those of xmask
  NetCfg candidate(unsigned mask, unsigned xmask, mlt::Model *whole) {
    NetCfg c;
    c.S = st.size; c.m = whole ? whole : &st.model;
    if (!whole && mask) { c.mback = &st.model_w2; c.back_mask = mask; }
    if (!whole && xmask) { c.mx = &st.model_exact; c.x_units = xmask; }
    return c;
  }
  // the set through the arithmetic of `c`, kSub CUs at a time: logits -> out (with_mag: and the logit magnitudes -> t.mag)
  int run(Set &t, std::vector<float> &out, const NetCfg &c, bool with_mag) {
    const int S = st.size, nl = st.model.n_logits;
    const size_t cs = (size_t)S * S;
    const bool prof = ctx->profile;
    ctx->profile = false;
    int rc = MLT_OK;
    for (int i0 = 0; i0 < t.n && rc == MLT_OK; i0 += kSub) {
      GuardOut go;
      go.d_mag = with_mag ? t.d_mag + i0 : nullptr;
      rc = run_network(ctx, st, c, t.n - i0 < kSub ? t.n - i0 : kSub,
                       PassIO{Planes::dense(t.d_org + i0 * cs, t.d_pred + i0 * cs, S), t.d_poc + i0, t.d_qp + i0, t.d_split, t.d_lg + (size_t)i0 * nl, nullptr}, go);
    }
    ctx->profile = prof;
    if (rc) return rc;
    out.resize((size_t)t.n * nl);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out.data(), t.d_lg, out.size() * 4, hipMemcpyDeviceToHost));
    if (with_mag) {
      t.mag.resize((size_t)t.n);
      HIP_TRY(ctx, hipMemcpy(t.mag.data(), t.d_mag, (size_t)t.n * 4, hipMemcpyDeviceToHost));
    }
    return MLT_OK;
  }
  // MLT_CALIB_REPLACE needs enough of the caller's CUs to carry the statistical admission rule on their own (it assumes thousands of logits:
  // the synthetic set has 560 CUs): when fewer than kCalibMinReplace of them are left after dropping those the flat-content guard re-evaluates
  // exactly anyway -- all of them flat, or a tiny n -- the synthetic set is kept and the caller's CUs are APPENDED to it instead (visible to the
  // caller as mlt_arith_info.calib_cus > calib_caller_cus).  No tier is ever admitted on an empty or near-empty set.
  static constexpr int kCalibMinReplace = 256;
  int begin() {
    int rc = stage_set(extra && extra->replace);
    if (rc == MLT_OK && extra && extra->replace && n_used < kCalibMinReplace) {
      (void)hipFree(main.d);
      main = Set();
      rc = stage_set(false);
    }
    return rc ? rc : run(main, main.le, st.exact_cfg(), want_mag);
  }
  int stage_set(bool replace) {
    const int S = st.size;
    const size_t cs = (size_t)S * S;
    const CalibInputs *syn = replace ? nullptr : &calibration_set(S);
    n_syn = syn ? kCalibN : 0;
    const int n_ex = extra ? extra->n : 0;
    n = n_syn + n_ex;
    int rc = alloc(main, n);
    if (rc) return rc;
    main.cls.assign((size_t)n, kCalibClasses);
    main.use.assign((size_t)n, 1);
    if (syn) std::copy(syn->cls.begin(), syn->cls.end(), main.cls.begin());
    if (syn) {
      HIP_TRY(ctx, hipMemcpy(main.d_org, syn->org.data(), cs * 2 * kCalibN, hipMemcpyHostToDevice));
      HIP_TRY(ctx, hipMemcpy(main.d_pred, syn->pred.data(), cs * 2 * kCalibN, hipMemcpyHostToDevice));
      HIP_TRY(ctx, hipMemcpy(main.d_poc, syn->poc.data(), (size_t)kCalibN * 4, hipMemcpyHostToDevice));
      HIP_TRY(ctx, hipMemcpy(main.d_qp, syn->qp.data(), (size_t)kCalibN * 4, hipMemcpyHostToDevice));
    }
    if (n_ex) {
      HIP_TRY(ctx, hipMemcpy(main.d_org + cs * n_syn, extra->org, cs * 2 * (size_t)n_ex, hipMemcpyHostToDevice));
      HIP_TRY(ctx, hipMemcpy(main.d_pred + cs * n_syn, extra->pred, cs * 2 * (size_t)n_ex, hipMemcpyHostToDevice));
      HIP_TRY(ctx, hipMemcpy(main.d_poc + n_syn, extra->poc, (size_t)n_ex * 4, hipMemcpyHostToDevice));
      HIP_TRY(ctx, hipMemcpy(main.d_qp + n_syn, extra->qp, (size_t)n_ex * 4, hipMemcpyHostToDevice));
      if ((rc = drop_flat(main, n_syn))) return rc;
    }
    n_used = 0; n_caller_used = 0;
    for (int i = 0; i < n; ++i) { n_used += main.use[(size_t)i]; if (i >= n_syn) n_caller_used += main.use[(size_t)i]; }
    return MLT_OK;
  }
  struct TierPrice_ { float rms = 0.f, max = 0.f, tail = 0.f; double cls_rms[kCalibClasses + 2] = {0}, head_rms[4] = {0}; };
  // pooled figures of (candidate - exact) over the CUs of `sets` that count and whose magnitude is <= thr (thr <= 0: all of them)
  void pool(const Set *const *sets, int n_sets, float thr, TierPrice_ &out, int *n_kept = nullptr, const std::vector<char> *const *masks = nullptr) {
    const int nl = st.model.n_logits;
    double mx = 0.0, s2_all = 0.0;
    double s2_cls[kCalibClasses + 2] = {0}, s2_head[4] = {0};
    size_t n_cls[kCalibClasses + 2] = {0}, n_head[4] = {0}, n_all = 0;
    int kept = 0;
    for (int t = 0; t < n_sets; ++t) {
      const Set &T = *sets[t];
      const std::vector<char> &use = masks ? *masks[t] : T.use;
      for (int i = 0; i < T.n; ++i) {
        if (!use[(size_t)i]) continue;
        if (thr > 0.f && !(T.mag[(size_t)i] <= thr)) continue;
        ++kept;
        int lo = 0;
        for (int h = 0; h < st.model.n_heads; ++h) {
          for (int k = 0; k < st.model.heads[h].classes; ++k) {
            const size_t j = (size_t)i * nl + lo + k;
            const double e = std::fabs((double)T.lf[j] - (double)T.le[j]);
            if (!(e <= mx)) mx = e;  // NaN -> mx = NaN -> fails the admission test
            s2_cls[T.cls[(size_t)i]] += e * e; ++n_cls[T.cls[(size_t)i]];
            s2_head[h] += e * e; ++n_head[h];
            s2_all += e * e; ++n_all;
          }
          lo += st.model.heads[h].classes;
        }
      }
    }
    double worst = 0.0;
    for (int c = 0; c < kCalibClasses + 2; ++c) if (n_cls[c]) { const double r = std::sqrt(s2_cls[c] / (double)n_cls[c]); if (!(r <= worst)) worst = r; }
    for (int h = 0; h < st.model.n_heads; ++h) if (n_head[h]) { const double r = std::sqrt(s2_head[h] / (double)n_head[h]); if (!(r <= worst)) worst = r; }
    const double rms_all = n_all ? std::sqrt(s2_all / (double)n_all) : 0.0;
    out.rms = (float)worst; out.max = (float)mx; out.tail = (float)(rms_all > 0.0 ? mx / rms_all : 0.0);
    for (int c = 0; c < kCalibClasses + 2; ++c) out.cls_rms[c] = std::sqrt(s2_cls[c] / (double)(n_cls[c] ? n_cls[c] : 1));
    for (int h = 0; h < 4; ++h) out.head_rms[h] = std::sqrt(s2_head[h] / (double)(n_head[h] ? n_head[h] : 1));
    if (n_kept) *n_kept = kept;
  }
  int price(unsigned mask, unsigned xmask, mlt::Model *whole) {
    int rc = run(main, main.lf, candidate(mask, xmask, whole), false);
    if (rc) return rc;
    TierPrice_ P;
    const Set *sets[1] = {&main};
    std::vector<char> keep_use;
    if (whole && st.cfg_flat_guard) {  // the exact-lite tier runs behind the flat guard at 1 / 16 (SizeState.flat_div): the CUs THAT guard re-evaluates do not count
      keep_use = main.use;
      if ((rc = drop_flat(main, 0, 16))) return rc;
    }
    pool(sets, 1, 0.f, P);
    if (!keep_use.empty()) main.use = keep_use;
    tail_ratio = P.tail;
    if (std::getenv("MLT_CALIB_VERBOSE")) {  // diagnostics: which content class / head decides the admission
      std::fprintf(stderr, "mltcnn calibration (size %d, %d CUs of which %d the caller's, hi+lo weights in units 0x%x, exact in units 0x%x): rms per class", st.size, n_used, n_caller_used, mask, xmask);
      for (int c = 0; c <= kCalibClasses; ++c) std::fprintf(stderr, " %.3e", P.cls_rms[c]);
      std::fprintf(stderr, " | per head");
      for (int h = 0; h < st.model.n_heads; ++h) std::fprintf(stderr, " %.3e", P.head_rms[h]);
      std::fprintf(stderr, " | max %.3e = %.1f x rms\n", (double)P.max, (double)tail_ratio);
    }
    st.calibrated = true;
    st.calib_rms = P.rms;
    st.calib_max = P.max;
    return MLT_OK;
  }
  // The configuration price() has just measured, behind the MAGNITUDE guard.  Threshold: the LARGEST magnitude T on a quarter-octave grid (from the
  // largest magnitude in the sets downwards) such that the CUs with M <= T -- main set + the in-distribution set, which is staged, and its exact
  // logits computed, on first use -- meet the REFINED admission rule (mlt_tier_search.h: k x rms <= 0.95 x and max <= 0.6 x tolerance: the rule for
  // choices made on the calibration data itself) with at least kGuardMinKept CUs left and at most flag_max of the in-distribution CUs above T.
  // The rule is the plain one applied to the population that will really run the tier -- the logic of the flat-content guard ("content the guard
  // catches does not count") with the threshold found instead of fixed.  (A first form derived T from the worst RELATIVE error over all CUs,
  // T = 0.65 x tolerance / max(e / M): it charged ordinary content for the relative error of the constant-band classes -- 4 x the others' -- and
  // flagged 9 % of it where the kept CUs' largest error was a quarter of the limit: profiles/r06b_calib_trained1.txt.)
  static constexpr int kGuardMinKept = 256;
  int price_guarded(unsigned mask, unsigned xmask, const mlt::TierRules &R, mlt::TierPrice &out) {
    out.g_valid = false;
    if (!want_mag || main.mag.size() != (size_t)main.n) return MLT_OK;
    int rc;
    if (!xtra.d) {
      const CalibInputs &ci = calibration_extra_set(st.size);
      const size_t cs = (size_t)st.size * st.size;
      if ((rc = alloc(xtra, kCalibExtraN))) return rc;
      xtra.cls = ci.cls;
      xtra.use.assign((size_t)kCalibExtraN, 1);
      HIP_TRY(ctx, hipMemcpy(xtra.d_org, ci.org.data(), cs * 2 * kCalibExtraN, hipMemcpyHostToDevice));
      HIP_TRY(ctx, hipMemcpy(xtra.d_pred, ci.pred.data(), cs * 2 * kCalibExtraN, hipMemcpyHostToDevice));
      HIP_TRY(ctx, hipMemcpy(xtra.d_poc, ci.poc.data(), (size_t)kCalibExtraN * 4, hipMemcpyHostToDevice));
      HIP_TRY(ctx, hipMemcpy(xtra.d_qp, ci.qp.data(), (size_t)kCalibExtraN * 4, hipMemcpyHostToDevice));
      if ((rc = drop_flat(xtra, 0))) return rc;
      if ((rc = run(xtra, xtra.le, st.exact_cfg(), true))) return rc;
    }
    if ((rc = run(xtra, xtra.lf, candidate(mask, xmask, nullptr), false))) return rc;
    const Set *sets[2] = {&main, &xtra};
    // A tier behind the magnitude guard also runs the FLAT guard at 1 / 16 of the quads exactly flat instead of 1 / 8 (SizeState.flat_div): the weight
    // sets that need this guard are the ones whose errors grow with what they amplify, and a 10-12 % constant band -- just under 1 / 8 -- was the one class
    // whose deep tail left the contract behind the guard (5 of 331,776 probed logits of the first trained family at 1.0-1.35e-3, all in that class:
    // profiles/r06d_tail_probe_trained.txt; 80 such CUs in the calibration set do not see a 1-in-7000 event).  The CUs THAT guard takes do not count here.
    if (use16[0].empty()) {
      use16[0] = main.use; use16[1] = xtra.use;
      if ((rc = drop_flat(main, 0, 16, &use16[0]))) return rc;
      if ((rc = drop_flat(xtra, 0, 16, &use16[1]))) return rc;
    }
    const std::vector<char> *masks[2] = {&use16[0], &use16[1]};
    float m_hi = 0.f, m_lo = INFINITY;
    int in_dist = 0;
    for (int t = 0; t < 2; ++t) {
      const Set *T = sets[t];
      for (int i = 0; i < T->n; ++i) {
        if (!use16[t][(size_t)i]) continue;
        const float m = T->mag[(size_t)i];
        if (!(m > 0.f) || !std::isfinite(m)) return MLT_OK;   // (a NaN / zero magnitude: no guarded variant)
        if (m > m_hi) m_hi = m;
        if (m < m_lo) m_lo = m;
        const int c = T->cls[(size_t)i];
        if (c == 0 || c == kCalibClasses || c == kClassScenes) ++in_dist;
      }
    }
    if (!(m_hi > 0.f) || in_dist == 0) return MLT_OK;
    const bool verbose = std::getenv("MLT_CALIB_VERBOSE") != nullptr;
    for (float thr = m_hi * 0.840896415f; thr >= m_lo; thr *= 0.840896415f) {   // 2^(-1/4) per step; T = m_hi would be the plain rule again
      TierPrice_ P;
      int kept = 0;
      pool(sets, 2, thr, P, &kept, masks);
      if (kept < kGuardMinKept) break;
      mlt::TierPrice tp;
      tp.rms = P.rms; tp.max = P.max; tp.tail = P.tail;
      if (!R.within_refined(tp)) continue;
      // the guard's price on ordinary content: the in-distribution CUs (texture, 1/f scenes, the caller's own) it sends to the exact re-run
      int flagged = 0;
      for (int t = 0; t < 2; ++t) {
        const Set *T = sets[t];
        for (int i = 0; i < T->n; ++i) {
          const int c = T->cls[(size_t)i];
          if (use16[t][(size_t)i] && (c == 0 || c == kCalibClasses || c == kClassScenes) && !(T->mag[(size_t)i] <= thr)) ++flagged;
        }
      }
      out.g_valid = true;
      out.g_rms = P.rms; out.g_max = P.max; out.g_tail = P.tail; out.g_thr = thr; out.g_flag = (float)flagged / (float)in_dist;
      if (verbose) {
        std::fprintf(stderr, "mltcnn calibration, behind the magnitude guard (threshold %.3f of %.3f .. %.3f: %d CUs at or below it, %d of %d in-distribution CUs above): rms per class",
                     (double)thr, (double)m_lo, (double)m_hi, kept, flagged, in_dist);
        for (int c = 0; c < kCalibClasses + 2; ++c) std::fprintf(stderr, " %.3e", P.cls_rms[c]);
        std::fprintf(stderr, " | per head");
        for (int h = 0; h < st.model.n_heads; ++h) std::fprintf(stderr, " %.3e", P.head_rms[h]);
        std::fprintf(stderr, " | max %.3e = %.1f x rms\n", (double)P.max, (double)P.tail);
      }
      return MLT_OK;
    }
    if (verbose) std::fprintf(stderr, "mltcnn calibration, behind the magnitude guard: no threshold in %.3f .. %.3f meets the refined rule with >= %d CUs\n", (double)m_lo, (double)m_hi, kGuardMinKept);
    return MLT_OK;
  }
  std::vector<char> use16[2];   // main / xtra: the CUs that count behind the flat guard at 1 / 16
};

}  // namespace
void drop_graphs(mlt_ctx *ctx, int si) {  // a captured kernel chain bakes in weight / workspace pointers
  for (int v = 0; v < 3; ++v) {
    SingleCu &sg = ctx->single[si + 4 * v];
    if (sg.exec) (void)hipGraphExecDestroy(sg.exec);
    if (sg.graph) (void)hipGraphDestroy(sg.graph);
    sg.exec = nullptr; sg.graph = nullptr;
  }
}
namespace {

// The pricer of the tier search (mlt_tier_search.h) on the device: a configuration = launch units in hi+lo weights / in the exact arithmetic +
// the realisation of the single-pass weights' rounding.  Models are built and uploaded lazily: another realisation replaces st.model
// (~50 ms each), the hi+lo-weights copy appears with the first candidate that needs it.
struct DevicePricer : mlt::TierPricer {
  mlt_ctx *ctx; SizeState &st; CalibSession &cal;
  const void *blob; size_t bytes; int size;
  int cur_rounding = 0;
  const mlt::TierRules *rules = nullptr;   // != NULL: configurations the plain rule rejects are also priced behind the magnitude guard
  DevicePricer(mlt_ctx *c, SizeState &s, CalibSession &cs, const void *b, size_t n, int sz) : ctx(c), st(s), cal(cs), blob(b), bytes(n), size(sz) {}
  int price(unsigned w2_units, unsigned x_units, int rounding, mlt::TierPrice &out) override {
    std::string err;
    int rc;
    if (rounding != cur_rounding) {
      mlt::Model mv;
      if (!mlt::build_model(blob, bytes, mlt::MLT_MODEL_FAST, size, mv, err, rounding)) { ctx->err = "weights (rounding " + std::to_string(rounding) + "): " + err; return MLT_ERR_WEIGHTS; }
      if ((rc = upload_model(ctx, mv))) { free_model(mv); return rc; }
      std::swap(st.model, mv);
      free_model(mv);
      cur_rounding = rounding;
    }
    if (w2_units && !st.model_w2.on_device) {
      mlt::Model mw;
      if (!mlt::build_model(blob, bytes, mlt::MLT_MODEL_W2, size, mw, err)) { ctx->err = "weights (hi+lo copy): " + err; return MLT_ERR_WEIGHTS; }
      st.model_w2 = std::move(mw);
      if ((rc = upload_model(ctx, st.model_w2))) return rc;
    }
    if ((rc = cal.price(w2_units, x_units, nullptr))) return rc;
    out.rms = st.calib_rms; out.max = st.calib_max; out.tail = cal.tail_ratio;
    // (the refined rule is the stricter of the two: whatever the search is about to test, a configuration that fails it gets its guarded figures)
    if (rules && cal.want_mag && !rules->within_refined(out) && (rc = cal.price_guarded(w2_units, x_units, *rules, out))) return rc;
    return MLT_OK;
  }
  int price_lite(mlt::TierPrice &out) override {
    std::string err;
    int rc;
    if (!st.model_xl.on_device) {
      mlt::Model mx;
      if (!mlt::build_model(blob, bytes, mlt::MLT_MODEL_XLITE, size, mx, err)) { ctx->err = "weights (exact-lite copy): " + err; return MLT_ERR_WEIGHTS; }
      st.model_xl = std::move(mx);
      if ((rc = upload_model(ctx, st.model_xl))) return rc;
    }
    if ((rc = cal.price(0, 0, &st.model_xl))) return rc;
    out.rms = st.calib_rms; out.max = st.calib_max; out.tail = cal.tail_ratio;
    return MLT_OK;
  }
};

int env_int(const char *name) {  // tuning switch holding a number (MLT_TUNING=1 only); -1: not set
  const char *e = tuning_env(name);
  return e ? (int)std::strtol(e, nullptr, 0) : -1;
}

void unload_size(mlt_ctx *ctx, int si) {
  SizeState &st = ctx->sz[si];
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  drop_graphs(ctx, si);
  free_model(st.model); free_model(st.model_exact); free_model(st.model_w2); free_model(st.model_xl);
  st.model = mlt::Model(); st.model_exact = mlt::Model(); st.model_w2 = mlt::Model(); st.model_xl = mlt::Model();
  st.loaded = false;
  st.plans.clear();
}

// Load (or re-calibrate: `extra` = the caller's CUs) ONE device's copy of a size.  blob / bytes stay valid for the call.
int load_one(mlt_ctx *ctx, int size, const void *blob, size_t bytes, const CalibExtra *extra) {
  const int si = size_index(size);
  if (si < 0) { ctx->err = "unsupported CU size"; return MLT_ERR_ARG; }
  SizeState &st = ctx->sz[si];
  if (!st.enabled) { ctx->err = "CU size not enabled in size_mask"; return MLT_ERR_SIZE_DISABLED; }
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  std::string err;
  mlt::Model m;
  const bool no_small_mix = tuning().no_small_mix;
  const bool small_mix = st.small_mix && !no_small_mix;   // (then: fast copy = `model`, exact copy = `model_exact`, the calibration picks the stages)
  if (!mlt::build_model(blob, bytes, (st.want_exact && !small_mix) ? (ctx->xlite ? mlt::MLT_MODEL_XLITE : mlt::MLT_MODEL_EXACT) : mlt::MLT_MODEL_FAST, size, m, err)) { ctx->err = "weights: " + err; return MLT_ERR_WEIGHTS; }
  if (m.arch != (size == 128 ? 0 : 1)) { ctx->err = "weights: blob arch does not match CU size"; return MLT_ERR_WEIGHTS; }
  if (st.head_index < 0 || st.head_index >= m.n_heads) { ctx->err = "head_index out of range"; return MLT_ERR_ARG; }
  // a reload replaces device buffers that captured graphs and in-flight work point to
  (void)hipStreamSynchronize(ctx->stream);
  drop_graphs(ctx, si);
  // (models own device buffers: whatever the state held -- loaded or left over from a failed load -- is released first, and every
  // error path below releases what it uploaded, so a failed reload leaves the size cleanly unloaded instead of leaking)
  free_model(st.model); free_model(st.model_exact); free_model(st.model_w2); free_model(st.model_xl);
  st.loaded = false;
  st.plans.clear();
  st.exact = st.want_exact && !small_mix;
  st.lite = false; st.flat_guard = st.cfg_flat_guard; st.flat_div = 8; st.guard_margin = ctx->guard_margin;
  st.w2 = false; st.w2_mask = 0; st.w2_units = 0; st.x_mask = 0; st.x_units = 0;
  st.mag_thr = 0.f; st.calib_rel = 0.f; st.mag_flag = 0.f; st.mag_kind = 0;
  st.calibrated = false; st.calib_rms = st.calib_max = 0.f;
  st.calib_cus = st.calib_caller_cus = 0;
  st.model = std::move(m);
  st.model_exact = mlt::Model();
  st.model_w2 = mlt::Model();
  st.model_xl = mlt::Model();
  auto fail = [&](int rc) {
    free_model(st.model); free_model(st.model_exact); free_model(st.model_w2); free_model(st.model_xl);
    st.model = mlt::Model(); st.model_exact = mlt::Model(); st.model_w2 = mlt::Model(); st.model_xl = mlt::Model();
    return rc;
  };
  int rc = upload_model(ctx, st.model);
  if (rc) return fail(rc);
  if (!st.exact && (st.flat_guard || st.margin_guard || st.calibrate || small_mix)) {
    mlt::Model me;
    if (!mlt::build_model(blob, bytes, mlt::MLT_MODEL_EXACT, size, me, err)) { ctx->err = "weights (exact copy): " + err; return fail(MLT_ERR_WEIGHTS); }
    st.model_exact = std::move(me);
    if ((rc = upload_model(ctx, st.model_exact))) return fail(rc);
    if (small_mix || st.calibrate) {
      // The search itself lives in mlt_tier_search.h (no HIP in it; unit-tested on the CPU with a stub pricer):
      //  128: single pass -> other realisations of the weights' rounding -> hi+lo weights in a subset of stages (cheapest first) -> some stages
      //       exact -> refinements at launch-unit granularity -> exact;
      //  64 / 32 / 16 (maps of 1 .. 32 pixels: their time is in the FIRST stages, their error in the LAST ones): the longest single-pass
      //       prefix, layer0 with hi+lo weights, half of layer0 -> exact.  Largest error held to 0.5 x tolerance (their tails are heavier:
      //       profiles/r04s_tail_probe_{64,32}.txt measured 1.5 .. 1.85 x the calibration set's largest error).
      CalibSession cal(ctx, st, extra);
      // (the magnitude guard serves the 128 model's tiers; the small models' search is over exact prefixes and is left as it was)
      const bool no_mag = tuning().no_mag_guard;
      cal.want_mag = !small_mix && st.cfg_mag_guard && !no_mag;
      if ((rc = cal.begin())) return fail(rc);
      DevicePricer pricer(ctx, st, cal, blob, bytes, size);
      mlt::TierRules rules;
      rules.tolerance = ctx->tolerance;
      rules.max_frac = small_mix ? 0.5f : 0.65f;
      if (cal.want_mag) pricer.rules = &rules;
      mlt::TierForce force;
      force.no_mag_guard = !cal.want_mag;
      force.rounding = env_int("MLT_ROUNDING"); force.w2_mask = env_int("MLT_W2_MASK"); force.x_mask = env_int("MLT_X_MASK");
      force.w2_units = env_int("MLT_W2_UNITS"); force.small_prefix = env_int("MLT_SMALL_PREFIX");
      force.x_units = env_int("MLT_X_UNITS");
      force.no_roundings = tuning_env("MLT_NO_ROUNDINGS") != nullptr; force.no_w2 = tuning_env("MLT_NO_W2") != nullptr;
      force.no_xmix = tuning_env("MLT_NO_XMIX") != nullptr; force.no_w2_units = tuning_env("MLT_NO_W2_UNITS") != nullptr;
      force.no_x_units = tuning_env("MLT_NO_X_UNITS") != nullptr; force.no_lite = tuning_env("MLT_NO_LITE") != nullptr;
      mlt::TierChoice ch;
      rc = small_mix ? mlt::search_tier_small(pricer, rules, force, st.model.n_stages, ch) : mlt::search_tier_128(pricer, rules, force, mlt::MLT_N_ROUNDINGS, ch);
      if (rc == mlt::kTierErrIllegalForce) { ctx->err = "MLT_X_UNITS / MLT_W2_UNITS: a single-pass stride-2 conv in front of a two-plane chain"; rc = MLT_ERR_ARG; }
      if (rc) return fail(rc);
      st.calib_cus = cal.n_used; st.calib_caller_cus = cal.n_caller_used;
      st.calib_rms = ch.price.rms; st.calib_max = ch.price.max;
      if (ch.lite) {  // the exact-lite arithmetic everywhere: its model becomes `model`; the exact copy stays for the decision guard's near-ties
        free_model(st.model_w2); st.model_w2 = mlt::Model();
        free_model(st.model);
        st.model = std::move(st.model_xl);
        st.model_xl = mlt::Model();
        st.lite = true;
        st.flat_guard = st.cfg_flat_guard;   // (round 5 switched it off here; round 6: on, at 1 / 16 of the quads exactly flat)
        st.flat_div = 16;
        if (!ctx->guard_margin_configured) st.guard_margin = std::min(ctx->guard_margin, std::max(1e-4f, 3.f * 1.7f * st.calib_max));
        if (!st.margin_guard && !st.flat_guard) { free_model(st.model_exact); st.model_exact = mlt::Model(); }
      } else if (ch.exact) {  // run it exact
        free_model(st.model_w2); st.model_w2 = mlt::Model();
        free_model(st.model_xl); st.model_xl = mlt::Model();
        free_model(st.model);
        st.model = std::move(st.model_exact);
        st.model_exact = mlt::Model();
        st.exact = true;
      } else {
        free_model(st.model_xl); st.model_xl = mlt::Model();
        st.w2 = ch.w2;
        st.w2_units = ch.w2_units; st.x_units = ch.x_units;
        st.w2_mask = mlt::stages_of_units(ch.w2_units); st.x_mask = mlt::stages_of_units(ch.x_units);
        if (!st.w2) { free_model(st.model_w2); st.model_w2 = mlt::Model(); }
        st.mag_thr = ch.mag_thr; st.mag_flag = ch.mag_flag;   // > 0: the tier was admitted behind the magnitude guard
        if (st.mag_thr > 0.f) { st.flat_div = 16; st.mag_kind = 2; }   // ... and then runs the flat guard at 1 / 16 (CalibSession::price_guarded)
        st.calib_rel = ch.mag_thr > 0.f ? ch.price.max / ch.mag_thr : 0.f;
      }
      // the RANGE guard of every non-exact tier the plain rule admitted (SizeState.mag_kind == 1)
      if (!st.exact && st.mag_kind == 0 && cal.want_mag && cal.main.mag.size() == (size_t)cal.main.n) {
        float m_hi = 0.f;
        for (int i = 0; i < cal.main.n; ++i)
          if (cal.main.use[(size_t)i] && cal.main.mag[(size_t)i] > m_hi) m_hi = cal.main.mag[(size_t)i];
        if (m_hi > 0.f && std::isfinite(m_hi)) { st.mag_thr = kMagRange * m_hi; st.mag_kind = 1; }
      }
    }
  }
  st.loaded = true;
  return MLT_OK;
}

// every device of a context: load / re-calibrate, then make sure they all landed on the SAME arithmetic (the header promises results
// bit-identical to a one-device context); on any failure the size is unloaded everywhere (no mixed weight sets)
int load_all(mlt_ctx *ctx, int size, const void *blob, size_t bytes, const CalibExtra *extra) {
  const int si = size_index(size);
  if (si < 0) { ctx->err = "unsupported CU size"; return MLT_ERR_ARG; }
  int rc = load_one(ctx, size, blob, bytes, extra);
  for (size_t i = 0; i < ctx->peers.size() && rc == MLT_OK; ++i) {
    mlt_ctx *p = ctx->peers[i];
    rc = load_one(p, size, blob, bytes, extra);
    if (rc) ctx->err = "device " + std::to_string(p->device) + ": " + p->err;
    else {
      const SizeState &a = ctx->sz[si], &b = p->sz[si];
      if (a.exact != b.exact || a.lite != b.lite || a.w2 != b.w2 || a.w2_units != b.w2_units || a.x_units != b.x_units || a.model.rounding != b.model.rounding || a.mag_thr != b.mag_thr || a.mag_kind != b.mag_kind) {
        ctx->err = "device " + std::to_string(p->device) + " calibrated to a different arithmetic than device " + std::to_string(ctx->device);
        rc = MLT_ERR_WEIGHTS;
      }
    }
  }
  if (rc) {
    unload_size(ctx, si);
    for (mlt_ctx *p : ctx->peers) unload_size(p, si);
    ctx->sz[si].blob.clear();
  }
  return rc;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int mlt_load_weights(mlt_ctx *ctx, int size, const void *blob, size_t bytes) {
  if (!ctx || !blob) return MLT_ERR_ARG;
  const int si = size_index(size);
  if (si < 0) { ctx->err = "unsupported CU size"; return MLT_ERR_ARG; }
  // the library keeps the blob (5.6 - 6.3 MB): mlt_calibrate re-packs from it
  std::vector<char> keep((const char *)blob, (const char *)blob + bytes);
  const int rc = load_all(ctx, size, keep.data(), keep.size(), nullptr);
  if (rc == MLT_OK) ctx->sz[si].blob = std::move(keep);
  return rc;
}

int mlt_calibrate(mlt_ctx *ctx, int size, const int16_t *org, const int16_t *pred, const int32_t *poc, const int32_t *qp, int n, int mode) {
  if (!ctx) return MLT_ERR_ARG;
  if (!org || !pred || !poc || !qp || n <= 0 || n > kCalibCallerMax || (mode != MLT_CALIB_APPEND && mode != MLT_CALIB_REPLACE)) { ctx->err = "mlt_calibrate: bad argument"; return MLT_ERR_ARG; }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  if (st->blob.empty()) { ctx->err = "mlt_calibrate: no weight blob kept for this size"; return MLT_ERR_WEIGHTS; }
  if (!st->calibrate && !st->small_mix) return MLT_OK;  // configured exact / calibration switched off: nothing to decide
  const CalibExtra ex{org, pred, poc, qp, n, mode == MLT_CALIB_REPLACE};
  std::vector<char> keep = std::move(st->blob);  // (load_all clears the kept blob on failure)
  rc = load_all(ctx, size, keep.data(), keep.size(), &ex);
  if (rc == MLT_OK) ctx->sz[size_index(size)].blob = std::move(keep);
  return rc;
}

// Host-only hook (not part of include/mltcnn.h; no HIP call): the synthetic calibration set of a CU size, so that the numerics tools
// (tools/attribute_error.py, scripts/emul_fast.py) and the CPU tests see exactly the CUs the load-time calibration prices.  Buffers: dense
// [560][size][size] int16 org / pred, int32 poc / qp / content class; any of them may be NULL.  Returns the number of CUs (560) or -1.
int mlt_calibration_set_copy(int size, int16_t *org, int16_t *pred, int32_t *poc, int32_t *qp, int32_t *cls) {
  if (size_index(size) < 0) return -1;
  const CalibInputs &ci = calibration_set(size);
  const size_t cs = (size_t)size * size * kCalibN;
  if (org) std::memcpy(org, ci.org.data(), cs * 2);
  if (pred) std::memcpy(pred, ci.pred.data(), cs * 2);
  if (poc) std::memcpy(poc, ci.poc.data(), (size_t)kCalibN * 4);
  if (qp) std::memcpy(qp, ci.qp.data(), (size_t)kCalibN * 4);
  if (cls) for (int i = 0; i < kCalibN; ++i) cls[i] = ci.cls[(size_t)i];
  return kCalibN;
}

// CPU test hook of the tier search (mlt_tier_search.h; not part of include/mltcnn.h): no HIP call on this path
int mlt_tier_search_run_n(int kind, int n, float tolerance, float max_frac, const int *force, int n_force,
                          int (*price_cb)(void *user, unsigned w2_units, unsigned x_units, int rounding, float *out3), void *user, int *result, float *figures) {
  if (!price_cb || !result || !figures || n <= 0 || (force && n_force < 12)) return MLT_ERR_ARG;
  struct CbPricer : mlt::TierPricer {
    int (*cb)(void *, unsigned, unsigned, int, float *); void *user;
    int price(unsigned w2u, unsigned xu, int r, mlt::TierPrice &out) override {
      float o[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const int rc = cb(user, w2u, xu, r, o);
      out.rms = o[0]; out.max = o[1]; out.tail = o[2];
      out.g_valid = o[3] != 0.f; out.g_rms = o[4]; out.g_max = o[5]; out.g_tail = o[6]; out.g_thr = o[7]; out.g_flag = o[8];
      return rc;
    }
    int price_lite(mlt::TierPrice &out) override { return price(~0u, ~0u, 0, out); }
  } pricer;
  pricer.cb = price_cb; pricer.user = user;
  mlt::TierRules rules;
  if (tolerance > 0.f) rules.tolerance = tolerance;
  if (max_frac > 0.f) rules.max_frac = max_frac;
  mlt::TierForce f;
  if (force) {
    f.rounding = force[0]; f.w2_mask = force[1]; f.x_mask = force[2]; f.w2_units = force[3]; f.small_prefix = force[4];
    f.no_roundings = force[5] != 0; f.no_w2 = force[6] != 0; f.no_xmix = force[7] != 0; f.no_w2_units = force[8] != 0; f.no_x_units = force[9] != 0; f.no_lite = force[10] != 0; f.no_mag_guard = force[11] != 0;
    if (n_force > 12) f.x_units = force[12];
  }
  mlt::TierChoice ch;
  const int rc = kind == 0 ? mlt::search_tier_128(pricer, rules, f, n, ch) : mlt::search_tier_small(pricer, rules, f, n, ch);
  result[0] = ch.exact ? 1 : 0; result[1] = ch.w2 ? 1 : 0; result[2] = (int)ch.w2_units; result[3] = (int)ch.x_units; result[4] = ch.rounding; result[5] = ch.priced;
  result[6] = ch.lite ? 1 : 0; result[7] = ch.mag_thr > 0.f ? 1 : 0;
  figures[0] = ch.price.rms; figures[1] = ch.price.max; figures[2] = ch.price.tail; figures[3] = ch.mag_thr;
  return rc;
}

// (the hook as it was before MLT_X_UNITS: force[12], the exact unit mask never forced)
int mlt_tier_search_run(int kind, int n, float tolerance, float max_frac, const int *force,
                        int (*price_cb)(void *user, unsigned w2_units, unsigned x_units, int rounding, float *out3), void *user, int *result, float *figures) {
  return mlt_tier_search_run_n(kind, n, tolerance, max_frac, force, 12, price_cb, user, result, figures);
}

int mlt_arithmetic(mlt_ctx *ctx, int size, mlt_arith_info *out) {
  if (!ctx || !out) return MLT_ERR_ARG;
  // the caller says how large ITS struct is; only that much is written (a later, longer mlt_arith_info cannot overrun an older caller)
  if (out->struct_size < offsetof(mlt_arith_info, mag_guard_thr)) { ctx->err = "mlt_arith_info.struct_size does not cover the ABI-4 fields"; return MLT_ERR_ARG; }
  SizeState *st;
  int rc = check_size(ctx, size, &st);
  if (rc) return rc;
  out->exact = st->exact ? 1 : st->lite ? 5 : st->x_units ? 4 : st->w2 ? (st->w2_units != 0xFFu ? 3 : 2) : 0;
  out->w2_stages = st->w2 ? (int32_t)st->w2_mask : 0;
  out->x_stages = st->exact ? 0 : (int32_t)st->x_mask;
  out->w2_units = st->w2 ? (int32_t)st->w2_units : 0;
  out->x_units = st->exact ? 0 : (int32_t)st->x_units;
  out->rounding = st->model.rounding;
  out->guard_margin = (!st->exact && st->margin_guard) ? st->guard_margin : 0.f;
  out->calibrated = st->calibrated ? 1 : 0;
  out->calib_rms = st->calib_rms; out->calib_max = st->calib_max;
  out->flat_guard = (!st->exact && st->flat_guard) ? 1 : 0;
  out->decision_guard = (!st->exact && st->margin_guard) ? 1 : 0;
  out->guard_reruns = st->reruns;
  out->calib_cus = st->calib_cus; out->calib_caller_cus = st->calib_caller_cus;
  if (out->struct_size >= sizeof(mlt_arith_info)) {  // round 6 fields: written only into a struct that has them
    out->mag_guard_thr = st->exact ? 0.f : st->mag_thr;
    out->mag_guard_flagged = st->exact ? 0.f : st->mag_flag;
    out->mag_guard_kind = st->exact ? 0 : st->mag_kind;
  }
  return MLT_OK;
}

#pragma GCC visibility pop
}  // extern "C"
