// mlt_tail_kernels.inc -- heads + argmax and the parity-guard kernels; part of mlt_kernels.hip (one translation unit).
// ---------------------------------------------------------------------------------------------
// Heads + argmax (arch:282-297, EncCu.cpp:913-921).  One workgroup per CU; fp32 throughout.
// feat = (sum of the GAP partial sums written by the stage's last conv) / HW
// logits_k = W_k . [feat (C floats), poc, qp] + b_k ; split = first maximal index (torch.argmax).
// Every class of a head runs the identical operation sequence, so identical rows tie exactly.
// Each piece that more than one kernel runs is ONE device function here: gap_features (a head's features), head_decision / head_candidates (a head's argmax,
// confidence, margin / candidate set), decision_tail (split mode under the gate + record of one (CU, point)), max_magnitude, and guard_rule -- the parity guards'
// selection rule, stated once.  heads_kernel<DEC> / heads_cand_kernel (heads_body) run them per CU, sweep_heads_kernel per (CU, point); guard_select_kernel runs
// guard_rule on logits read back from memory.
// ---------------------------------------------------------------------------------------------
// Decision of one head from its K logits: first-max argmax (torch.argmax), top-1 minus top-2 logit (margin_guard's scan), and the
// softmax probability of the argmax -- fp32, max-subtracted, the full-precision expf, every class through the same operations and summed in class order, so tied
// rows give tied probabilities (the argmax's own term is expf(0) = 1).  A NaN logit gives a NaN confidence.
__device__ __forceinline__ void head_decision(const float *l, int K, int &best, float &conf, float &margin) {
  best = 0;
  for (int k = 1; k < K; ++k)
    if (l[k] > l[best]) best = k;
  float t1 = -3.4e38f, t2 = -3.4e38f;
  for (int c = 0; c < K; ++c) {
    if (l[c] > t1) { t2 = t1; t1 = l[c]; } else if (l[c] > t2) t2 = l[c];
  }
  margin = t1 - t2;
  const float mx = l[best];
  float sum = 0.f;
  for (int k = 0; k < K; ++k) sum += expf(l[k] - mx);
  conf = 1.f / sum;
}

// The decision guard's rule on one head's K logits: the top-2 margin (head_decision's scan) is not >= thr, or a logit is NaN.  The NaN needs its own test: a NaN
// loses both comparisons of the scan, which then reports the margin of the OTHER classes, and !(t1 - t2 >= thr) alone catches only a head whose logits are ALL
// NaN.  (guard_rule's decision guard.)
__device__ __forceinline__ bool margin_guard(const float *l, int K, float thr) {
  float t1 = -3.4e38f, t2 = -3.4e38f;
  bool nan = false;
  for (int c = 0; c < K; ++c) {
    nan = nan || l[c] != l[c];
    if (l[c] > t1) { t2 = t1; t1 = l[c]; } else if (l[c] > t2) t2 = l[c];
  }
  return nan || !(t1 - t2 >= thr);
}

// Candidate set of one head from its K <= MLT_MAX_CAND_K logits, the counterpart of head_decision (include/mltcnn.h: mlt_candidates states the semantics):
// classes ranked by logit, descending, equal logits in class order (an insertion sort by adjacent exchanges on registers: every index is a compile-time constant
// after unrolling, nothing lives in scratch); the fp32 softmax of every class -- the operations of head_decision, so prob[argmax] is its confidence bit for bit --
// prefix sums in rank order; the shortest prefix that reaches `coverage` is kept, every class when that needs more than max_modes > 0 of them or a logit is NaN.
// flag (band > 0: the candidate guard): a proper prefix sum lies within `band` of the coverage, or classes are dropped over a logit gap below gap_thr -- in the
// !(x >= y) form, so a NaN flags.
__device__ __forceinline__ void head_candidates(const float *l, int K, float coverage, int max_modes, float band, float gap_thr, CandRec &r, bool &flag) {
  int best = 0;
  for (int k = 1; k < K; ++k)
    if (l[k] > l[best]) best = k;
  const float mx = l[best];
  float sum = 0.f;
  for (int k = 0; k < K; ++k) sum += expf(l[k] - mx);
  float key[MLT_MAX_CAND_K], pr[MLT_MAX_CAND_K];
  int id[MLT_MAX_CAND_K];
  bool nan = false;
#pragma unroll
  for (int k = 0; k < MLT_MAX_CAND_K; ++k) {
    const bool in = k < K;
    const float v = l[in ? k : 0];
    nan = nan || (in && v != v);
    key[k] = in ? v : -__builtin_inff();   // (padding never moves up: nothing is below it, and equal keys keep their order)
    id[k] = in ? k : -1;
    pr[k] = in ? expf(v - mx) / sum : 0.f;
    r.prob[k] = pr[k];
  }
#pragma unroll
  for (int i = 1; i < MLT_MAX_CAND_K; ++i) {
#pragma unroll
    for (int j = i; j > 0; --j) {
      const bool up = key[j] > key[j - 1];
      const float tk = key[j], tp = pr[j];
      const int ti = id[j];
      key[j] = up ? key[j - 1] : tk; pr[j] = up ? pr[j - 1] : tp; id[j] = up ? id[j - 1] : ti;
      key[j - 1] = up ? tk : key[j - 1]; pr[j - 1] = up ? tp : pr[j - 1]; id[j - 1] = up ? ti : id[j - 1];
    }
  }
  float cum = 0.f;
  int n = K;
  bool found = false, near = false;
#pragma unroll
  for (int rk = 0; rk < MLT_MAX_CAND_K; ++rk) {
    if (rk < K) {
      cum += pr[rk];
      if (!found && cum >= coverage) { n = rk + 1; found = true; }
      if (rk < K - 1) near = near || !(fabsf(cum - coverage) >= band);
    }
  }
  const int kept = (nan || (max_modes > 0 && n > max_modes)) ? K : n;
  uint32_t mask = 0;
  float gap = 3.4e38f;   // (nothing dropped: no boundary)
#pragma unroll
  for (int rk = 0; rk < MLT_MAX_CAND_K; ++rk) {
    if (rk < kept) mask |= 1u << (nan ? rk : id[rk]);
    if (rk + 1 < MLT_MAX_CAND_K && rk + 1 == kept && kept < K) gap = key[rk] - key[rk + 1];
  }
  r.mask = mask;
  r.count = kept;
#pragma unroll
  for (int rk = 0; rk < MLT_MAX_CAND_K; ++rk) r.order[rk] = (int8_t)(rk < K ? (nan ? rk : id[rk]) : -1);   // (a NaN row is listed in class order)
  r.order[6] = r.order[7] = -1;
  flag = band > 0.f && (near || !(gap >= gap_thr));
}

// The magnitude guard's statistic of a CU: the largest of its logits' sums of |w_ck feat_k| (a NaN sticks).
__device__ __forceinline__ float max_magnitude(const float *lgm, int n_logits) {
  float mag = 0.f;
  for (int k = 0; k < n_logits; ++k) mag = !(lgm[k] <= mag) ? lgm[k] : mag;
  return mag;
}

// THE selection rule of the parity guards (mlt_kernels.h: GuardRule states it in words): whether one CU is re-evaluated with the exact arithmetic.  Every
// floating-point comparison is in the negated !(x >= y) form, so a NaN -- logit, confidence or magnitude -- flags.  flat_on / flat: the CU's flat-content statistic (off: no
// flat guard); l, K: the decision head's logits (NULL: the decision guard and what rides on it are off); dec_on, conf, min_conf: the head's confidence and the
// gate it met (dec_on false: the launch computed neither records nor gate); cflag: head_candidates' flag (false where no candidate set was computed); mag: the
// CU's max_magnitude (0 where there is none: never above a threshold).  Called by the tail of the heads kernels, by sweep_heads_kernel per point and by
// guard_select_kernel; what follows the verdict (append, ballot, scan) is the caller's.
__device__ __forceinline__ bool guard_rule(const GuardRule &r, bool flat_on, int flat, const float *l, int K, bool dec_on, float conf, float min_conf, bool cflag, float mag) {
  bool s = flat_on && ((flat >> MLT_FLAT_EXACT_SHIFT) >= r.flat_thr || (flat & 0xFFFF) >= r.near_thr);
  if (l && r.margin > 0.f) {
    s = s || margin_guard(l, K, r.margin);
    if (dec_on && r.conf_band > 0.f) s = s || !(fabsf(conf - min_conf) >= r.conf_band);   // the gate guard (mlt_kernels.h: MLT_CONF_BAND_FRAC)
    s = s || cflag;   // the candidate guard (head_candidates: off unless cand_band > 0)
  }
  if (r.mag_thr > 0.f) s = s || !(mag <= r.mag_thr);
  return s;
}

// GAP features of head hd of CU n, one thread per channel: the partial sums of the stage's last conv added in slot order (eight loads in flight), / (float)hw.
__device__ __forceinline__ void gap_features(const HeadArgs &a, int hd, int n, int tid, float *feat) {
  const int C = a.c[hd], slots = a.slots[hd];
  if (tid < C) {
    const float *g = a.gap[hd] + (size_t)n * slots * C + tid;
    float s = 0.f;
    for (int i = 0; i < slots; i += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = i + u < slots ? g[(size_t)(i + u) * C] : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i + u < slots) s += v[u];
    }
    feat[tid] = s / (float)a.hw[hd];
  }
}

// Decision tail of one (CU, point), one thread: first-max argmax of the decision head's logits l; with dec_on the head's confidence (conf, else 0), the gate
// (a NaN confidence gates) and -- dec != NULL -- the record, from the point's per-head rows hmode / hconf / hmarg (head_decision).  Returns the split mode.
__device__ __forceinline__ int decision_tail(const HeadArgs &a, const float *l, bool dec_on, const int *hmode, const float *hconf, const float *hmarg, DecisionRec *dec, float &conf) {
  int best = 0;
  for (int k = 1; k < a.classes[a.decision_head]; ++k)
    if (l[k] > l[best]) best = k;
  int out = best;
  conf = 0.f;
  if (dec_on) {
    conf = hconf[a.decision_head];
    if (a.min_conf > 0.f) out = conf >= a.min_conf ? best : -1;
    if (dec) {
      DecisionRec r;
      r.split_mode = out; r.raw_mode = best; r.confidence = conf; r.margin = hmarg[a.decision_head];
#pragma unroll
      for (int hd = 0; hd < MLT_MAX_HEADS_K; ++hd) {
        r.level_mode[hd] = hd < a.n_heads ? hmode[hd] : -1;
        r.level_conf[hd] = hd < a.n_heads ? hconf[hd] : 0.f;
      }
      *dec = r;
    }
  }
  return out;
}

// DEC: the instantiation that also computes the decision records / applies the confidence gate (HeadArgs.dec != NULL or min_conf > 0: mlt_launch_heads picks it);
// <false> is the kernel as it was before records existed -- launches that want neither run exactly that code.  CAND: the body of heads_cand_kernel, which also
// computes the candidate records and the candidate guard (HeadArgs.cand != NULL or a policy other than (0, 0)); heads_kernel<DEC> is the body without them.
template <bool DEC, bool CAND>
__device__ __forceinline__ void heads_body(const HeadArgs &a) {
  __shared__ float feat[MLT_MAX_HEADS_K][256 + 2];
  __shared__ float lg[MLT_MAX_LOGITS_K];
  __shared__ int hmode[MLT_MAX_HEADS_K];      // per head: argmax, its softmax probability, top-2 margin (only when records or the gate are wanted)
  __shared__ float hconf[MLT_MAX_HEADS_K], hmarg[MLT_MAX_HEADS_K];
  __shared__ float lgm[MLT_MAX_LOGITS_K];   // sum_k |w_ck feat_k| per logit (the magnitude guard's statistic)
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float fpoc = (float)a.poc[n], fqp = (float)a.qp[n];  // EncCu.cpp:881-882 (int -> float, exact)
  // GAP features of ALL heads first (one barrier instead of two per head: this kernel is pure latency, and it is a visible share of the one-CU-per-call path).
  for (int hd = 0; hd < a.n_heads; ++hd) {
    gap_features(a, hd, n, tid, feat[hd]);
    if (tid == 0) { feat[hd][a.c[hd]] = fpoc; feat[hd][a.c[hd] + 1] = fqp; }
  }
  __syncthreads();
  int lo = 0;
  for (int hd = 0; hd < a.n_heads; ++hd) {
    const int C = a.c[hd], K = a.classes[hd];
    for (int k = wave; k < K; k += 4) {
      const float *w = a.w[hd] + (size_t)k * (C + 2);
      float s = 0.f, m = 0.f;
      for (int i = lane; i < C + 2; i += 64) {
        s = __builtin_fmaf(w[i], feat[hd][i], s);   // (the contraction hipcc applies to s += w * f by default, spelt out)
        if (i < C) m += fabsf(w[i] * feat[hd][i]);  // (the features only: poc and qp are exact integers, no rounding error rides on them)
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) { s += __shfl_down(s, off, 64); m += __shfl_down(m, off, 64); }
      if (lane == 0) { lg[lo + k] = s + a.b[hd][k]; lgm[lo + k] = m; }
    }
    lo += K;
  }
  __syncthreads();
  if (tid < lo && a.logits) a.logits[(size_t)n * lo + tid] = lg[tid];
  if constexpr (DEC) {   // one thread per head
    if (tid < a.n_heads) {
      int o = 0;
      for (int hd = 0; hd < tid; ++hd) o += a.classes[hd];
      int bm; float cf, mg;
      head_decision(lg + o, a.classes[tid], bm, cf, mg);
      hmode[tid] = bm; hconf[tid] = cf; hmarg[tid] = mg;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int off = 0;
    for (int hd = 0; hd < a.decision_head; ++hd) off += a.classes[hd];
    float conf;
    const int out = decision_tail(a, lg + off, DEC, hmode, hconf, hmarg, (DEC && a.dec) ? a.dec + n : nullptr, conf);
    bool cflag = false;
    if constexpr (CAND) {
      CandRec cr;
      head_candidates(lg + off, a.classes[a.decision_head], a.cand_cov, a.cand_max, a.rule.cand_band, a.rule.margin, cr, cflag);
      if (a.cand) a.cand[n] = cr;
    }
    if (!DEC || a.split) a.split[n] = out;   // (only a launch that writes records may come without a split buffer)
    float mag = 0.f;
    if (a.mag || a.rule.mag_thr > 0.f) {
      mag = max_magnitude(lgm, lo);
      if (a.mag) a.mag[n] = mag;
    }
    if (a.g_count && (n == 0 || a.g_next)) {  // the selection: mlt_predict's one-CU launches, and every launch of a slot with a counter pair (g_next)
      int flat = 0;
      if (a.g_flat) { flat = a.g_flat[n]; a.g_flat[n] = 0; }   // consume-and-clear
      const bool s = guard_rule(a.rule, a.g_flat != nullptr, flat, lg + off, a.classes[a.decision_head], DEC, conf, a.min_conf, cflag, mag);
      if (a.g_next) {   // unordered append to a count that was zero on entry; workgroup 0 re-arms the slot's other counter for the next launch
        if (n == 0) a.g_next[0] = 0;
        if (s) a.g_idx[atomicAdd(a.g_count, 1)] = n;
      } else {
        a.g_idx[0] = 0;
        a.g_count[0] = s ? 1 : 0;
      }
    }
  }
}

template <bool DEC>
__global__ __launch_bounds__(256) void heads_kernel(const HeadArgs a) { heads_body<DEC, false>(a); }

// Records, gate and candidate sets: launched only when a candidate buffer or a candidate policy is present (mlt_launch_heads).
__global__ __launch_bounds__(256) void heads_cand_kernel(const HeadArgs a) { heads_body<true, true>(a); }

// QP sweep (HeadSweepArgs): the heads of ONE pass under n_qps values of qp -- slab q holds what heads_kernel / heads_cand_kernel give with every qp[i] = qps[q],
// bit for bit.  qp enters a logit as the LAST element of one lane's fmaf chain (index C + 1 of [feat, poc, qp]: lane (C + 1) & 63), so the per-lane partial sums
// over [feat, poc] are computed once per (head, class) with heads_body's chain; a point adds its one fmaf in that lane and repeats the shuffle tree and the bias.
// The magnitude statistic does not see qp: once.  The tails run on one thread per (point, head) -- head_decision -- and one per point -- decision_tail, the
// candidate set, guard_rule: the points of wave 0 vote the CU's mask.  Fix-up launches (sa.fix_idx) write only the masked points.
// a.qp != NULL: CU n's point q is qps[q] + a.qp[n] -- added as integers before the one conversion, so the slab holds the bytes of a CU whose qp is that sum.
__global__ __launch_bounds__(256) void sweep_heads_kernel(const HeadSweepArgs sa) {
  const HeadArgs &a = sa.h;
  __shared__ float feat[MLT_MAX_HEADS_K][256 + 2];
  __shared__ float lg[MLT_SWEEP_MAX_QPS_K][MLT_MAX_LOGITS_K];
  __shared__ int hmode[MLT_SWEEP_MAX_QPS_K][MLT_MAX_HEADS_K];
  __shared__ float hconf[MLT_SWEEP_MAX_QPS_K][MLT_MAX_HEADS_K], hmarg[MLT_SWEEP_MAX_QPS_K][MLT_MAX_HEADS_K];
  __shared__ float lgm[MLT_MAX_LOGITS_K];
  __shared__ int sflat;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, Q = sa.n_qps;
  const int row = sa.fix_idx ? sa.fix_idx[n] : n;
  const uint32_t all = Q >= 32 ? 0xFFFFFFFFu : (1u << Q) - 1u;
  const uint32_t wr = sa.fix_idx ? sa.mask[row] & all : all;   // the points this workgroup writes
  const bool select = !sa.fix_idx && a.g_count && a.g_next;
  const float fpoc = (float)a.poc[n];
  const int qp_off = a.qp ? a.qp[n] : 0;
  for (int hd = 0; hd < a.n_heads; ++hd) {
    gap_features(a, hd, n, tid, feat[hd]);
    if (tid == 0) feat[hd][a.c[hd]] = fpoc;   // (qp: per point, below)
  }
  if (tid == 0 && select && a.g_flat) { sflat = a.g_flat[n]; a.g_flat[n] = 0; }   // consume-and-clear, once for all points
  __syncthreads();
  int lo = 0;
  for (int hd = 0; hd < a.n_heads; ++hd) {
    const int C = a.c[hd], K = a.classes[hd];
    for (int k = wave; k < K; k += 4) {
      const float *w = a.w[hd] + (size_t)k * (C + 2);
      float s = 0.f, m = 0.f;
      for (int i = lane; i < C + 1; i += 64) {
        s = __builtin_fmaf(w[i], feat[hd][i], s);
        if (i < C) m += fabsf(w[i] * feat[hd][i]);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) m += __shfl_down(m, off, 64);
      const bool mine = lane == ((C + 1) & 63);
      const float wq = w[C + 1], bk = a.b[hd][k];
      for (int q = 0; q < Q; ++q) {
        float sq = mine ? __builtin_fmaf(wq, (float)(sa.qps[q] + qp_off), s) : s;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sq += __shfl_down(sq, off, 64);
        if (lane == 0) lg[q][lo + k] = sq + bk;
      }
      if (lane == 0) lgm[lo + k] = m;
    }
    lo += K;
  }
  __syncthreads();
  if (a.logits)
    for (int t = tid; t < Q * lo; t += 256) {
      const int q = t / lo, e = t - q * lo;
      if ((wr >> q) & 1u) a.logits[((size_t)q * sa.slab + row) * lo + e] = lg[q][e];
    }
  const bool cand_on = a.cand || a.cand_cov > 0.f || a.cand_max > 0;   // mlt_launch_heads' choice of heads_cand_kernel ...
  const bool dec_on = cand_on || a.dec || a.min_conf > 0.f;           // ... and of heads_kernel<true>
  if (dec_on) {   // one thread per (point, head)
    if (tid < Q * a.n_heads) {
      const int q = tid / a.n_heads, hd = tid - q * a.n_heads;
      int o = 0;
      for (int h = 0; h < hd; ++h) o += a.classes[h];
      int bm; float cf, mg;
      head_decision(lg[q] + o, a.classes[hd], bm, cf, mg);
      hmode[q][hd] = bm; hconf[q][hd] = cf; hmarg[q][hd] = mg;
    }
    __syncthreads();
  }
  if (wave == 0) {   // one thread per point
    bool s = false;
    if (tid < Q) {
      const int q = tid;
      const bool wq_on = (wr >> q) & 1u;
      const size_t dst = (size_t)q * sa.slab + row;
      const float *l = lg[q];
      int off = 0;
      for (int hd = 0; hd < a.decision_head; ++hd) off += a.classes[hd];
      float conf;
      const int out = decision_tail(a, l + off, dec_on, hmode[q], hconf[q], hmarg[q], (a.dec && wq_on) ? a.dec + dst : nullptr, conf);
      bool cflag = false;
      if (cand_on) {
        CandRec cr;
        head_candidates(l + off, a.classes[a.decision_head], a.cand_cov, a.cand_max, a.rule.cand_band, a.rule.margin, cr, cflag);
        if (a.cand && wq_on) a.cand[dst] = cr;
      }
      if (a.split && wq_on) a.split[dst] = out;
      if (select)   // this CU under qps[q]
        s = guard_rule(a.rule, a.g_flat != nullptr, a.g_flat ? sflat : 0, l + off, a.classes[a.decision_head], dec_on, conf, a.min_conf, cflag,
                       a.rule.mag_thr > 0.f ? max_magnitude(lgm, lo) : 0.f);
    }
    const uint32_t mask = (uint32_t)__ballot(s) & all & (sa.active ? sa.active[n] : 0xFFFFFFFFu);   // (tree sweeps: only the points whose tree holds this CU)
    if (tid == 0 && select) {
      sa.mask[n] = mask;
      if (n == 0) a.g_next[0] = 0;   // re-arm the slot's other counter
      if (mask) a.g_idx[atomicAdd(a.g_count, 1)] = n;
    }
  }
}


// ---------------------------------------------------------------------------------------------
// Parity guard of the fast arithmetic.  fp16 rounding noise is averaged away by the global pooling only where
// neighbouring pixels DIFFER: on exactly-constant areas every pixel carries the same rounding error (measured: a constant
// 128x128 CU reaches |dlogit| 1.3e-3, ordinary content 2-7e-4), and nearly so where they differ by a few LSB (dither, low
// contrast, gentle ramps: rms 1.2-1.5x the textured one, measured per content class in round 3).  flat_stat_kernel counts,
// per CU, the aligned 4-pixel quads whose org values and whose |org - pred| values each span <= MLT_FLAT_RANGE; the selection (guard_rule above: as the tail of the
// heads kernels, or as guard_select_kernel) lists the CUs whose count reaches the threshold and those the other guards flag; the host runtime re-evaluates exactly
// those CUs with the exact (hi, lo) arithmetic (gather -> exact network -> scatter).  Integer statistics: deterministic.
// ---------------------------------------------------------------------------------------------
template <bool ALIGNED>
__global__ __launch_bounds__(256) void flat_stat_kernel(const FlatStatArgs a) {
  __shared__ int wsum[4];
  const int n = blockIdx.x, tid = threadIdx.x, S = 1 << a.s_l, qrow_l = a.s_l - 2;  // quads per row = S / 4
  const int nquads = S << qrow_l;
  const int16_t *o = a.org + (size_t)n * a.org_cu_stride, *p = a.pred + (size_t)n * a.pred_cu_stride;
  int cnt = 0;
  for (int q = tid; q < nquads; q += 256) {
    const int y = q >> qrow_l, x = (q & ((1 << qrow_l) - 1)) * 4;
    int16_t vo[4], vp[4];
    if constexpr (ALIGNED) {
      typedef uint32_t uint2v __attribute__((ext_vector_type(2)));
      const uint2v wo = *(const uint2v *)(o + (size_t)y * a.org_row_stride + x), wp = *(const uint2v *)(p + (size_t)y * a.pred_row_stride + x);
#pragma unroll
      for (int j = 0; j < 4; ++j) { vo[j] = (int16_t)(wo[j >> 1] >> (16 * (j & 1))); vp[j] = (int16_t)(wp[j >> 1] >> (16 * (j & 1))); }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) { vo[j] = o[(size_t)y * a.org_row_stride + x + j]; vp[j] = p[(size_t)y * a.pred_row_stride + x + j]; }
    }
    // what the network sees (uint16 cast, absdiff, clip)
    const int fb = quad_flat_bits(prep_pair(vo[0], vp[0]), prep_pair(vo[1], vp[1]), prep_pair(vo[2], vp[2]), prep_pair(vo[3], vp[3]));
    cnt += (fb & 1) + ((fb >> 1) << MLT_FLAT_EXACT_SHIFT);  // (<= 4096 quads per CU: the two 16-bit fields cannot carry into each other)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) a.flat[n] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup; ascending index list by a block-wide prefix scan (deterministic order)
__global__ __launch_bounds__(1024) void guard_select_kernel(const GuardSelectArgs a) {
  __shared__ int part[1024];
  const int tid = threadIdx.x, per = (a.n + 1023) / 1024, lo = tid * per, hi = lo + per < a.n ? lo + per : a.n;
  auto selected = [&](int i) -> bool {
    const float *l = a.logits ? a.logits + (size_t)i * a.n_logits + a.head_off : nullptr;
    float conf = 0.f;
    bool cflag = false;
    if (l && a.rule.margin > 0.f) {   // what the heads kernel had at hand, recomputed from the logits it left in memory (head_decision, head_candidates: its own functions)
      if (a.rule.conf_band > 0.f) { int bm; float mg; head_decision(l, a.head_classes, bm, conf, mg); }
      if (a.rule.cand_band > 0.f) { CandRec cr; head_candidates(l, a.head_classes, a.cand_cov, a.cand_max, a.rule.cand_band, a.rule.margin, cr, cflag); }
    }
    return guard_rule(a.rule, a.flat != nullptr, a.flat ? a.flat[i] : 0, l, a.head_classes, true, conf, a.min_conf, cflag, a.mag ? a.mag[i] : 0.f);
  };
  int c = 0;
  for (int i = lo; i < hi; ++i) c += selected(i) ? 1 : 0;
  part[tid] = c;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // inclusive Hillis-Steele scan
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int pos = part[tid] - c;
  for (int i = lo; i < hi; ++i)
    if (selected(i)) a.idx[pos++] = i;
  if (tid == 1023) *a.count = part[1023];
}

// grid (k, 2): plane blockIdx.y of the blockIdx.x-th selected CU -> dense staging
__global__ __launch_bounds__(256) void guard_gather_kernel(const GuardGatherArgs a) {
  const int j = blockIdx.x, src = a.idx[j], S = 1 << a.s_l, tid = threadIdx.x;
  const bool is_pred = blockIdx.y == 1;
  const int16_t *s = is_pred ? a.pred + (size_t)src * a.pred_cu_stride : a.org + (size_t)src * a.org_cu_stride;
  const long rs = is_pred ? a.pred_row_stride : a.org_row_stride;
  int16_t *d = (is_pred ? a.g_pred : a.g_org) + ((size_t)j << (2 * a.s_l));
  for (int i = tid; i < S * S; i += 256) d[i] = s[(size_t)(i >> a.s_l) * rs + (i & (S - 1))];
  if (tid == 0 && !is_pred) { a.g_poc[j] = a.poc[src]; a.g_qp[j] = a.qp[src]; }
}

__global__ __launch_bounds__(256) void guard_scatter_kernel(const GuardScatterArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x, j = t / (a.n_logits + 1), e = t - j * (a.n_logits + 1);
  if (j >= a.k) return;
  const int dst = a.idx[j];
  if (e == a.n_logits) {
    if (a.split) a.split[dst] = a.g_split[j];
    if (a.dec) a.dec[dst] = a.g_dec[j];
    if (a.cand) a.cand[dst] = a.g_cand[j];
  } else if (a.logits) a.logits[(size_t)dst * a.n_logits + e] = a.g_logits[(size_t)j * a.n_logits + e];
}

