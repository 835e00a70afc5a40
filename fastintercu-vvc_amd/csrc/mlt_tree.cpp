// mlt_tree.cpp -- partition trees of a picture (include/mltcnn.h): mlt_predict_tree, mlt_predict_trees, mlt_predict_tree_sweep, mlt_predict_trees_sweep, mlt_tree_roots,
// mlt_tree_max_nodes.
//
// Both calls run ONE descent (descend below) over the trees of P picture pairs of one geometry; mlt_predict_tree is P = 1.  Per level: the network on the level's
// nodes -- predict_at_chunks (mlt_pictures.cpp) on the slice of the device-resident position list that IS the level, over all pictures, so launches, guards and
// exact re-runs are mlt_predict_at's and so is every result -- then tree_expand_kernel (mlt_tree_kernels.inc): the level's decisions into its node records, the next
// level's nodes and positions behind them, the next level's count; tree_raster_kernel paints the level's leaves into the maps; one 4-byte count comes back.  Nodes,
// positions and the per-node logits / records are indexed by NODE in one device arena, LEVEL-major (picture 0's segment of a level, picture 1's, ...), so a level's
// arrays are slices of the arena's.  One picture's arena is already in the contract's order and mlt_predict_tree ends in a handful of D2H copies;
// mlt_predict_trees lets tree_pack_kernel permute into the picture-major order of its contract first, then one D2H copy per requested array.
// mlt_predict_tree_sweep (one pair, several qp) and mlt_predict_trees_sweep (several pairs, several qp each) run ONE descent of their own over the UNION of every
// entry's trees: descend_sweep below, P = 1 for the former; rank and pack kernels cut the union into one slice per (entry, point): sweep_results.
// What the two descents and the four entry points share is written once: the checks of the entries and of node_cap (check_tree_entries, check_node_cap), the
// call's device tables (upload_tree_tables), a level's count coming back (read_level_count) and the copy of a packed result to the caller (copy_packed).  The
// gather of a chunk is mlt_pictures.cpp's enqueue_gather in both descents.
#include "mlt_runtime.h"

namespace {

const int kRowLogits = Lay::TreeArena::kRow;   // floats the arena reserves per node (a level's logits are dense [n][n_logits] from the level's first row)

bool tree_sizes(int &top, int &mn) {
  if (top == 0) top = 128;
  if (mn == 0) mn = 16;
  return size_index(top) >= 0 && size_index(mn) >= 0 && mn <= top;
}
bool dims_ok(int w, int h) { return w >= kPictureMinDim && h >= kPictureMinDim && w <= kPictureMaxDim && h <= kPictureMaxDim; }

// roots of level S under top: the whole grid at top; below, the complete S-aligned CUs right of / under the area the complete 2S-aligned blocks cover
int roots_of(int w, int h, int top, int S, int32_t *xy, int cap) {
  if (S == top) return mlt_grid_positions(w, h, S, xy, cap);
  const int cols = w / S, rows = h / S, P = 2 * S, w2 = w / P * P, h2 = h / P * P;
  long long count = 0;
  for (int r = 0; r < rows; ++r) {
    const int y = r * S;
    for (int c = y < h2 ? w2 / S : 0; c < cols; ++c) {
      if (xy && count < cap) { xy[2 * count] = c * S; xy[2 * count + 1] = y; }
      ++count;
    }
  }
  return (int)count;
}

// the levels of a tree call: every size top..min loaded, every descend mask inside its decision head (`who` opens the messages)
struct TreeLevels { int top, mn, L; SizeState *st[4]; uint32_t mask[4]; };
int tree_levels(mlt_ctx *ctx, const char *who, const mlt_tree_config *cfg, TreeLevels &lv) {
  lv.top = cfg->top_size; lv.mn = cfg->min_size; lv.L = 0;
  if (!tree_sizes(lv.top, lv.mn)) { ctx->err = std::string(who) + ": top_size / min_size must be 128, 64, 32 or 16 with min_size <= top_size"; return MLT_ERR_ARG; }
  int rc;
  for (int S = lv.top; S >= lv.mn; S >>= 1, ++lv.L) {
    if ((rc = check_size(ctx, S, &lv.st[lv.L]))) return rc;
    const uint32_t m = cfg->descend_mask[size_index(S)];
    lv.mask[lv.L] = m ? m : 1u << 1;
    const int K = lv.st[lv.L]->head_classes();
    if (lv.mask[lv.L] >> K) {
      char msg[160];
      std::snprintf(msg, sizeof msg, "%s: descend_mask of size %d names a class at or above the %d classes of its decision head", who, S, K);
      ctx->err = msg;
      return MLT_ERR_ARG;
    }
  }
  return MLT_OK;
}

// the roots of every level, level after level: roots[2 * off[l] ..], n[l] of them
struct TreeRoots { std::vector<int32_t> xy; int off[4], n[4]; };
void tree_roots_of(int W, int H, int top, int L, TreeRoots &r) {
  for (int l = 0, S = top; l < L; ++l, S >>= 1) {
    r.off[l] = (int)(r.xy.size() / 2);
    r.n[l] = roots_of(W, H, top, S, nullptr, 0);
    r.xy.resize(r.xy.size() + 2 * (size_t)r.n[l]);
    if (r.n[l]) (void)roots_of(W, H, top, S, r.xy.data() + 2 * (size_t)r.off[l], r.n[l]);
  }
}

// the entries of a several-pair call: every pair given and of this context, one geometry over the call; with qps: every entry's qp offset + point fits int32
int check_tree_entries(mlt_ctx *ctx, const char *who, int P, const mlt_tree_picture *pics, const int32_t *qps = nullptr, int Q = 0) {
  char msg[224];
  for (int p = 0; p < P; ++p) {
    const mlt_picture *o = pics[p].org, *q = pics[p].pred;
    if (!o || !q || !owns_picture(ctx, o) || !owns_picture(ctx, q)) {
      std::snprintf(msg, sizeof msg, "%s: entry %d: both pictures must be given and belong to this context", who, p);
      ctx->err = msg;
      return MLT_ERR_ARG;
    }
    if (o->width != q->width || o->height != q->height || o->width != pics[0].org->width || o->height != pics[0].org->height) {
      std::snprintf(msg, sizeof msg, "%s: entry %d: every picture of a call must have the width and height of entry 0's (%d x %d)", who, p, pics[0].org->width,
                    pics[0].org->height);
      ctx->err = msg;
      return MLT_ERR_ARG;
    }
    for (int k = 0; k < Q; ++k) {   // the QP of entry p under point k
      const long long qp = (long long)pics[p].qp + (long long)qps[k];
      if (qp < INT32_MIN || qp > INT32_MAX) {
        std::snprintf(msg, sizeof msg, "%s: entry %d: its qp offset %d + qps[%d] = %d does not fit int32", who, p, pics[p].qp, k, qps[k]);
        ctx->err = msg;
        return MLT_ERR_ARG;
      }
    }
  }
  return MLT_OK;
}

// node_cap against the call's trees (`factors`: its pictures, its points, both, or none for one tree) x mlt_tree_max_nodes of one W x H picture
int check_node_cap(mlt_ctx *ctx, const char *who, int node_cap, std::initializer_list<int> factors, int max_nodes, int W, int H) {
  long long cap_all = max_nodes;
  std::string times;
  for (int f : factors) { cap_all *= f; times += std::to_string(f) + " x "; }
  if (node_cap >= cap_all && cap_all <= 0x7fffffff) return MLT_OK;
  char msg[224];
  std::snprintf(msg, sizeof msg, "%s: node_cap %d is below %smlt_tree_max_nodes = %d of a %d x %d picture", who, node_cap, times.c_str(), max_nodes, W, H);
  ctx->err = msg;
  return MLT_ERR_ARG;
}

// the optional outputs of a tree call as the caller gave them (NULL: not wanted) | whether the call descends on the candidate sets
struct TreeOut { uint8_t *maps; float *logits; int logit_stride; mlt_decision *dec; mlt_candidates *cand; };
bool by_candidates(const mlt_tree_config *cfg) { return (cfg->flags & MLT_TREE_BY_CANDIDATES) != 0; }

// What either descent puts on the device before its first launch (A: its arena): the entry table of a call over several pairs -- one pair's planes, poc and qp are
// launch arguments of the gather --, the roots of every level and the 0xFF fill of the `maps` leaf maps; the pinned word the level counts come back through.
template <class Ptrs> int upload_tree_tables(mlt_ctx *ctx, const Ptrs &A, int P, const mlt_tree_picture *pics, const TreeRoots &tr, size_t maps, size_t map_bytes) {
  if (!ctx->tree_host) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->tree_host, 64, hipHostMallocDefault));
  if (P > 1) {
    std::vector<TreesEntry> entries((size_t)P);
    for (int p = 0; p < P; ++p) {
      const AtPlanes pl = AtPlanes::of(pics[p].org, pics[p].pred, 0);
      entries[(size_t)p] = TreesEntry{pl.org, pl.pred, pl.org_pitch, pl.pred_pitch, pl.org_vec ? 1 : 0, pl.pred_vec ? 1 : 0, pics[p].poc, pics[p].qp};
    }
    // (pageable sources: both copies have read them when they return)
    HIP_TRY(ctx, hipMemcpyAsync(A.entries, entries.data(), entries.size() * sizeof(TreesEntry), hipMemcpyHostToDevice, ctx->stream));
  }
  if (!tr.xy.empty()) HIP_TRY(ctx, hipMemcpyAsync(A.roots, tr.xy.data(), tr.xy.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (maps) HIP_TRY(ctx, hipMemsetAsync(A.map, 0xFF, maps * map_bytes, ctx->stream));
  return MLT_OK;
}

// The one host synchronisation of a level beside the guards': n <- how many nodes the next level has over all pictures -- its `roots` and four per descending
// node, `room` at most.
template <class Ptrs> int read_level_count(mlt_ctx *ctx, const char *who, const Ptrs &A, long long roots, long long room, int &n) {
  HIP_TRY(ctx, hipMemcpyAsync(ctx->tree_host, A.count, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  n = ctx->tree_host[0];
  if (n < roots || ((n - roots) & 3) || n > room) { ctx->err = std::string(who) + ": bad node count from the device"; return MLT_ERR_HIP; }
  return MLT_OK;
}

// The packed output of an arena (A.o_*: `total` nodes, picture- or slice-major) and its `maps` leaf maps to the caller, enqueued: nodes, whole zero-padded logits
// rows, records, candidate records, maps.
template <class Ptrs> int copy_packed(mlt_ctx *ctx, const Ptrs &A, int total, size_t maps, size_t map_bytes, mlt_tree_node *nodes, const TreeOut &out) {
  if (total) {
    HIP_TRY(ctx, hipMemcpyAsync(nodes, A.o_nodes, (size_t)total * sizeof(TreeNodeRec), hipMemcpyDeviceToHost, ctx->stream));
    if (out.logits) {
      if (out.logit_stride == kRowLogits) HIP_TRY(ctx, hipMemcpyAsync(out.logits, A.o_logits, (size_t)total * kRowLogits * 4, hipMemcpyDeviceToHost, ctx->stream));
      else HIP_TRY(ctx, hipMemcpy2DAsync(out.logits, (size_t)out.logit_stride * 4, A.o_logits, (size_t)kRowLogits * 4, (size_t)kRowLogits * 4, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (out.dec) HIP_TRY(ctx, hipMemcpyAsync(out.dec, A.o_dec, (size_t)total * sizeof(DecisionRec), hipMemcpyDeviceToHost, ctx->stream));
    if (out.cand) HIP_TRY(ctx, hipMemcpyAsync(out.cand, A.o_cand, (size_t)total * sizeof(CandRec), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (out.maps) HIP_TRY(ctx, hipMemcpyAsync(out.maps, A.map, maps * map_bytes, hipMemcpyDeviceToHost, ctx->stream));
  return MLT_OK;
}

// what a descent leaves behind: the arena, the node count over all pictures and every level's node range
struct Descent { Lay::TreeArena::Ptrs A; size_t map_bytes; int total, start[4], n[4]; };

// The descent of the trees of pics[0 .. P) (W x H each, checked by the caller) on this context's own device; everything stays in the arena, enqueued or done.
// packed: the arena also carries the entry table and tree_pack_kernel's picture-major output.
int descend(mlt_ctx *ctx, const char *who, const TreeLevels &lv, int W, int H, int P, const mlt_tree_picture *pics, bool by_cand, bool packed, const TreeOut &want,
            Descent &d) {
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  const int top = lv.top, L = lv.L, max_nodes = mlt_tree_max_nodes(W, H, top, lv.mn), N = P * max_nodes;
  int rc;
  // candidate records come from the heads launch only where cand_mask can differ from 1 << raw_mode (a policy is set) or the caller asks for them
  bool want_cand[4], any_cand = false;
  for (int l = 0; l < L; ++l) any_cand = (want_cand[l] = want.cand || by_cand || lv.st[l]->cand_policy()) || any_cand;
  TreeRoots tr;
  tree_roots_of(W, H, top, L, tr);
  const int map_w = W / 16, map_h = H / 16;
  const size_t map_bytes = d.map_bytes = (size_t)map_w * map_h;
  const Lay::TreeArena arena((size_t)P, (size_t)max_nodes, tr.xy.size() / 2, map_bytes, sizeof(TreesEntry), any_cand, packed, want.logits, want.dec, want.cand);
  if ((rc = ctx->tree_dev.reserve(ctx, arena.bytes(), who))) return rc;
  const Lay::TreeArena::Ptrs A = d.A = arena.at(ctx->tree_dev.p);
  // One pair: its planes, poc and qp are launch arguments of the gather (no table lookup per item).  Several: the entry table, looked up through the nodes' pic.
  const AtPlanes planes = P == 1 ? AtPlanes::of(pics[0].org, pics[0].pred, 0) : AtPlanes{};
  if ((rc = upload_tree_tables(ctx, A, P, pics, tr, want.maps ? (size_t)P : 0, map_bytes))) return rc;
  auto expand = [&](const TreeExpandArgs &ea) -> int {
    // algorithmic bytes the host knows: the level's records and picture indices read and its node fields written, every picture's next roots written, the segment
    // table's rows (the children's count is the device's)
    PROF_HIP_TRY(ctx, "tree_expand", 0.0, (double)ea.lvl_n * (sizeof(DecisionRec) + 20) + (double)P * ea.n_next_roots * (sizeof(TreeNodeRec) + 12) + (double)P * 8,
                 mlt_launch_tree_expand(ea, ctx->stream));
    return MLT_OK;
  };
  TreeExpandArgs ea{};
  ea.nodes = A.nodes; ea.xy = A.xy; ea.pic = A.pic; ea.node_cap = N; ea.by_candidates = by_cand ? 1 : 0;
  ea.seg_start = A.seg_start; ea.seg_n = A.seg_n; ea.pack_base = A.pack_base; ea.n_pictures = P; ea.n_levels = L; ea.first_node = A.first_node;
  // the trees open: no parents, every picture's top-level roots
  ea.lvl_start = 0; ea.lvl_n = 0; ea.size = 2 * top; ea.lvl = -1;
  ea.next_roots = A.roots; ea.n_next_roots = tr.n[0]; ea.root_flags = 0; ea.count = nullptr;
  if ((rc = expand(ea))) return rc;
  int start = 0, n = P * tr.n[0];
  for (int l = 0, S = top; l < L; ++l, S >>= 1) {
    SizeState *s = lv.st[l];
    const bool last = l == L - 1;
    d.start[l] = start; d.n[l] = n;
    float *d_lg = A.logits + (size_t)start * kRowLogits;
    DecisionRec *d_dec = A.dec + start;
    CandRec *d_cand = want_cand[l] ? A.cand + start : nullptr;
    if (n > 0) {
      const AtOut out{nullptr, d_lg, (mlt_decision *)d_dec, (mlt_candidates *)d_cand};
      const int32_t *d_xy = A.xy + 2 * (size_t)start;
      const AtList list = P == 1 ? AtList::on_device(d_xy, pics[0].poc, pics[0].qp) : AtList::of_entries(d_xy, A.pic + start, (const TreesEntry *)A.entries, P);
      if ((rc = predict_at_chunks(ctx, s, planes, n, list, out))) return rc;
    }
    ea.lvl_start = start; ea.lvl_n = n; ea.size = S; ea.lvl = l;
    ea.dec = d_dec; ea.cand = d_cand; ea.logits = d_lg; ea.n_logits = s->model.n_logits;
    ea.head_off = s->head_off(); ea.head_classes = s->head_classes();
    ea.descend_mask = last ? 0u : lv.mask[l];
    ea.next_roots = last ? nullptr : A.roots + 2 * (size_t)tr.off[l + 1];
    ea.n_next_roots = last ? 0 : tr.n[l + 1];
    ea.root_flags = 1;
    ea.count = last ? nullptr : A.count;
    if ((rc = expand(ea))) return rc;
    if (n > 0 && want.maps) {
      TreeRasterArgs ra{};
      ra.nodes = A.nodes; ra.pic = A.pic; ra.lvl_start = start; ra.lvl_n = n; ra.blk_l = ilog2(S) - 4; ra.map = A.map; ra.map_bytes = map_bytes; ra.map_w = map_w; ra.map_h = map_h;
      // algorithmic bytes: every node record and picture index read once, one byte per block of a leaf written (at most the level's whole area)
      PROF_HIP_TRY(ctx, "tree_raster", 0.0, (double)n * (sizeof(TreeNodeRec) + 4 + (double)(1 << (2 * ra.blk_l))), mlt_launch_tree_raster(ra, ctx->stream));
    }
    start += n;
    if (last) break;
    if ((rc = read_level_count(ctx, who, A, (long long)P * tr.n[l + 1], (long long)N - start, n))) return rc;
  }
  d.total = start;
  return MLT_OK;
}

// The UNION descent of mlt_predict_tree_sweep (P = 1) and mlt_predict_trees_sweep: the trees of pics[0 .. P) (W x H each, checked by the caller) under qps[0 .. Q),
// every node that exists under any point of its entry evaluated once.  Per level, over ALL entries: the gather from the level's slice of the device position
// list, ONE sweep pass per chunk (run_checked_sweep: the heads under every point, slab-major straight into the arena with the level's slab stride; a node is
// flagged only under the points it is alive under), tree_expand_sweep_kernel, the leaves into the maps, one 4-byte count.  One entry: its planes and poc are
// launch arguments of the gather and qps[] are the points' QPs themselves (the caller has added the entry's offset).  Several: the entry table, looked up through
// the nodes' pic by picture_gather_multi_kernel, which also writes the chunk's per-CU poc and qp -- the entry's OFFSET, which the sweep heads add to every point.
struct SweepDescent { Lay::TreeSweepArena::Ptrs A; size_t map_bytes; int n[4], start[4], cap[4]; bool has_cand[4]; };
int descend_sweep(mlt_ctx *ctx, const char *who, const TreeLevels &lv, int W, int H, int P, const mlt_tree_picture *pics, const int32_t *qps, int Q, bool by_cand,
                  const TreeOut &want, SweepDescent &d) {
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  const int top = lv.top, L = lv.L;
  int rc;
  bool any_cand = false, all_cand = true;
  size_t lvl_cap[4] = {0, 0, 0, 0};
  for (int l = 0, S = top; l < L; ++l, S >>= 1) {
    d.has_cand[l] = want.cand || by_cand || lv.st[l]->cand_policy();   // (descend: where cand_mask can differ from 1 << raw_mode, or the caller asks)
    any_cand = any_cand || d.has_cand[l];
    all_cand = all_cand && d.has_cand[l];
    lvl_cap[l] = (size_t)(W / S) * (size_t)(H / S);
  }
  TreeRoots tr;
  tree_roots_of(W, H, top, L, tr);
  const int map_w = W / 16, map_h = H / 16;
  const size_t map_bytes = d.map_bytes = (size_t)map_w * map_h;
  // logits: the caller's, or what cand_mask is made from on the levels without candidate records
  const Lay::TreeSweepArena arena((size_t)Q, L, lvl_cap, tr.xy.size() / 2, map_bytes, want.logits || !all_cand, any_cand, want.maps != nullptr, want.logits, want.dec,
                                  want.cand, (size_t)P, sizeof(TreesEntry));
  if ((rc = ctx->tree_dev.reserve(ctx, arena.bytes(), who))) return rc;
  const Lay::TreeSweepArena::Ptrs A = d.A = arena.at(ctx->tree_dev.p);
  const int N = (int)arena.n;
  const GatherSrc src{AtPlanes::of(pics[0].org, pics[0].pred, 0), (const TreesEntry *)A.entries, P};
  if ((rc = upload_tree_tables(ctx, A, P, pics, tr, want.maps ? (size_t)P * (size_t)Q : 0, map_bytes))) return rc;
  auto expand = [&](const TreeSweepExpandArgs &ea) -> int {
    // algorithmic bytes the host knows: the level's alive masks and, under every point, its records read, its node fields written, the next roots written
    // (several entries: + a picture index per node and root, the segment table's rows)
    double bytes = (double)ea.lvl_n * ((double)Q * sizeof(DecisionRec) + 16) + (double)P * ea.n_next_roots * (sizeof(TreeNodeRec) + 24);
    if (P > 1) bytes += 4.0 * ((double)ea.lvl_n + (double)P * ea.n_next_roots) + (double)P * 8;
    PROF_HIP_TRY(ctx, "tree_expand_sweep", 0.0, bytes, mlt_launch_tree_expand_sweep(ea, ctx->stream));
    return MLT_OK;
  };
  SweepPart sw;
  sw.n_qps = Q;
  std::memcpy(sw.qps, qps, (size_t)Q * 4);
  TreeSweepExpandArgs ea{};
  ea.nodes = A.nodes; ea.xy = A.xy; ea.alive = A.alive; ea.desc = A.desc; ea.pic = A.pic; ea.seg_start = A.seg_start; ea.seg_n = A.seg_n; ea.n_pictures = P;
  ea.node_cap = N; ea.n_qps = Q; ea.by_candidates = by_cand ? 1 : 0;
  // the unions open: no parents, every entry's top-level roots
  ea.lvl_start = 0; ea.lvl_n = 0; ea.next_start = 0; ea.next_cap = (int)arena.cap[0]; ea.size = 2 * top; ea.lvl = -1;
  ea.next_roots = A.roots; ea.n_next_roots = tr.n[0]; ea.root_flags = 0; ea.count = nullptr;
  if ((rc = expand(ea))) return rc;
  int n = P * tr.n[0];
  for (int l = 0, S = top; l < L; ++l, S >>= 1) {
    SizeState *s = lv.st[l];
    const bool last = l == L - 1;
    const int start = (int)arena.off[l], nl = s->model.n_logits;
    d.start[l] = start; d.n[l] = n; d.cap[l] = (int)arena.cap[l];
    const size_t e0l = arena.slab0(l);
    DecisionRec *d_dec = A.dec + e0l;
    float *d_lg = A.logits ? A.logits + e0l * kRowLogits : nullptr;
    CandRec *d_cand = d.has_cand[l] ? A.cand + e0l : nullptr;
    sw.slab = (long)arena.cap[l];
    if (n > 0) {
      const int cap = n < ctx->chunk ? n : ctx->chunk;
      const StageSet lay(S, cap, nl, false, false);
      if ((rc = ctx->stage.reserve(ctx, lay.bytes(), "staging"))) return rc;
      const StageSet::Ptrs G = lay.at(ctx->stage.p);
      if (P == 1) HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)G.d_poc, pics[0].poc, (size_t)cap, ctx->stream));   // one poc: every chunk reads its first c entries
      for (int i0 = 0; i0 < n; i0 += cap) {
        const int c = n - i0 < cap ? n - i0 : cap;
        // the chunk's slice of the list and (several entries) of its entry indices: that launch writes the chunk's poc and qp offsets as well
        if ((rc = enqueue_gather(ctx, src, A.xy + 2 * ((size_t)start + (size_t)i0), P == 1 ? nullptr : A.pic + start + i0, G.d_org, G.d_pred, G.d_poc, G.d_qp, c, S)))
          return rc;
        sw.active = A.alive + start + i0;
        const PassIO io{Planes::dense(G.d_org, G.d_pred, S), G.d_poc, P == 1 ? nullptr : G.d_qp, nullptr, d_lg ? d_lg + (size_t)i0 * nl : nullptr, d_dec + i0,
                        d_cand ? d_cand + i0 : nullptr, sw};
        if ((rc = run_checked_sweep(ctx, *s, c, io))) return rc;   // (the stream orders this chunk's reads of the staged planes before the next chunk's gather)
      }
    }
    ea.lvl_start = start; ea.lvl_n = n; ea.next_start = last ? 0 : (int)arena.off[l + 1]; ea.next_cap = last ? 0 : (int)arena.cap[l + 1]; ea.size = S; ea.lvl = l;
    ea.dec = d_dec; ea.cand = d_cand; ea.logits = d_lg; ea.slab = sw.slab; ea.n_logits = nl; ea.head_off = s->head_off(); ea.head_classes = s->head_classes();
    ea.descend_mask = last ? 0u : lv.mask[l];
    ea.next_roots = last ? nullptr : A.roots + 2 * (size_t)tr.off[l + 1];
    ea.n_next_roots = last ? 0 : tr.n[l + 1];
    ea.root_flags = 1;
    ea.count = last ? nullptr : A.count;
    if ((rc = expand(ea))) return rc;
    if (n > 0 && want.maps) {
      TreeSweepRasterArgs ra{};
      ra.nodes = A.nodes; ra.alive = A.alive; ra.desc = A.desc; ra.pic = A.pic; ra.dec = d_dec; ra.slab = sw.slab; ra.lvl_start = start; ra.lvl_n = n; ra.blk_l = ilog2(S) - 4;
      ra.n_qps = Q; ra.n_pictures = P; ra.map = A.map; ra.map_bytes = map_bytes; ra.map_w = map_w; ra.map_h = map_h;
      // algorithmic bytes: every node record and mask pair read once, one byte per block of a leaf written under every point (at most the level's whole area each)
      PROF_HIP_TRY(ctx, "tree_sweep_raster", 0.0, (double)n * (sizeof(TreeNodeRec) + 8 + (P > 1 ? 4 : 0) + (double)Q * (1 << (2 * ra.blk_l))),
                   mlt_launch_tree_sweep_raster(ra, ctx->stream));
    }
    if (last) break;
    if ((rc = read_level_count(ctx, who, A, (long long)P * tr.n[l + 1], (long long)arena.cap[l + 1], n))) return rc;
  }
  for (int l = L; l < 4; ++l) { d.start[l] = 0; d.n[l] = 0; d.cap[l] = 0; d.has_cand[l] = false; }
  return MLT_OK;
}

// What follows a union descent: rank and pack -- one slice per (entry, point), slice p * Q + q -- then everything the caller asked for and one synchronisation.
// max_nodes: mlt_tree_max_nodes of one picture.
int sweep_results(mlt_ctx *ctx, const char *who, const TreeLevels &lv, const SweepDescent &d, int P, int Q, int max_nodes, mlt_tree_node *nodes, int32_t *first_node,
                  int32_t *union_nodes_opt, const TreeOut &out) {
  const Lay::TreeSweepArena::Ptrs &A = d.A;
  const long long cap_all = (long long)P * Q * max_nodes;
  const size_t PQ = (size_t)P * (size_t)Q;
  TreeSweepPackArgs pa{};
  pa.nodes = A.nodes; pa.alive = A.alive; pa.desc = A.desc; pa.dec = A.dec; pa.logits = A.logits; pa.cand = A.cand;
  pa.pic = A.pic; pa.seg_start = A.seg_start; pa.seg_n = A.seg_n; pa.n_pictures = P;
  pa.idx = A.idx; pa.total = A.total; pa.first_node = A.first_node; pa.union_nodes = A.union_nodes;
  pa.o_nodes = A.o_nodes; pa.o_logits = A.o_logits; pa.o_dec = A.o_dec; pa.o_cand = A.o_cand;
  pa.n_qps = Q; pa.n_levels = lv.L; pa.node_cap = P * max_nodes; pa.out_cap = (int)cap_all;
  long long un = 0;
  for (int l = 0; l < lv.L; ++l) {
    pa.lvl_start[l] = d.start[l]; pa.lvl_n[l] = d.n[l]; pa.lvl_cap[l] = d.cap[l]; pa.has_cand[l] = d.has_cand[l] ? 1 : 0;
    pa.n_logits[l] = lv.st[l]->model.n_logits; pa.head_off[l] = lv.st[l]->head_off(); pa.head_classes[l] = lv.st[l]->head_classes();
    un += d.n[l];
  }
  // algorithmic bytes: the alive mask of every union node read and its index written under every point | per (point, node) at most one node record, its slab
  // record and the requested rows and records, read and written
  const double per = 2.0 * sizeof(TreeNodeRec) + 12 + sizeof(DecisionRec) + (out.logits ? 2.0 * kRowLogits * 4 : 0) + (out.dec ? sizeof(DecisionRec) : 0) + (out.cand ? 2.0 * sizeof(CandRec) : 0);
  PROF_HIP_TRY(ctx, "tree_sweep_rank", 0.0, (double)Q * (double)un * 8, mlt_launch_tree_sweep_rank(pa, ctx->stream));
  PROF_HIP_TRY(ctx, "tree_sweep_pack", 0.0, (double)Q * (double)un * per, mlt_launch_tree_sweep_pack(pa, ctx->stream));
  // the slices' sizes first: the copies below take exactly the packed nodes (the caller's arrays stay untouched behind them)
  std::vector<int32_t> first(PQ + 1), un_l((size_t)P * 4);
  HIP_TRY(ctx, hipMemcpyAsync(first.data(), A.first_node, (PQ + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(un_l.data(), A.union_nodes, (size_t)P * 16, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const int total = first[PQ];
  bool ok = first[0] == 0 && total >= 0 && total <= cap_all;
  for (size_t s = 0; s < PQ && ok; ++s) ok = first[s + 1] >= first[s];
  if (!ok) { ctx->err = std::string(who) + ": bad node count from the device"; return MLT_ERR_HIP; }
  if (int rc = copy_packed(ctx, A, total, PQ, d.map_bytes, nodes, out)) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(first_node, first.data(), (PQ + 1) * 4);
  if (union_nodes_opt) std::memcpy(union_nodes_opt, un_l.data(), (size_t)P * 16);
  return MLT_OK;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int mlt_tree_max_nodes(int width, int height, int top_size, int min_size) {
  if (!tree_sizes(top_size, min_size) || !dims_ok(width, height)) return 0;
  long long total = 0;
  for (int S = top_size; S >= min_size; S >>= 1) total += (long long)(width / S) * (height / S);
  return total > 0x7fffffff ? 0 : (int)total;
}

int mlt_tree_roots(int width, int height, int top_size, int size, int32_t *xy, int cap) {
  int mn = size;
  if (!tree_sizes(top_size, mn) || mn != size || !dims_ok(width, height)) return 0;
  return roots_of(width, height, top_size, size, xy, cap);
}

int mlt_predict_tree(mlt_ctx *ctx, const mlt_picture *org, const mlt_picture *pred, const mlt_tree_config *cfg, mlt_tree_node *nodes, int node_cap, int *n_nodes,
                     uint8_t *leaf_map_opt, float *logits_opt, int logit_stride, mlt_decision *dec_opt, mlt_candidates *cand_opt) {
  if (!ctx) return MLT_ERR_ARG;
  if (!cfg || cfg->struct_size != sizeof(mlt_tree_config) || !nodes || !n_nodes || !org || !pred || (logits_opt && logit_stride < MLT_MAX_LOGITS) ||
      (cfg->flags & ~MLT_TREE_BY_CANDIDATES)) {
    ctx->err = "mlt_predict_tree: bad argument (cfg with struct_size = sizeof(mlt_tree_config), nodes, n_nodes, both pictures; logit_stride >= 15)";
    return MLT_ERR_ARG;
  }
  TreeLevels lv;
  int rc;
  if ((rc = tree_levels(ctx, "mlt_predict_tree", cfg, lv))) return rc;
  if ((rc = check_at_pair(ctx, "mlt_predict_tree", org, pred))) return rc;
  const int W = org->width, H = org->height;
  const int max_nodes = mlt_tree_max_nodes(W, H, lv.top, lv.mn);
  if ((rc = check_node_cap(ctx, "mlt_predict_tree", node_cap, {}, max_nodes, W, H))) return rc;
  // ---- arguments are good: the tree runs on this context's own device (devices[0] of a multi-device context) ----
  const mlt_tree_picture one{org, pred, cfg->poc, cfg->qp};
  Descent d;
  if ((rc = descend(ctx, "mlt_predict_tree", lv, W, H, 1, &one, by_candidates(cfg), false, TreeOut{leaf_map_opt, logits_opt, logit_stride, dec_opt, cand_opt}, d))) return rc;
  // ---- results: one picture's arena is in the contract's order; everything the caller asked for, then one synchronisation ----
  const Lay::TreeArena::Ptrs &A = d.A;
  if (d.total) HIP_TRY(ctx, hipMemcpyAsync(nodes, A.nodes, (size_t)d.total * sizeof(TreeNodeRec), hipMemcpyDeviceToHost, ctx->stream));
  if (leaf_map_opt) HIP_TRY(ctx, hipMemcpyAsync(leaf_map_opt, A.map, d.map_bytes, hipMemcpyDeviceToHost, ctx->stream));
  for (int l = 0; l < lv.L; ++l) {
    if (!d.n[l]) continue;
    const int nl = lv.st[l]->model.n_logits;
    const size_t s0 = (size_t)d.start[l], c = (size_t)d.n[l];
    if (logits_opt)   // the level's n_logits floats per row; the rest of the caller's row is left alone
      HIP_TRY(ctx, hipMemcpy2DAsync(logits_opt + s0 * (size_t)logit_stride, (size_t)logit_stride * 4, A.logits + s0 * kRowLogits, (size_t)nl * 4, (size_t)nl * 4, c,
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (dec_opt) HIP_TRY(ctx, hipMemcpyAsync(dec_opt + s0, A.dec + s0, c * sizeof(DecisionRec), hipMemcpyDeviceToHost, ctx->stream));
    if (cand_opt) HIP_TRY(ctx, hipMemcpyAsync(cand_opt + s0, A.cand + s0, c * sizeof(CandRec), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *n_nodes = d.total;
  return MLT_OK;
}

int mlt_predict_trees(mlt_ctx *ctx, int n_pictures, const mlt_tree_picture *pics, const mlt_tree_config *cfg, mlt_tree_node *nodes, int node_cap, int32_t *first_node,
                      uint8_t *leaf_maps_opt, float *logits_opt, int logit_stride, mlt_decision *dec_opt, mlt_candidates *cand_opt) {
  if (!ctx) return MLT_ERR_ARG;
  if (n_pictures < 1 || n_pictures > MLT_TREES_MAX_PICTURES || !pics || !cfg || cfg->struct_size != sizeof(mlt_tree_config) || !nodes || !first_node ||
      (logits_opt && logit_stride < MLT_MAX_LOGITS) || (cfg->flags & ~MLT_TREE_BY_CANDIDATES)) {
    ctx->err = "mlt_predict_trees: bad argument (1 .. 256 pictures, pics, cfg with struct_size = sizeof(mlt_tree_config), nodes, first_node; logit_stride >= 15)";
    return MLT_ERR_ARG;
  }
  TreeLevels lv;
  int rc;
  if ((rc = tree_levels(ctx, "mlt_predict_trees", cfg, lv))) return rc;
  const int P = n_pictures;
  if ((rc = check_tree_entries(ctx, "mlt_predict_trees", P, pics))) return rc;
  const int W = pics[0].org->width, H = pics[0].org->height;
  const int max_nodes = mlt_tree_max_nodes(W, H, lv.top, lv.mn);
  if ((rc = check_node_cap(ctx, "mlt_predict_trees", node_cap, {P}, max_nodes, W, H))) return rc;
  // ---- arguments are good: the trees run on this context's own device (devices[0] of a multi-device context) ----
  const TreeOut out{leaf_maps_opt, logits_opt, logit_stride, dec_opt, cand_opt};
  Descent d;
  if ((rc = descend(ctx, "mlt_predict_trees", lv, W, H, P, pics, by_candidates(cfg), true, out, d))) return rc;
  // ---- level-major -> picture-major, then everything the caller asked for and one synchronisation ----
  const Lay::TreeArena::Ptrs &A = d.A;
  const int total = d.total;
  if (total) {
    TreesPackArgs pa{};
    pa.nodes = A.nodes; pa.pic = A.pic; pa.logits = A.logits; pa.dec = A.dec; pa.cand = A.cand;
    pa.o_nodes = A.o_nodes; pa.o_logits = A.o_logits; pa.o_dec = A.o_dec; pa.o_cand = A.o_cand;
    pa.segs = TreesSegs{A.seg_start, A.seg_n, A.pack_base}; pa.first_node = A.first_node; pa.n_pictures = P; pa.n_levels = lv.L; pa.total = total;
    for (int l = 0; l < lv.L; ++l) { pa.lvl_start[l] = d.start[l]; pa.n_logits[l] = lv.st[l]->model.n_logits; }
    const double per_node = 2.0 * sizeof(TreeNodeRec) + 4 + (logits_opt ? 2.0 * kRowLogits * 4 : 0) + (dec_opt ? 2.0 * sizeof(DecisionRec) : 0) + (cand_opt ? 2.0 * sizeof(CandRec) : 0);
    PROF_HIP_TRY(ctx, "tree_pack", 0.0, (double)total * per_node, mlt_launch_trees_pack(pa, ctx->stream));
  }
  if ((rc = copy_packed(ctx, A, total, (size_t)P, d.map_bytes, nodes, out))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(first_node, A.first_node, ((size_t)P + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (first_node[P] != total) { ctx->err = "mlt_predict_trees: bad node count from the device"; return MLT_ERR_HIP; }
  return MLT_OK;
}

int mlt_predict_tree_sweep(mlt_ctx *ctx, const mlt_picture *org, const mlt_picture *pred, const mlt_tree_config *cfg, const int32_t *qps, int n_qps, mlt_tree_node *nodes,
                           int node_cap, int32_t *first_node, int32_t *union_nodes_opt, uint8_t *leaf_maps_opt, float *logits_opt, int logit_stride, mlt_decision *dec_opt,
                           mlt_candidates *cand_opt) {
  if (!ctx) return MLT_ERR_ARG;
  if (!cfg || cfg->struct_size != sizeof(mlt_tree_config) || !qps || n_qps < 1 || n_qps > MLT_SWEEP_MAX_QPS || !nodes || !first_node || !org || !pred ||
      (logits_opt && logit_stride < MLT_MAX_LOGITS) || (cfg->flags & ~MLT_TREE_BY_CANDIDATES)) {
    ctx->err = "mlt_predict_tree_sweep: bad argument (cfg with struct_size = sizeof(mlt_tree_config), qps, 1 <= n_qps <= 32, nodes, first_node, both pictures; logit_stride >= 15)";
    return MLT_ERR_ARG;
  }
  TreeLevels lv;
  int rc;
  if ((rc = tree_levels(ctx, "mlt_predict_tree_sweep", cfg, lv))) return rc;
  if ((rc = check_at_pair(ctx, "mlt_predict_tree_sweep", org, pred))) return rc;
  const int W = org->width, H = org->height, Q = n_qps;
  const int max_nodes = mlt_tree_max_nodes(W, H, lv.top, lv.mn);
  if ((rc = check_node_cap(ctx, "mlt_predict_tree_sweep", node_cap, {Q}, max_nodes, W, H))) return rc;
  // ---- arguments are good: the union descent runs on this context's own device (devices[0] of a multi-device context) ----
  const mlt_tree_picture one{org, pred, cfg->poc, 0};
  const TreeOut out{leaf_maps_opt, logits_opt, logit_stride, dec_opt, cand_opt};
  SweepDescent d;
  if ((rc = descend_sweep(ctx, "mlt_predict_tree_sweep", lv, W, H, 1, &one, qps, Q, by_candidates(cfg), out, d))) return rc;
  return sweep_results(ctx, "mlt_predict_tree_sweep", lv, d, 1, Q, max_nodes, nodes, first_node, union_nodes_opt, out);
}

int mlt_predict_trees_sweep(mlt_ctx *ctx, int n_pictures, const mlt_tree_picture *pics, const mlt_tree_config *cfg, const int32_t *qps, int n_qps, mlt_tree_node *nodes,
                            int node_cap, int32_t *first_node, int32_t *union_nodes_opt, uint8_t *leaf_maps_opt, float *logits_opt, int logit_stride, mlt_decision *dec_opt,
                            mlt_candidates *cand_opt) {
  if (!ctx) return MLT_ERR_ARG;
  if (n_pictures < 1 || n_pictures > MLT_TREES_MAX_PICTURES || !pics || !cfg || cfg->struct_size != sizeof(mlt_tree_config) || !qps || n_qps < 1 ||
      n_qps > MLT_SWEEP_MAX_QPS || !nodes || !first_node || (logits_opt && logit_stride < MLT_MAX_LOGITS) || (cfg->flags & ~MLT_TREE_BY_CANDIDATES)) {
    ctx->err = "mlt_predict_trees_sweep: bad argument (1 .. 256 pictures, pics, cfg with struct_size = sizeof(mlt_tree_config), qps, 1 <= n_qps <= 32, nodes, first_node; "
               "logit_stride >= 15)";
    return MLT_ERR_ARG;
  }
  TreeLevels lv;
  int rc;
  if ((rc = tree_levels(ctx, "mlt_predict_trees_sweep", cfg, lv))) return rc;
  const int P = n_pictures, Q = n_qps;
  if ((rc = check_tree_entries(ctx, "mlt_predict_trees_sweep", P, pics, qps, Q))) return rc;
  const int W = pics[0].org->width, H = pics[0].org->height;
  const int max_nodes = mlt_tree_max_nodes(W, H, lv.top, lv.mn);
  if ((rc = check_node_cap(ctx, "mlt_predict_trees_sweep", node_cap, {P, Q}, max_nodes, W, H))) return rc;
  // ---- arguments are good: the union descent runs on this context's own device (devices[0] of a multi-device context) ----
  // one entry: its offset goes into the points (integers, as the sweep heads would add it) and the descent is mlt_predict_tree_sweep's
  int32_t folded[MLT_SWEEP_MAX_QPS];
  for (int k = 0; k < Q; ++k) folded[k] = P == 1 ? (int32_t)((long long)pics[0].qp + qps[k]) : qps[k];
  const TreeOut out{leaf_maps_opt, logits_opt, logit_stride, dec_opt, cand_opt};
  SweepDescent d;
  if ((rc = descend_sweep(ctx, "mlt_predict_trees_sweep", lv, W, H, P, pics, folded, Q, by_candidates(cfg), out, d))) return rc;
  return sweep_results(ctx, "mlt_predict_trees_sweep", lv, d, P, Q, max_nodes, nodes, first_node, union_nodes_opt, out);
}

#pragma GCC visibility pop
}  // extern "C"
