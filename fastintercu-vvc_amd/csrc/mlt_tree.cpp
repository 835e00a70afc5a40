// mlt_tree.cpp -- partition trees of a picture (include/mltcnn.h): mlt_predict_tree, mlt_tree_roots, mlt_tree_max_nodes.
//
// Per level: the network on the level's nodes -- predict_at_chunks (mlt_pictures.cpp) on the slice of the device-resident position list that IS the level, so
// launches, guards and exact re-runs are mlt_predict_at's and so is every result -- then tree_expand_kernel (mlt_tree_kernels.inc): the level's decisions into its
// node records, the next level's nodes and positions behind them, the next level's count; tree_raster_kernel paints the level's leaves into the map; one 4-byte
// count comes back.  Nodes, positions and the per-node logits / records are indexed by NODE in one device arena, so a level's arrays are slices of the tree's and the
// end of the call is a handful of D2H copies.
#include "mlt_runtime.h"

namespace {

const int kMinDim = 16, kMaxDim = 16384;   // a picture's geometry (mlt_picture_create)
const int kRowLogits = Lay::TreeArena::kRow;   // floats the arena reserves per node (a level's logits are dense [n][n_logits] from the level's first row)

bool tree_sizes(int &top, int &mn) {
  if (top == 0) top = 128;
  if (mn == 0) mn = 16;
  return size_index(top) >= 0 && size_index(mn) >= 0 && mn <= top;
}
bool dims_ok(int w, int h) { return w >= kMinDim && h >= kMinDim && w <= kMaxDim && h <= kMaxDim; }

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
  int top = cfg->top_size, mn = cfg->min_size;
  if (!tree_sizes(top, mn)) { ctx->err = "mlt_predict_tree: top_size / min_size must be 128, 64, 32 or 16 with min_size <= top_size"; return MLT_ERR_ARG; }
  // the levels: every size top..min loaded, every descend mask inside its decision head
  SizeState *st[4];
  uint32_t mask[4];
  int L = 0, rc;
  for (int S = top; S >= mn; S >>= 1, ++L) {
    if ((rc = check_size(ctx, S, &st[L]))) return rc;
    const uint32_t m = cfg->descend_mask[size_index(S)];
    mask[L] = m ? m : 1u << 1;
    const int K = st[L]->head_classes();
    if (mask[L] >> K) {
      char msg[160];
      std::snprintf(msg, sizeof msg, "mlt_predict_tree: descend_mask of size %d names a class at or above the %d classes of its decision head", S, K);
      ctx->err = msg;
      return MLT_ERR_ARG;
    }
  }
  if (!owns_picture(ctx, org) || !owns_picture(ctx, pred)) { ctx->err = "mlt_predict_tree: both pictures must belong to this context"; return MLT_ERR_ARG; }
  if (org->width != pred->width || org->height != pred->height) { ctx->err = "mlt_predict_tree: the two pictures differ in width or height"; return MLT_ERR_ARG; }
  const int W = org->width, H = org->height;
  const int max_nodes = mlt_tree_max_nodes(W, H, top, mn);
  if (node_cap < max_nodes) {
    char msg[160];
    std::snprintf(msg, sizeof msg, "mlt_predict_tree: node_cap %d is below mlt_tree_max_nodes = %d of a %d x %d picture", node_cap, max_nodes, W, H);
    ctx->err = msg;
    return MLT_ERR_ARG;
  }
  // ---- arguments are good: the tree runs on this context's own device (devices[0] of a multi-device context) ----
  if (hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return MLT_ERR_NO_DEVICE; }
  const bool by_cand = (cfg->flags & MLT_TREE_BY_CANDIDATES) != 0;
  // candidate records come from the heads launch only where cand_mask can differ from 1 << raw_mode (a policy is set) or the caller asks for them
  bool want_cand[4], any_cand = false;
  for (int l = 0; l < L; ++l) any_cand = (want_cand[l] = cand_opt || by_cand || st[l]->cand_policy()) || any_cand;
  std::vector<int32_t> roots;
  int root_off[4], n_roots[4];
  for (int l = 0, S = top; l < L; ++l, S >>= 1) {
    root_off[l] = (int)(roots.size() / 2);
    n_roots[l] = roots_of(W, H, top, S, nullptr, 0);
    roots.resize(roots.size() + 2 * (size_t)n_roots[l]);
    if (n_roots[l]) (void)roots_of(W, H, top, S, roots.data() + 2 * (size_t)root_off[l], n_roots[l]);
  }
  const int map_w = W / 16, map_h = H / 16;
  const size_t map_bytes = (size_t)map_w * map_h;
  const Lay::TreeArena arena((size_t)max_nodes, roots.size() / 2, map_bytes, any_cand);
  if ((rc = ctx->tree_dev.reserve(ctx, arena.bytes(), "mlt_predict_tree"))) return rc;
  if (!ctx->tree_host) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->tree_host, 64, hipHostMallocDefault));
  const Lay::TreeArena::Ptrs A = arena.at(ctx->tree_dev.p);
  if (!roots.empty()) HIP_TRY(ctx, hipMemcpyAsync(A.roots, roots.data(), roots.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(A.map, 0xFF, map_bytes, ctx->stream));
  const AtPlanes pl = AtPlanes::of(org, pred, 0);
  Launch prof{ctx};
  auto expand = [&](const TreeExpandArgs &ea) -> int {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int r;
    // algorithmic bytes the host knows: the level's records read and its node fields written, the next level's roots written (the children's count is the device's)
    if ((r = prof.prof_begin("tree_expand", 0.0, (double)ea.lvl_n * (sizeof(DecisionRec) + 16) + (double)ea.n_next_roots * (sizeof(TreeNodeRec) + 16), e0, e1))) return r;
    HIP_TRY(ctx, mlt_launch_tree_expand(ea, ctx->stream));
    return prof.prof_end(e1);
  };
  TreeExpandArgs ea{};
  ea.nodes = A.nodes; ea.xy = A.xy; ea.node_cap = max_nodes; ea.by_candidates = by_cand ? 1 : 0;
  // the tree opens: no parents, the top level's roots
  ea.lvl_start = 0; ea.lvl_n = 0; ea.size = 2 * top; ea.depth = -1;
  ea.next_roots = A.roots; ea.n_next_roots = n_roots[0]; ea.root_flags = 0; ea.count = nullptr;
  if ((rc = expand(ea))) return rc;
  int start = 0, n = n_roots[0], lvl_start[4], lvl_n[4];
  for (int l = 0, S = top; l < L; ++l, S >>= 1) {
    SizeState *s = st[l];
    const int nl = s->model.n_logits;
    const bool last = l == L - 1;
    lvl_start[l] = start; lvl_n[l] = n;
    float *d_lg = A.logits + (size_t)start * kRowLogits;
    DecisionRec *d_dec = A.dec + start;
    CandRec *d_cand = want_cand[l] ? A.cand + start : nullptr;
    if (n > 0) {
      const AtOut out{nullptr, d_lg, (mlt_decision *)d_dec, (mlt_candidates *)d_cand};
      if ((rc = predict_at_chunks(ctx, s, pl, n, AtList::on_device(A.xy + 2 * (size_t)start, cfg->poc, cfg->qp), out))) return rc;
    }
    ea.lvl_start = start; ea.lvl_n = n; ea.size = S; ea.depth = l;
    ea.dec = d_dec; ea.cand = d_cand; ea.logits = d_lg; ea.n_logits = nl;
    ea.head_off = s->head_off(); ea.head_classes = s->head_classes();
    ea.descend_mask = last ? 0u : mask[l];
    ea.next_roots = last ? nullptr : A.roots + 2 * (size_t)root_off[l + 1];
    ea.n_next_roots = last ? 0 : n_roots[l + 1];
    ea.root_flags = 1;
    ea.count = last ? nullptr : A.count;
    if ((rc = expand(ea))) return rc;
    if (n > 0 && leaf_map_opt) {
      TreeRasterArgs ra{};
      ra.nodes = A.nodes; ra.lvl_start = start; ra.lvl_n = n; ra.blk_l = ilog2(S) - 4; ra.map = A.map; ra.map_w = map_w; ra.map_h = map_h;
      hipEvent_t e0 = nullptr, e1 = nullptr;
      // algorithmic bytes: every node record read once, one byte per block of a leaf written (at most the level's whole area)
      if ((rc = prof.prof_begin("tree_raster", 0.0, (double)n * (sizeof(TreeNodeRec) + (double)(1 << (2 * ra.blk_l))), e0, e1))) return rc;
      HIP_TRY(ctx, mlt_launch_tree_raster(ra, ctx->stream));
      if ((rc = prof.prof_end(e1))) return rc;
    }
    start += n;
    if (last) break;
    // the one host synchronisation of the level beside the guards': how many nodes the next level has
    HIP_TRY(ctx, hipMemcpyAsync(ctx->tree_host, A.count, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    n = ctx->tree_host[0];
    if (n < n_roots[l + 1] || ((n - n_roots[l + 1]) & 3) || (long long)start + n > max_nodes) { ctx->err = "mlt_predict_tree: bad node count from the device"; return MLT_ERR_HIP; }
  }
  // ---- results: everything the caller asked for, then one synchronisation ----
  const int total = start;
  if (total) HIP_TRY(ctx, hipMemcpyAsync(nodes, A.nodes, (size_t)total * sizeof(TreeNodeRec), hipMemcpyDeviceToHost, ctx->stream));
  if (leaf_map_opt && map_bytes) HIP_TRY(ctx, hipMemcpyAsync(leaf_map_opt, A.map, map_bytes, hipMemcpyDeviceToHost, ctx->stream));
  for (int l = 0; l < L; ++l) {
    if (!lvl_n[l]) continue;
    const int nl = st[l]->model.n_logits;
    const size_t s0 = (size_t)lvl_start[l], c = (size_t)lvl_n[l];
    if (logits_opt)
      HIP_TRY(ctx, hipMemcpy2DAsync(logits_opt + s0 * (size_t)logit_stride, (size_t)logit_stride * 4, A.logits + s0 * kRowLogits, (size_t)nl * 4, (size_t)nl * 4, c,
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (dec_opt) HIP_TRY(ctx, hipMemcpyAsync(dec_opt + s0, A.dec + s0, c * sizeof(DecisionRec), hipMemcpyDeviceToHost, ctx->stream));
    if (cand_opt) HIP_TRY(ctx, hipMemcpyAsync(cand_opt + s0, A.cand + s0, c * sizeof(CandRec), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *n_nodes = total;
  return MLT_OK;
}

#pragma GCC visibility pop
}  // extern "C"
