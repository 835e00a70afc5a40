// mlt_tree_kernels.inc -- partition trees of pictures (include/mltcnn.h: mlt_predict_tree, mlt_predict_trees): the quadtree descent between two network levels, on
// the device.  Included by mlt_kernels.hip.  The union descent of mlt_predict_tree_sweep has kernels of its own at the end of the file.
//
// tree_expand_kernel   one level's evaluated nodes -> their split_mode / confidence / cand_mask / first_child, the next level's nodes (per picture its border roots,
//                      then four children per descending parent, in the parents' order) with their positions and picture indices, the next level's node count
//                      and its row of the segment table.
// tree_raster_kernel   one level's leaves -> the per-16x16-block leaf map of every node's picture.
// tree_pack_kernel     after the last level of mlt_predict_trees: level-major arena -> picture-major output, parent / first_child rewritten to indices inside the
//                      picture's slice.
//
// The arena is LEVEL-major over the n_pictures pictures of the call (mlt_predict_tree: one): a level is one node range -- picture 0's segment, picture 1's, ... --
// and one list for the network pass.  The node order is part of the ABI, so the compaction is an ORDERED one: a tiled exclusive prefix scan of the "descends"
// predicate over the WHOLE level -- wave ballot + popcount for the 64 nodes of a wave, the 16 wave totals of a 1024-node tile through LDS, a running base carried
// from tile to tile -- not an atomic append.  One workgroup walks the tiles: a level holds at most (16384 / 16)^2 ~ 1 M nodes per picture = 1024 tiles of two
// barriers and one 32-byte node record each, and the launch sits between two network passes of milliseconds.
//
// The next level, with nr = n_next_roots roots per picture (all pictures share the geometry), R_i the exclusive rank of descending parent i over the whole level,
// p_i its picture and D_p the rank at the start of picture p's segment (the descending parents of the pictures before p):
//   picture p's segment   starts at next_start + p nr + 4 D_p and holds nr + 4 (D_{p+1} - D_p) nodes: its roots, then its children
//   parent i's children   start at next_start + (p_i + 1) nr + 4 R_i   (= its segment's start + nr + 4 (R_i - D_{p_i}))
// D_p is known once the scan has passed the segment's first node, so the scan comes first and the roots after it.  The first node of a non-empty segment publishes
// its rank as D_p; an EMPTY segment (no roots at that level and nothing descended into it) has no node to do so and takes the rank of the first non-empty segment
// behind it, or the level's total.  With one picture D_0 = 0: the roots sit at next_start, the children behind them.  Everything is written with ordinary vector
// stores; no atomics are needed (the order is the scan's and every output word has exactly one writer).
//
// What the plain and the union descent share is written once, ahead of the kernels: tree_tile_scan (the scan of one tile -- both expand kernels and
// tree_sweep_rank_kernel), tree_point_cmask (a node's cand_mask), tree_write_node (a new node's record, position and picture; the union's overload adds its masks)
// and tree_open_next_level (D_p, the next level's rows of the segment table, the border roots and the count, behind the scan of either expand kernel).

#define MLT_TREE_TILE 1024
#define MLT_TREES_MAX_PICTURES_K 256   // include/mltcnn.h: MLT_TREES_MAX_PICTURES (the per-picture ranks live in LDS)
// (selected, not indexed: a dynamically indexed argument array would be copied to scratch or LDS)
#define MLT_TREE_SEL(v, l) ((l) == 0 ? (v)[0] : (l) == 1 ? (v)[1] : (l) == 2 ? (v)[2] : (v)[3])

// One tile of the ordered scan, called by all MLT_TREE_TILE threads of the workgroup: -> how many threads before this one hold `on`, total <- how many of the tile
// do.  Ballot + popcount inside a wave, the 16 wave totals through wave_total[MLT_TREE_TILE / 64] (LDS); the second barrier keeps the next tile's totals off this
// tile's reads.  The caller carries the base from tile to tile.
__device__ __forceinline__ int tree_tile_scan(bool on, int *wave_total, int &total) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const unsigned long long b = __ballot(on);
  if (lane == 0) wave_total[wave] = __popcll(b);
  __syncthreads();
  int woff = 0;
  total = 0;
  for (int w = 0; w < MLT_TREE_TILE / 64; ++w) {
    const int s = wave_total[w];
    woff += w < wave ? s : 0;
    total += s;
  }
  __syncthreads();   // (the next tile overwrites wave_total)
  return woff + __popcll(b & ((1ull << lane) - 1ull));
}

// cand_mask of one evaluated element: the candidate record's, or the default policy's without asking the heads launch for one -- the argmax alone, every class when
// a logit of the decision head is NaN (head_candidates)
__device__ __forceinline__ uint32_t tree_point_cmask(const DecisionRec &d, const CandRec *cand, const float *logits, size_t e, int n_logits, int head_off, int head_classes) {
  if (cand) return cand[e].mask;
  const float *l = logits + e * (size_t)n_logits + head_off;
  bool nan = false;
  for (int k = 0; k < head_classes; ++k) nan = nan || (l[k] != l[k]);
  return nan ? (1u << head_classes) - 1u : 1u << d.raw_mode;
}

__device__ __forceinline__ void tree_write_node(const TreeLevelArgs &a, int idx, int pic, int x, int y, int size, int depth, int flags, int parent) {
  if (idx < 0 || idx >= a.node_cap) return;   // (the host sizes the arena for trees -- unions -- that descend everywhere: never taken)
  TreeNodeRec r;
  r.x = x; r.y = y; r.size = (int16_t)size; r.depth = (int8_t)depth; r.flags = (uint8_t)flags;
  r.parent = parent; r.first_child = -1; r.split_mode = -1; r.confidence = 0.f; r.cand_mask = 0u;
  a.nodes[idx] = r;
  a.xy[2 * (size_t)idx] = x;
  a.xy[2 * (size_t)idx + 1] = y;
  a.pic[idx] = pic;
}
// a node of the union descent: + the points it is alive under, descending under none yet
__device__ __forceinline__ void tree_write_node(const TreeSweepExpandArgs &a, int idx, int pic, int x, int y, int size, int depth, int flags, int parent, uint32_t alive) {
  if (idx < 0 || idx >= a.node_cap) return;
  tree_write_node(static_cast<const TreeLevelArgs &>(a), idx, pic, x, y, size, depth, flags, parent);
  a.alive[idx] = alive;
  a.desc[idx] = 0u;
}

// Behind the scan of a level (base: its descending nodes; seg_rank[p]: D_p as the first node of picture p's segment published it): seg_first <- D_p of every
// picture -- its own first node's rank, or (empty segment) that of the first non-empty segment behind it, [n_pictures] the level's total --, the next level's rows
// of the segment table, every picture's border roots (host-known, raster order, the same for all pictures) through write_root(k, p, x, y), k counted from the next
// level's first node, and the next level's count.  Called by the whole workgroup.
template <class WriteRoot>
__device__ __forceinline__ void tree_open_next_level(const TreeLevelArgs &a, const int *seg_rank, int *seg_first, int base, int next_start, WriteRoot write_root) {
  const int tid = (int)threadIdx.x, P = a.n_pictures, nr = a.n_next_roots;
  const int32_t *cur_n = a.seg_n + (size_t)(a.lvl < 0 ? 0 : a.lvl) * P;
  __syncthreads();   // seg_rank is complete
  if (tid <= P) {
    int q = tid;
    while (q < P && (a.lvl < 0 || cur_n[q] == 0)) ++q;
    seg_first[tid] = q < P ? seg_rank[q] : base;
  }
  __syncthreads();
  if (tid < P) {
    a.seg_start[(size_t)(a.lvl + 1) * P + tid] = next_start + tid * nr + 4 * seg_first[tid];
    a.seg_n[(size_t)(a.lvl + 1) * P + tid] = nr + 4 * (seg_first[tid + 1] - seg_first[tid]);
  }
  for (int i = tid; i < P * nr; i += MLT_TREE_TILE) {
    const int p = i / nr, r = i - p * nr;
    write_root(p * nr + 4 * seg_first[p] + r, p, a.next_roots[2 * r], a.next_roots[2 * r + 1]);
  }
  if (tid == 0 && a.count) a.count[0] = P * nr + 4 * base;
}

__global__ __launch_bounds__(MLT_TREE_TILE) void tree_expand_kernel(const TreeExpandArgs a) {
  __shared__ int wave_total[MLT_TREE_TILE / 64];
  __shared__ int seg_rank[MLT_TREES_MAX_PICTURES_K];       // D_p as published by the first node of a non-empty segment
  __shared__ int seg_first[MLT_TREES_MAX_PICTURES_K + 1];  // D_p of every picture; [n_pictures] = the level's total
  __shared__ int pic_total[MLT_TREES_MAX_PICTURES_K];      // last launch: nodes of picture p over all levels
  const int tid = (int)threadIdx.x, P = a.n_pictures, nr = a.n_next_roots;
  const int next_start = a.lvl_start + a.lvl_n, child_size = a.size >> 1;
  const int32_t *cur_start = a.seg_start + (size_t)(a.lvl < 0 ? 0 : a.lvl) * P;
  int base = 0;   // descending parents of the tiles before this one (the same value in every thread)
  for (int t0 = 0; t0 < a.lvl_n; t0 += MLT_TREE_TILE) {
    const int i = t0 + tid;
    const bool in = i < a.lvl_n;
    const int node = a.lvl_start + (in ? i : 0);
    bool desc = false;
    int32_t split = -1;
    float conf = 0.f;
    uint32_t cmask = 0u;
    int p = 0;
    if (in) {
      p = a.pic[node];
      const DecisionRec &d = a.dec[i];
      split = d.split_mode;
      conf = d.confidence;
      cmask = tree_point_cmask(d, a.cand, a.logits, (size_t)i, a.n_logits, a.head_off, a.head_classes);
      desc = a.by_candidates ? (cmask & a.descend_mask) != 0u : (split >= 0 && ((a.descend_mask >> split) & 1u) != 0u);
    }
    int total;
    const int rank = base + tree_tile_scan(desc, wave_total, total);
    if (in) {
      if ((unsigned)p < (unsigned)P && node == cur_start[p]) seg_rank[p] = rank;   // the segment's first node: one writer per picture
      int first_child = -1;
      if (desc) {
        const int fc = next_start + (p + 1) * nr + 4 * rank;
        if (fc + 3 < a.node_cap) {
          first_child = fc;
          const int x = a.xy[2 * (size_t)node], y = a.xy[2 * (size_t)node + 1];
          for (int j = 0; j < 4; ++j) tree_write_node(a, fc + j, p, x + (j & 1) * child_size, y + (j >> 1) * child_size, child_size, a.lvl + 1, 0, node);
        }
      }
      TreeNodeRec &r = a.nodes[node];
      r.first_child = first_child; r.split_mode = split; r.confidence = conf; r.cand_mask = cmask;
    }
    base += total;
  }
  if (a.lvl != a.n_levels - 1) {
    tree_open_next_level(a, seg_rank, seg_first, base, next_start,
                         [&](int k, int p, int x, int y) { tree_write_node(a, next_start + k, p, x, y, child_size, a.lvl + 1, a.root_flags, -1); });
    return;
  }
  // the last level: where every (level, picture) segment starts in the picture-major output, and first_node[]
  if (tid < P) {
    int s = 0;
    for (int l = 0; l < a.n_levels; ++l) s += a.seg_n[(size_t)l * P + tid];
    pic_total[tid] = s;
  }
  __syncthreads();
  if (tid <= P) {
    int first = 0;
    for (int q = 0; q < tid; ++q) first += pic_total[q];
    a.first_node[tid] = first;
    if (tid < P)
      for (int l = 0; l < a.n_levels; ++l) {
        a.pack_base[(size_t)l * P + tid] = first;
        first += a.seg_n[(size_t)l * P + tid];
      }
  }
}

// One work item per 16 x 16 block of every node of the level; the items of a node that has children leave.  Leaves are disjoint, so plain byte stores suffice (the
// maps were filled with 0xFF before the first level).
__global__ __launch_bounds__(256) void tree_raster_kernel(const TreeRasterArgs a) {
  const size_t total = (size_t)a.lvl_n << (2 * a.blk_l), step = (size_t)gridDim.x * 256;
  for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < total; it += step) {
    const int i = (int)(it >> (2 * a.blk_l)), b = (int)(it & ((1u << (2 * a.blk_l)) - 1u));
    const TreeNodeRec &r = a.nodes[a.lvl_start + i];
    if (r.first_child >= 0) continue;
    const int mx = (r.x >> 4) + (b & ((1 << a.blk_l) - 1)), my = (r.y >> 4) + (b >> a.blk_l);
    if (mx < 0 || my < 0 || mx >= a.map_w || my >= a.map_h) continue;   // (a node is a complete CU of the picture: never taken)
    a.map[(size_t)a.pic[a.lvl_start + i] * a.map_bytes + (size_t)my * a.map_w + mx] = (uint8_t)(a.blk_l | ((r.split_mode + 1) << 4));
  }
}

// One work item per node.  Node g of level l, picture p goes to pack_base[l][p] + (g - seg_start[l][p]); its parent (level l - 1) and first child (level l + 1) lie
// in the same picture's segments of those levels, and an index inside the slice is the packed position minus first_node[p].
__global__ __launch_bounds__(256) void tree_pack_kernel(const TreesPackArgs a) {
  const int P = a.n_pictures, step = (int)gridDim.x * 256;
  for (int g = (int)(blockIdx.x * 256 + threadIdx.x); g < a.total; g += step) {
    TreeNodeRec r = a.nodes[g];
    const int p = a.pic[g], l = r.depth;
    if ((unsigned)p >= (unsigned)P || (unsigned)l >= (unsigned)a.n_levels) continue;   // (never taken)
    const size_t at = (size_t)l * P + p;
    const int first = a.first_node[p], dst = a.segs.pack_base[at] + (g - a.segs.start[at]);
    if ((unsigned)dst >= (unsigned)a.total) continue;                                     // (never taken)
    if (r.parent >= 0 && l > 0) r.parent = a.segs.pack_base[at - P] + (r.parent - a.segs.start[at - P]) - first;
    if (r.first_child >= 0 && l + 1 < a.n_levels) r.first_child = a.segs.pack_base[at + P] + (r.first_child - a.segs.start[at + P]) - first;
    a.o_nodes[dst] = r;
    if (a.o_logits) {
      const int nl = MLT_TREE_SEL(a.n_logits, l), ls = MLT_TREE_SEL(a.lvl_start, l);
      const float *src = a.logits + (size_t)ls * MLT_TREES_ROW + (size_t)(g - ls) * nl;
      float *o = a.o_logits + (size_t)dst * MLT_TREES_ROW;
      for (int k = 0; k < MLT_TREES_ROW; ++k) o[k] = k < nl ? src[k] : 0.f;
    }
    if (a.o_dec) a.o_dec[dst] = a.dec[g];
    if (a.o_cand) a.o_cand[dst] = a.cand[g];
  }
}

// ---------------------------------------------------------------------------------------------
// Tree sweeps (mlt_predict_tree_sweep): ONE descent over the UNION of the trees of a picture pair under n_qps points.
//
// tree_expand_sweep_kernel   one level's union nodes -> desc (bit q: the node descends under point q -- tree_expand_kernel's rule on slab q's records, for the
//                            points the node is alive under), the next level: its border roots (alive under every point), then four children per node with
//                            desc != 0 (alive = desc), in the parents' order -- the same ordered tiled scan -- and the next level's count.
// tree_sweep_raster_kernel   one level's leaves into the map of every point: a leaf under q is alive under q and does not descend under q.
// tree_sweep_rank_kernel     after the last level, one workgroup per point: an ordered scan of "alive under q" over the levels -> a node's index inside slice q.
//                            Restricted to the nodes alive under q the union's level order IS the single descent's order (roots first, then children in their
//                            parents' order, and a parent alive under q keeps its rank among those), so the scan's running count is that index.
// tree_sweep_pack_kernel     one work item per (point, union node): the node's record of slice q -- parent / first_child through idx, split_mode / confidence /
//                            cand_mask from slab q -- with its logits row and records; workgroup 0 also writes first_node[] and union_nodes[].
// Plain vector stores, one writer per output word, no atomics.
// ---------------------------------------------------------------------------------------------

// The next level of the union of n_pictures entries is tree_expand_kernel's: with nr roots per entry, R_i the exclusive rank of descending node i over the WHOLE
// level and D_p the rank at the start of entry p's segment, entry p's segment starts at next_start + p nr + 4 D_p and node i's children at
// next_start + (p_i + 1) nr + 4 R_i; an empty segment takes the rank of the first non-empty segment behind it, or the level's total.  One entry: D_0 = 0.
__global__ __launch_bounds__(MLT_TREE_TILE) void tree_expand_sweep_kernel(const TreeSweepExpandArgs a) {
  __shared__ int wave_total[MLT_TREE_TILE / 64];
  __shared__ int seg_rank[MLT_TREES_MAX_PICTURES_K];       // D_p as published by the first node of a non-empty segment
  __shared__ int seg_first[MLT_TREES_MAX_PICTURES_K + 1];  // D_p of every entry; [n_pictures] = the level's total
  const int tid = (int)threadIdx.x, Q = a.n_qps, P = a.n_pictures, nr = a.n_next_roots, child_size = a.size >> 1;
  const uint32_t all = Q >= 32 ? 0xFFFFFFFFu : (1u << Q) - 1u;
  const int32_t *cur_start = a.seg_start + (size_t)(a.lvl < 0 ? 0 : a.lvl) * P;
  int base = 0;   // descending nodes of the tiles before this one (the same value in every thread)
  for (int t0 = 0; t0 < a.lvl_n; t0 += MLT_TREE_TILE) {
    const int i = t0 + tid;
    const bool in = i < a.lvl_n;
    const int node = a.lvl_start + (in ? i : 0);
    uint32_t dm = 0u;
    int p = 0;
    if (in) p = a.pic[node];
    if (in && a.descend_mask) {
      const uint32_t al = a.alive[node] & all;
      for (int q = 0; q < Q; ++q) {
        if (!((al >> q) & 1u)) continue;
        const size_t e = (size_t)q * (size_t)a.slab + (size_t)i;
        const DecisionRec &d = a.dec[e];
        const int32_t split = d.split_mode;
        bool ds;
        if (a.by_candidates) ds = (tree_point_cmask(d, a.cand, a.logits, e, a.n_logits, a.head_off, a.head_classes) & a.descend_mask) != 0u;
        else ds = split >= 0 && ((a.descend_mask >> split) & 1u) != 0u;
        if (ds) dm |= 1u << q;
      }
    }
    const bool desc = dm != 0u;
    int total;
    const int rank = base + tree_tile_scan(desc, wave_total, total);
    if (in) {
      const bool p_ok = (unsigned)p < (unsigned)P;
      if (p_ok && node == cur_start[p]) seg_rank[p] = rank;   // the segment's first node: one writer per entry
      int first_child = -1;
      if (desc && p_ok) {
        const int k = (p + 1) * nr + 4 * rank;
        if (k + 3 < a.next_cap && a.next_start + k + 3 < a.node_cap) {
          const int fc = first_child = a.next_start + k;
          const int x = a.xy[2 * (size_t)node], y = a.xy[2 * (size_t)node + 1];
          for (int j = 0; j < 4; ++j) tree_write_node(a, fc + j, p, x + (j & 1) * child_size, y + (j >> 1) * child_size, child_size, a.lvl + 1, 0, node, dm);
        }
      }
      a.nodes[node].first_child = first_child;
      a.desc[node] = first_child >= 0 ? dm : 0u;
    }
    base += total;
  }
  if (!a.next_roots && !a.count) return;   // the last level
  // the border roots are part of every tree of their entry
  tree_open_next_level(a, seg_rank, seg_first, base, a.next_start, [&](int k, int p, int x, int y) {
    if (k < a.next_cap) tree_write_node(a, a.next_start + k, p, x, y, child_size, a.lvl + 1, a.root_flags, -1, all);
  });
}

// One work item per 16 x 16 block of every union node of the level; under a point the leaves are disjoint, and every (entry, point) has a map of its own.
__global__ __launch_bounds__(256) void tree_sweep_raster_kernel(const TreeSweepRasterArgs a) {
  const size_t total = (size_t)a.lvl_n << (2 * a.blk_l), step = (size_t)gridDim.x * 256;
  const uint32_t all = a.n_qps >= 32 ? 0xFFFFFFFFu : (1u << a.n_qps) - 1u;
  for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < total; it += step) {
    const int i = (int)(it >> (2 * a.blk_l)), b = (int)(it & ((1u << (2 * a.blk_l)) - 1u));
    const int node = a.lvl_start + i;
    const uint32_t leaf = a.alive[node] & ~a.desc[node] & all;
    if (!leaf) continue;
    const TreeNodeRec &r = a.nodes[node];
    const int mx = (r.x >> 4) + (b & ((1 << a.blk_l) - 1)), my = (r.y >> 4) + (b >> a.blk_l), p = a.pic[node];
    if (mx < 0 || my < 0 || mx >= a.map_w || my >= a.map_h || (unsigned)p >= (unsigned)a.n_pictures) continue;   // (a node is a complete CU of its entry's picture: never taken)
    for (int q = 0; q < a.n_qps; ++q)
      if ((leaf >> q) & 1u)
        a.map[((size_t)p * a.n_qps + q) * a.map_bytes + (size_t)my * a.map_w + mx] = (uint8_t)(a.blk_l | ((a.dec[(size_t)q * (size_t)a.slab + (size_t)i].split_mode + 1) << 4));
  }
}

// Workgroup p * n_qps + q: the ordered scan of bit q of alive over entry p's segment of every level, level after level (tree_expand_kernel's tile scan with the
// base carried on).  Every union node belongs to one entry, so idx[q][node] has one writer.
__global__ __launch_bounds__(MLT_TREE_TILE) void tree_sweep_rank_kernel(const TreeSweepPackArgs a) {
  __shared__ int wave_total[MLT_TREE_TILE / 64];
  const int tid = (int)threadIdx.x, P = a.n_pictures;
  if ((int)blockIdx.x >= P * a.n_qps) return;
  const int p = (int)blockIdx.x / a.n_qps, q = (int)blockIdx.x - p * a.n_qps;
  int32_t *idx = a.idx + (size_t)q * (size_t)a.node_cap;
  int base = 0;
  for (int l = 0; l < a.n_levels && l < MLT_TREES_LEVELS; ++l) {
    const int start = a.seg_start[(size_t)l * P + p], n = a.seg_n[(size_t)l * P + p];
    for (int t0 = 0; t0 < n; t0 += MLT_TREE_TILE) {
      const int i = t0 + tid, node = start + i;
      const bool in = i < n && node >= 0 && node < a.node_cap;
      const bool on = in && ((a.alive[node] >> q) & 1u) != 0u;
      int total;
      const int rank = base + tree_tile_scan(on, wave_total, total);
      if (in) idx[node] = on ? rank : -1;
      base += total;
    }
  }
  if (tid == 0) a.total[blockIdx.x] = base;
}

#define MLT_TREE_SWEEP_MAX_SLICES (MLT_TREES_MAX_PICTURES_K * MLT_SWEEP_MAX_QPS_K)

__global__ __launch_bounds__(256) void tree_sweep_pack_kernel(const TreeSweepPackArgs a) {
  __shared__ int first[MLT_TREE_SWEEP_MAX_SLICES + 1];   // where slice p * n_qps + q starts: every workgroup sums the slices' totals for itself
  __shared__ int part[256];
  const int tid = (int)threadIdx.x, Q = a.n_qps, P = a.n_pictures;
  const int S = P * Q <= MLT_TREE_SWEEP_MAX_SLICES ? P * Q : MLT_TREE_SWEEP_MAX_SLICES, per = (S + 255) / 256;
  const int s_lo = tid * per < S ? tid * per : S, s_hi = s_lo + per < S ? s_lo + per : S;
  {
    int sum = 0;
    for (int s = s_lo; s < s_hi; ++s) sum += a.total[s];
    part[tid] = sum;
  }
  __syncthreads();
  {
    int f = 0;
    for (int t = 0; t < tid; ++t) f += part[t];
    for (int s = s_lo; s < s_hi; ++s) {
      first[s] = f;
      if (blockIdx.x == 0) a.first_node[s] = f;
      f += a.total[s];
    }
    if (s_lo < S && s_hi == S) {   // the thread of the last slice
      first[S] = f;
      if (blockIdx.x == 0) a.first_node[S] = f;
    }
  }
  if (blockIdx.x == 0)
    for (int t = tid; t < P * MLT_TREES_LEVELS; t += 256) {
      const int p = t / MLT_TREES_LEVELS, l = t - p * MLT_TREES_LEVELS;
      a.union_nodes[t] = l < a.n_levels ? a.seg_n[(size_t)l * P + p] : 0;
    }
  __syncthreads();
  int un = 0;   // union nodes over all levels and entries
  for (int l = 0; l < a.n_levels && l < MLT_TREES_LEVELS; ++l) un += MLT_TREE_SEL(a.lvl_n, l);
  const size_t items = (size_t)Q * (size_t)un, step = (size_t)gridDim.x * 256;
  for (size_t it = (size_t)blockIdx.x * 256 + tid; it < items; it += step) {
    const int q = (int)(it / (size_t)un);
    int u = (int)(it - (size_t)q * (size_t)un), l = 0;
    while (l + 1 < a.n_levels && u >= MLT_TREE_SEL(a.lvl_n, l)) { u -= MLT_TREE_SEL(a.lvl_n, l); ++l; }
    const int start = MLT_TREE_SEL(a.lvl_start, l), g = start + u;
    if (g >= a.node_cap || !((a.alive[g] >> q) & 1u)) continue;
    const int p = a.pic[g];
    if ((unsigned)p >= (unsigned)P) continue;   // (never taken)
    const int32_t *idx = a.idx + (size_t)q * (size_t)a.node_cap;
    const int li = idx[g], dst = first[p * Q + q] + li;
    if (li < 0 || (unsigned)dst >= (unsigned)a.out_cap) continue;   // (never taken)
    const int cap = MLT_TREE_SEL(a.lvl_cap, l), nl = MLT_TREE_SEL(a.n_logits, l);
    const size_t slab0 = (size_t)Q * (size_t)start, e = slab0 + (size_t)q * (size_t)cap + (size_t)u;   // element (l, q, u): level l starts at node off[l] = start
    TreeNodeRec r = a.nodes[g];
    r.parent = r.parent >= 0 && r.parent < a.node_cap ? idx[r.parent] : -1;
    r.first_child = ((a.desc[g] >> q) & 1u) && r.first_child >= 0 && r.first_child < a.node_cap ? idx[r.first_child] : -1;
    const DecisionRec d = a.dec[e];
    // a level's logits are dense rows of nl floats from the level's first reserved row; its candidate records are read only where the heads wrote them
    const float *lg = a.logits ? a.logits + slab0 * MLT_TREES_ROW : nullptr;
    const size_t le = (size_t)q * (size_t)cap + (size_t)u;
    r.split_mode = d.split_mode; r.confidence = d.confidence;
    r.cand_mask = tree_point_cmask(d, MLT_TREE_SEL(a.has_cand, l) ? a.cand + slab0 : nullptr, lg, le, nl, MLT_TREE_SEL(a.head_off, l), MLT_TREE_SEL(a.head_classes, l));
    a.o_nodes[dst] = r;
    if (a.o_logits) {
      const float *src = lg + le * (size_t)nl;
      float *o = a.o_logits + (size_t)dst * MLT_TREES_ROW;
      for (int k = 0; k < MLT_TREES_ROW; ++k) o[k] = k < nl ? src[k] : 0.f;
    }
    if (a.o_dec) a.o_dec[dst] = d;
    if (a.o_cand) a.o_cand[dst] = a.cand[e];
  }
}
