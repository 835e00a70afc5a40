// mlt_tree_kernels.inc -- partition trees of a picture (include/mltcnn.h: mlt_predict_tree): the quadtree descent between two network levels, on the device.
// Included by mlt_kernels.hip.
//
// tree_expand_kernel   one level's evaluated nodes -> their split_mode / confidence / cand_mask / first_child, the next level's nodes (its border roots, then
//                      four children per descending parent, in the parents' order) with their positions, and the next level's node count.
// tree_raster_kernel   one level's leaves -> the per-16x16-block leaf map.
//
// The node order is part of the ABI, so the compaction is an ORDERED one: a tiled exclusive prefix scan of the "descends" predicate -- wave ballot + popcount for
// the 64 nodes of a wave, the 16 wave totals of a 1024-node tile through LDS, a running base carried from tile to tile -- not an atomic append.  One workgroup
// walks the tiles: a level holds at most (16384 / 16)^2 ~ 1 M nodes = 1024 tiles of two barriers and one 32-byte node record each, and the launch sits between
// two network passes of milliseconds.  Everything is written with ordinary stores; no atomics are needed (every output word has exactly one writer).

#define MLT_TREE_TILE 1024

__device__ __forceinline__ void tree_write_node(const TreeExpandArgs &a, int idx, int x, int y, int size, int depth, int flags, int parent) {
  if (idx < 0 || idx >= a.node_cap) return;   // (the host sizes the arena for a tree that descends everywhere: never taken)
  TreeNodeRec r;
  r.x = x; r.y = y; r.size = (int16_t)size; r.depth = (int8_t)depth; r.flags = (uint8_t)flags;
  r.parent = parent; r.first_child = -1; r.split_mode = -1; r.confidence = 0.f; r.cand_mask = 0u;
  a.nodes[idx] = r;
  a.xy[2 * (size_t)idx] = x;
  a.xy[2 * (size_t)idx + 1] = y;
}

__global__ __launch_bounds__(MLT_TREE_TILE) void tree_expand_kernel(const TreeExpandArgs a) {
  __shared__ int wave_total[MLT_TREE_TILE / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int next_start = a.lvl_start + a.lvl_n, child_size = a.size >> 1, child_start = next_start + a.n_next_roots;
  // the next level opens with its border roots (host-known, raster order)
  for (int i = tid; i < a.n_next_roots; i += MLT_TREE_TILE)
    tree_write_node(a, next_start + i, a.next_roots[2 * i], a.next_roots[2 * i + 1], child_size, a.depth + 1, a.root_flags, -1);
  int base = 0;   // descending parents of the tiles before this one (the same value in every thread)
  for (int t0 = 0; t0 < a.lvl_n; t0 += MLT_TREE_TILE) {
    const int i = t0 + tid;
    const bool in = i < a.lvl_n;
    const int node = a.lvl_start + (in ? i : 0);
    bool desc = false;
    int32_t split = -1;
    float conf = 0.f;
    uint32_t cmask = 0u;
    if (in) {
      const DecisionRec &d = a.dec[i];
      split = d.split_mode;
      conf = d.confidence;
      if (a.cand) cmask = a.cand[i].mask;
      else {
        // the default policy's record without asking the heads launch for it: the argmax alone, every class when a logit of the decision head is NaN (head_candidates)
        const float *l = a.logits + (size_t)i * a.n_logits + a.head_off;
        bool nan = false;
        for (int k = 0; k < a.head_classes; ++k) nan = nan || (l[k] != l[k]);
        cmask = nan ? (1u << a.head_classes) - 1u : 1u << d.raw_mode;
      }
      desc = a.by_candidates ? (cmask & a.descend_mask) != 0u : (split >= 0 && ((a.descend_mask >> split) & 1u) != 0u);
    }
    const unsigned long long b = __ballot(desc);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(b);
    __syncthreads();
    int woff = 0, total = 0;
    for (int w = 0; w < MLT_TREE_TILE / 64; ++w) {
      const int s = wave_total[w];
      woff += w < wave ? s : 0;
      total += s;
    }
    __syncthreads();   // (the next tile overwrites wave_total)
    if (in) {
      int first_child = -1;
      if (desc) {
        const int fc = child_start + 4 * (base + woff + before);
        if (fc + 3 < a.node_cap) {
          first_child = fc;
          const int x = a.xy[2 * (size_t)node], y = a.xy[2 * (size_t)node + 1];
          for (int j = 0; j < 4; ++j) tree_write_node(a, fc + j, x + (j & 1) * child_size, y + (j >> 1) * child_size, child_size, a.depth + 1, 0, node);
        }
      }
      TreeNodeRec &r = a.nodes[node];
      r.first_child = first_child; r.split_mode = split; r.confidence = conf; r.cand_mask = cmask;
    }
    base += total;
  }
  if (tid == 0 && a.count) a.count[0] = a.n_next_roots + 4 * base;
}

// One work item per 16 x 16 block of every node of the level; the items of a node that has children leave.  Leaves are disjoint, so plain byte stores suffice (the
// map was filled with 0xFF before the first level).
__global__ __launch_bounds__(256) void tree_raster_kernel(const TreeRasterArgs a) {
  const size_t total = (size_t)a.lvl_n << (2 * a.blk_l), step = (size_t)gridDim.x * 256;
  for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < total; it += step) {
    const int i = (int)(it >> (2 * a.blk_l)), b = (int)(it & ((1u << (2 * a.blk_l)) - 1u));
    const TreeNodeRec &r = a.nodes[a.lvl_start + i];
    if (r.first_child >= 0) continue;
    const int mx = (r.x >> 4) + (b & ((1 << a.blk_l) - 1)), my = (r.y >> 4) + (b >> a.blk_l);
    if (mx < 0 || my < 0 || mx >= a.map_w || my >= a.map_h) continue;   // (a node is a complete CU of the picture: never taken)
    a.map[(size_t)my * a.map_w + mx] = (uint8_t)(a.blk_l | ((r.split_mode + 1) << 4));
  }
}
