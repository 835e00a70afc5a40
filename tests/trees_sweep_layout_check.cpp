// Stand-alone check of the union arena of a tree sweep over several pictures (fastintercu-vvc_amd/csrc/mlt_layout.h: Lay::TreeSweepArena with a picture count), built
// and run by tests/test_trees_sweep_cpu.py with g++ -fsanitize=address,undefined, in the manner of tests/tree_sweep_layout_check.cpp.  For 1, 2 and 5 entries x 1, 2
// and 32 points x three geometries x every combination of the optional parts: every part lies inside bytes(), parts are pairwise disjoint, every part starts on
// 256 bytes, has the size written HERE, at(base) is base + offset, the first and last byte of every part can be written, an absent part has no bytes and a NULL
// pointer -- and the addressing: a level's capacity is the entry count times one entry's, the elements (level, point, node) of the per-point parts are pairwise
// distinct and stay inside the part, a level's slab stride is its capacity, and the per-(entry, point) parts (total, first_node, union_nodes, maps) hold every slice.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../fastintercu-vvc_amd/csrc/mlt_layout.h"
#include "../include/mltcnn.h"

using Lay::Field;

static std::string g_what;
[[noreturn]] static void fail(const std::string &msg) {
  std::fprintf(stderr, "FAIL %s: %s\n", g_what.c_str(), msg.c_str());
  std::exit(1);
}

struct Part { const char *name; Field f; size_t want_bytes; bool want_on; const void *ptr; };
struct Geo { int levels; size_t cap[4], roots, map_bytes; };

int main() {
  const size_t NODE = sizeof(mlt_tree_node), DEC = sizeof(mlt_decision), CAND = sizeof(mlt_candidates), ENTRY = 48;   // (ENTRY: the device's entry record)
  if (NODE != 32 || DEC != 48 || CAND != 40 || Lay::TreeSweepArena::kRow != 15 || Lay::TreeSweepArena::kLevels != 4 || MLT_SWEEP_MAX_QPS != 32 || MLT_TREES_MAX_PICTURES != 256)
    fail("record sizes");
  // ONE entry's per-level capacities (W / S)(H / S) / roots of all levels / map bytes: 424 x 280 at 128..16, a 16 x 16 picture at 16, 208 x 176 at 32..16
  const Geo geo[] = {{4, {6, 24, 104, 442}, 40, 442}, {1, {1, 0, 0, 0}, 1, 1}, {2, {30, 143, 0, 0}, 53, 143}};
  const size_t pictures[] = {1, 2, 5}, points[] = {1, 2, 32};
  long checked = 0;
  for (size_t P : pictures)
    for (size_t Q : points)
      for (const Geo &g : geo)
        for (int sw = 0; sw < 64; ++sw) {
          const bool lg = sw & 1, cands = sw & 2, o_map = sw & 4, o_lg = sw & 8, o_dec = sw & 16, o_cand = sw & 32;
          if ((o_lg && !lg) || (o_cand && !cands)) continue;   // (a requested output is made from its slabs)
          char tag[160];
          std::snprintf(tag, sizeof tag, "entries %zu points %zu levels %d lg %d cands %d out %d%d%d%d", P, Q, g.levels, lg, cands, o_map, o_lg, o_dec, o_cand);
          g_what = tag;
          const Lay::TreeSweepArena a(Q, g.levels, g.cap, g.roots, g.map_bytes, lg, cands, o_map, o_lg, o_dec, o_cand, P, ENTRY);
          size_t n = 0;
          for (int l = 0; l < g.levels; ++l) {
            if (a.off[l] != n || a.cap[l] != P * g.cap[l]) fail("level offsets");
            n += P * g.cap[l];
          }
          if (a.n != n || a.n_qps != Q || a.pics != P) fail("node count");
          const size_t QN = Q * n, PQ = P * Q, bytes = a.bytes();
          if (bytes % 256) fail("size is no multiple of 256");
          char *base = (char *)std::aligned_alloc(256, bytes);
          if (!base) fail("allocation");
          const Lay::TreeSweepArena::Ptrs p = a.at(base);
          const std::vector<Part> parts = {
              {"nodes", a.nodes, n * NODE, true, p.nodes}, {"xy", a.xy, n * 8, true, p.xy}, {"alive", a.alive, n * 4, true, p.alive}, {"desc", a.desc, n * 4, true, p.desc},
              {"dec", a.dec, QN * DEC, true, p.dec}, {"logits", a.logits, QN * 15 * 4, lg, p.logits}, {"cand", a.cand, QN * CAND, cands, p.cand},
              {"roots", a.roots, g.roots * 8, true, p.roots}, {"count", a.count, 4, true, p.count}, {"idx", a.idx, QN * 4, true, p.idx}, {"total", a.total, PQ * 4, true, p.total},
              {"first_node", a.first_node, (PQ + 1) * 4, true, p.first_node}, {"union_nodes", a.union_nodes, P * 16, true, p.union_nodes},
              {"map", a.map, PQ * g.map_bytes, o_map, p.map},
              {"o_nodes", a.o_nodes, QN * NODE, true, p.o_nodes}, {"o_logits", a.o_logits, QN * 15 * 4, o_lg, p.o_logits}, {"o_dec", a.o_dec, QN * DEC, o_dec, p.o_dec},
              {"o_cand", a.o_cand, QN * CAND, o_cand, p.o_cand},
              {"pic", a.pic, n * 4, true, p.pic}, {"seg_start", a.seg_start, 4 * P * 4, true, p.seg_start}, {"seg_n", a.seg_n, 4 * P * 4, true, p.seg_n},
              {"entries", a.entries, P * ENTRY, P > 1, p.entries}};
          size_t covered = 0;
          for (const Part &x : parts) {
            if (x.f.on != x.want_on) fail(std::string(x.name) + ": present / absent the wrong way round");
            if (!x.f.on) {
              if (x.f.bytes || x.ptr) fail(std::string(x.name) + ": absent part with bytes or a pointer");
              continue;
            }
            if (x.f.bytes != x.want_bytes) fail(std::string(x.name) + ": " + std::to_string(x.f.bytes) + " bytes, expected " + std::to_string(x.want_bytes));
            if (x.f.off % 256) fail(std::string(x.name) + ": not on 256 bytes");
            if (x.f.end() > bytes) fail(std::string(x.name) + ": ends beyond bytes()");
            for (const Part &y : parts)
              if (&y != &x && y.f.on && x.f.bytes && y.f.bytes && x.f.off < y.f.end() && y.f.off < x.f.end()) fail(std::string(x.name) + " overlaps " + y.name);
            if (x.ptr != base + x.f.off) fail(std::string(x.name) + ": at(base) is not base + offset");
            if (x.f.bytes) {
              base[x.f.off] = 1;
              base[x.f.end() - 1] = 1;
            }
            covered = x.f.end() > covered ? x.f.end() : covered;
          }
          if (Lay::up256(covered) != bytes) fail("bytes() is not the end of the last part");   // (every field of the layout is in the list above)
          // the slabs: element (l, q, i) = n_qps * off[l] + q * cap[l] + i, every element exactly once in [0, n_qps * n); i runs over ALL entries' nodes of the level
          std::vector<char> seen(QN, 0);
          for (int l = 0; l < g.levels; ++l) {
            const size_t cap = P * g.cap[l];
            if (a.slab0(l) != Q * a.off[l]) fail("slab0");
            for (size_t q = 0; q < Q; ++q) {
              if (cap && q + 1 < Q && a.element(l, q + 1, 0) - a.element(l, q, 0) != cap) fail("slab stride is not the level's capacity");
              for (size_t i = 0; i < cap; ++i) {
                const size_t e = a.element(l, q, i);
                if (e >= QN) fail("element outside the part");
                if (seen[e]++) fail("two elements share an entry");
              }
            }
            // a level's logits rows are dense from the level's first reserved row: nl <= 15 floats per element stay inside the level's reserve
            const size_t rows_end = a.slab0(l) * 15 + Q * cap * 15;
            if (rows_end > QN * 15 || (l + 1 < g.levels && rows_end != a.slab0(l + 1) * 15)) fail("logits rows leave the level's reserve");
          }
          for (size_t e = 0; e < QN; ++e)
            if (!seen[e]) fail("an entry belongs to no element");
          // the per-slice parts: slice s = p * n_qps + q writes total[s], first_node[s] (and [P * Q]), map s; entry p writes union_nodes[p][0 .. 4) and its rows of
          // the segment table [level][entry]; idx[q][node] for every node
          for (size_t s = 0; s < PQ; ++s) {
            p.total[s] = (int32_t)s;
            p.first_node[s] = (int32_t)s;
            if (o_map && g.map_bytes) { p.map[s * g.map_bytes] = 1; p.map[(s + 1) * g.map_bytes - 1] = 1; }
          }
          p.first_node[PQ] = 0;
          for (size_t e = 0; e < P; ++e)
            for (size_t l = 0; l < 4; ++l) { p.union_nodes[e * 4 + l] = 1; p.seg_start[l * P + e] = 1; p.seg_n[l * P + e] = 1; }
          for (size_t q = 0; q < Q; ++q)
            for (size_t i = 0; i < n; ++i) p.idx[q * n + i] = -1;
          for (size_t i = 0; i < n; ++i) p.pic[i] = 0;
          if (P > 1) { p.entries[0] = 1; p.entries[P * ENTRY - 1] = 1; }
          std::free(base);
          ++checked;
        }
  std::printf("OK %ld arenas\n", checked);
  return 0;
}
