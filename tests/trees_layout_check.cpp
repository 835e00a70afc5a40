// Stand-alone check of the tree arena in mlt_predict_trees' packed shape (fastintercu-vvc_amd/csrc/mlt_layout.h: Lay::TreeArena), built and run by tests/test_trees_cpu.py with
// g++ -fsanitize=address,undefined, in the manner of tests/layouts_check.cpp.  For 1, 2 and 256 pictures, with and without candidate records in the arena and with
// every combination of requested outputs: every part lies inside bytes(), parts are pairwise disjoint, every part starts on 256 bytes, has the size written HERE,
// at(base) is base + offset, the first and last byte of every part can be written, and an absent part has no bytes and a NULL pointer.
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

int main() {
  const size_t NODE = sizeof(mlt_tree_node), DEC = sizeof(mlt_decision), CAND = sizeof(mlt_candidates), ENTRY = 48;
  if (NODE != 32 || DEC != 48 || CAND != 40 || sizeof(mlt_tree_picture) != 24 || Lay::TreeArena::kRow != 15 || Lay::TreeArena::kLevels != 4) fail("record sizes");
  // nodes per picture / roots / map bytes: 424 x 280 (576, 40, 442), a 16 x 16 picture (1, 1, 1), 208 x 176 at 32..16 (173, 53, 143)
  const size_t geo[][3] = {{576, 40, 442}, {1, 1, 1}, {173, 53, 143}};
  const size_t pics[] = {1, 2, 256};
  long checked = 0;
  for (size_t P : pics)
    for (const size_t *g : geo)
      for (int sw = 0; sw < 16; ++sw) {
        const bool cands = sw & 1, o_lg = sw & 2, o_dec = sw & 4, o_cand = sw & 8;
        char tag[128];
        std::snprintf(tag, sizeof tag, "pictures %zu nodes %zu cands %d out %d%d%d", P, g[0], cands, o_lg, o_dec, o_cand);
        g_what = tag;
        const Lay::TreeArena a(P, g[0], g[1], g[2], ENTRY, cands, true, o_lg, o_dec, o_cand);
        const size_t N = P * g[0], bytes = a.bytes();
        if (bytes % 256) fail("size is no multiple of 256");
        char *base = (char *)std::aligned_alloc(256, bytes);
        if (!base) fail("allocation");
        const Lay::TreeArena::Ptrs p = a.at(base);
        const std::vector<Part> parts = {
            {"nodes", a.nodes, N * NODE, true, p.nodes}, {"xy", a.xy, N * 8, true, p.xy}, {"logits", a.logits, N * 15 * 4, true, p.logits}, {"dec", a.dec, N * DEC, true, p.dec},
            {"cand", a.cand, N * CAND, cands, p.cand}, {"roots", a.roots, g[1] * 8, true, p.roots}, {"map", a.map, P * g[2], true, p.map}, {"count", a.count, 4, true, p.count},
            {"pic", a.pic, N * 4, true, p.pic}, {"seg_start", a.seg_start, 4 * P * 4, true, p.seg_start}, {"seg_n", a.seg_n, 4 * P * 4, true, p.seg_n},
            {"pack_base", a.pack_base, 4 * P * 4, true, p.pack_base}, {"first_node", a.first_node, (P + 1) * 4, true, p.first_node}, {"entries", a.entries, P * ENTRY, true, p.entries},
            {"o_nodes", a.o_nodes, N * NODE, true, p.o_nodes}, {"o_logits", a.o_logits, N * 15 * 4, o_lg, p.o_logits}, {"o_dec", a.o_dec, N * DEC, o_dec, p.o_dec},
            {"o_cand", a.o_cand, N * CAND, o_cand, p.o_cand}};
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
          base[x.f.off] = 1;
          base[x.f.end() - 1] = 1;
        }
        std::free(base);
        ++checked;
      }
  std::printf("OK %ld arenas\n", checked);
  return 0;
}
