// Stand-alone check of the host runtime's buffer layouts (fastintercu-vvc_amd/csrc/mlt_layout.h), built and run by tests/test_layouts_cpu.py with
// g++ -fsanitize=address,undefined.  For every layout over a grid of capacities, logit counts, CU sizes and record switches: every part lies inside the layout,
// parts are pairwise disjoint, every part has the alignment the kernels are given today (Pel planes of a set and every part of a staging set, a guard slot and the
// tree arena: 256 bytes; everything else its type's 4), every part has the size written HERE, the pointers of at(base) are base + offset (and the first and last
// byte of every part can be written), and the copies of mlt_predict and of a deferred batch cover exactly the parts they are for, within the sizes the copies
// had before the layouts had one definition each.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../fastintercu-vvc_amd/csrc/mlt_layout.h"
#include "../include/mltcnn.h"

using Lay::Field;

static long g_checked = 0;
static std::string g_what;

[[noreturn]] static void fail(const std::string &msg) {
  std::fprintf(stderr, "FAIL %s: %s\n", g_what.c_str(), msg.c_str());
  std::exit(1);
}

struct Part { const char *name; Field f; size_t want_bytes, align; const void *ptr; };   // ptr: what at(base) gave (NULL: not checked)

static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// inside, disjoint, aligned, sized; with a real buffer behind `base`: pointers and writable ends
static void check_parts(const std::vector<Part> &parts, size_t bytes, char *base) {
  if (bytes % 256) fail("size is no multiple of 256");
  for (const Part &p : parts) {
    if (!p.f.on) {
      if (p.f.bytes) fail(std::string(p.name) + ": absent part with bytes");
      if (p.ptr) fail(std::string(p.name) + ": absent part with a pointer");
      continue;
    }
    if (p.f.bytes != p.want_bytes) fail(std::string(p.name) + ": " + std::to_string(p.f.bytes) + " bytes, expected " + std::to_string(p.want_bytes));
    if (p.f.off % p.align) fail(std::string(p.name) + ": offset " + std::to_string(p.f.off) + " not aligned to " + std::to_string(p.align));
    if (p.f.end() > bytes) fail(std::string(p.name) + ": ends at " + std::to_string(p.f.end()) + " beyond " + std::to_string(bytes));
    for (const Part &q : parts)
      if (&q != &p && q.f.on && p.f.bytes && q.f.bytes && p.f.off < q.f.end() && q.f.off < p.f.end()) fail(std::string(p.name) + " overlaps " + q.name);
    if (base) {
      if (p.ptr != base + p.f.off) fail(std::string(p.name) + ": at(base) is not base + offset");
      if (p.f.bytes) { base[p.f.off] = 1; base[p.f.end() - 1] = 1; }
    }
  }
  ++g_checked;
}

// [lo, hi) covers exactly the parts named in `in` (no gap, nothing else of the layout inside)
static void check_cover(const std::vector<Part> &parts, const std::vector<std::string> &in, size_t lo, size_t hi, const char *what) {
  size_t sum = 0;
  for (const Part &p : parts) {
    bool wanted = false;
    for (const std::string &n : in) wanted = wanted || n == p.name;
    if (wanted) {
      if (!p.f.on || p.f.off < lo || p.f.end() > hi) fail(std::string(what) + " does not hold " + p.name);
      sum += p.f.bytes;
    } else if (p.f.on && p.f.bytes && p.f.off < hi && lo < p.f.end()) fail(std::string(what) + " holds " + p.name);
  }
  if (sum != hi - lo) fail(std::string(what) + ": " + std::to_string(hi - lo) + " bytes for parts of " + std::to_string(sum));
}

struct Buffer {   // a real allocation behind layouts of up to 64 MiB (base 256-byte aligned like hipMalloc's), none behind the larger ones
  char *p = nullptr;
  explicit Buffer(size_t bytes) { if (bytes <= (64u << 20)) p = (char *)std::aligned_alloc(256, bytes); }
  ~Buffer() { std::free(p); }
};

int main() {
  const size_t DEC = sizeof(mlt_decision), CAND = sizeof(mlt_candidates), NODE = sizeof(mlt_tree_node);
  if (DEC != 48 || CAND != 40 || NODE != 32) fail("record sizes");
  const size_t caps[] = {1, 3, 8, 64, 512, 4096}, nls[] = {9, 15}, sizes[] = {128, 64, 32, 16};
  char tag[160];
  for (size_t cap : caps)
    for (size_t nl : nls) {
      for (int rec = 0; rec < 2; ++rec)
        for (int cnd = 0; cnd < 2; ++cnd) {
          for (size_t S : sizes) {
            std::snprintf(tag, sizeof tag, "StageSet S=%zu cap=%zu nl=%zu rec=%d cand=%d", S, cap, nl, rec, cnd);
            g_what = tag;
            const Lay::StageSet L((int)S, cap, nl, rec != 0, cnd != 0);
            Buffer buf(L.bytes());
            const Lay::CuFields::Ptrs P = buf.p ? L.at(buf.p) : Lay::CuFields::Ptrs{};
            if (L.dec.on != (rec != 0) || L.cand.on != (cnd != 0)) fail("records / candidate records not as asked");
            check_parts({{"org", L.org, cap * S * S * 2, 256, P.d_org}, {"pred", L.pred, cap * S * S * 2, 256, P.d_pred}, {"poc", L.poc, cap * 4, 256, P.d_poc},
                         {"qp", L.qp, cap * 4, 256, P.d_qp}, {"split", L.split, cap * 4, 256, P.d_split}, {"lg", L.lg, cap * nl * 4, 256, P.d_lg},
                         {"dec", L.dec, cap * DEC, 256, P.d_dec}, {"cand", L.cand, cap * CAND, 256, P.d_cand}}, L.bytes(), buf.p);
          }
          std::snprintf(tag, sizeof tag, "ResultSet cap=%zu nl=%zu rec=%d cand=%d", cap, nl, rec, cnd);
          g_what = tag;
          const Lay::ResultSet R(cap, nl, rec != 0, cnd != 0);
          Buffer buf(R.bytes());
          const Lay::CuFields::Ptrs P = buf.p ? R.at(buf.p) : Lay::CuFields::Ptrs{};
          if (R.org.on || R.pred.on || R.poc.on || R.qp.on || R.dec.on != (rec != 0) || R.cand.on != (cnd != 0)) fail("parts not as asked");
          check_parts({{"split", R.split, cap * 4, 4, P.d_split}, {"lg", R.lg, cap * nl * 4, 4, P.d_lg}, {"dec", R.dec, cap * DEC, 4, P.d_dec}, {"cand", R.cand, cap * CAND, 4, P.d_cand}},
                      R.bytes(), buf.p);
        }
      {
        std::snprintf(tag, sizeof tag, "GuardLay n=%zu nl=%zu", cap, nl);
        g_what = tag;
        const Lay::GuardLay G(cap, nl);
        Buffer buf(G.bytes());
        const Lay::GuardFields::Ptrs P = buf.p ? G.at(buf.p) : Lay::GuardFields::Ptrs{};
        if (G.n != cap || G.nl != nl) fail("capacity not recorded");
        check_parts({{"flat", G.flat, cap * 4, 256, P.flat}, {"idx", G.idx, cap * 4, 256, P.idx}, {"count", G.count, 8, 256, P.count}, {"lg", G.lg, cap * nl * 4, 256, P.lg},
                     {"mag", G.mag, cap * 4, 256, P.mag}}, G.bytes(), buf.p);
      }
      {
        std::snprintf(tag, sizeof tag, "DeferOut cap=%zu nl=%zu", cap, nl);
        g_what = tag;
        const Lay::DeferOut O(cap, nl);
        Buffer buf(O.bytes());
        const Lay::CuFields::Ptrs P = buf.p ? O.at(buf.p) : Lay::CuFields::Ptrs{};
        const Lay::GuardFields::Ptrs Q = buf.p ? O.g.at(buf.p) : Lay::GuardFields::Ptrs{};
        if (O.g.lg.off != O.lg.off || O.g.lg.bytes != O.lg.bytes) fail("the guards' logits are not the batch's");
        if (O.org.on || O.pred.on || O.poc.on || O.qp.on) fail("inputs in the output set");
        if (buf.p && Q.lg != P.d_lg) fail("the guards' logits pointer is not the batch's");
        const std::vector<Part> parts = {{"split", O.split, cap * 4, 4, P.d_split}, {"lg", O.lg, cap * nl * 4, 4, P.d_lg}, {"count", O.g.count, 64, 4, Q.count},
                                         {"dec", O.dec, cap * DEC, 4, P.d_dec}, {"cand", O.cand, cap * CAND, 4, P.d_cand}, {"flat", O.g.flat, cap * 4, 4, Q.flat},
                                         {"idx", O.g.idx, cap * 4, 4, Q.idx}, {"mag", O.g.mag, cap * 4, 4, Q.mag}};
        check_parts(parts, O.bytes(), buf.p);
        // the batch's one D2H: split modes, logits, the counter pair and the records -- with the candidate records only when the batch carries them
        check_cover(parts, {"split", "lg", "count", "dec"}, 0, O.fetch_bytes(false), "the fetch without candidate records");
        check_cover(parts, {"split", "lg", "count", "dec", "cand"}, 0, O.fetch_bytes(true), "the fetch with candidate records");
        // what the copy was before: CAP * 4 * (1 + nl) + 64 + CAP * (48 [+ 40])
        if (O.fetch_bytes(false) > cap * 4 * (1 + nl) + 64 + cap * 48 || O.fetch_bytes(true) > cap * 4 * (1 + nl) + 64 + cap * 88) fail("the fetch grew");
      }
      for (size_t S : sizes) {
        std::snprintf(tag, sizeof tag, "DeferIn S=%zu cap=%zu", S, cap);
        g_what = tag;
        const Lay::DeferIn I(S, cap);
        Buffer buf(I.bytes());
        const Lay::CuFields::Ptrs P = buf.p ? I.at(buf.p) : Lay::CuFields::Ptrs{};
        if (I.plane != up256(S * S * 2)) fail("plane pitch");
        const std::vector<Part> parts = {{"org", I.org, cap * I.plane, 256, P.d_org}, {"pred", I.pred, cap * I.plane, 256, P.d_pred}, {"poc", I.poc, cap * 4, 4, P.d_poc},
                                         {"qp", I.qp, cap * 4, 4, P.d_qp}};
        check_parts(parts, I.bytes(), buf.p);
        check_cover(parts, {"poc", "qp"}, I.scalars().off, I.scalars().end(), "the copy of poc and qp");
      }
    }
  for (size_t nl : nls)
    for (size_t S : sizes) {
      std::snprintf(tag, sizeof tag, "SingleLay S=%zu nl=%zu", S, nl);
      g_what = tag;
      const Lay::SingleLay L(S, nl);
      Buffer buf(L.bytes());
      const Lay::CuFields::Ptrs P = L.at(buf.p);
      const Lay::GuardFields::Ptrs Q = L.g.at(buf.p);
      if (L.g.lg.off != L.lg.off || L.g.lg.bytes != L.lg.bytes || Q.lg != P.d_lg) fail("the guards' logits are not the call's");
      const std::vector<Part> parts = {{"org", L.org, S * S * 2, 256, P.d_org}, {"pred", L.pred, S * S * 2, 256, P.d_pred}, {"poc", L.poc, 4, 4, P.d_poc}, {"qp", L.qp, 4, 4, P.d_qp},
                                       {"split", L.split, 4, 4, P.d_split}, {"count", L.g.count, 4, 4, Q.count}, {"lg", L.lg, nl * 4, 4, P.d_lg}, {"dec", L.dec, DEC, 4, P.d_dec},
                                       {"cand", L.cand, CAND, 4, P.d_cand}, {"flat", L.g.flat, 4, 4, Q.flat}, {"idx", L.g.idx, 4, 4, Q.idx}, {"mag", L.g.mag, 4, 4, Q.mag}};
      check_parts(parts, L.bytes(), buf.p);
      // one H2D: the planes (each padded to 256 bytes), poc, qp -- at most 2 * plane + 8 bytes
      const size_t plane = up256(S * S * 2);
      if (L.h2d_bytes() > 2 * plane + 8) fail("the H2D grew");
      for (const Part &p : parts) {
        const bool up = !std::strcmp(p.name, "org") || !std::strcmp(p.name, "pred") || !std::strcmp(p.name, "poc") || !std::strcmp(p.name, "qp");
        if (up ? p.f.end() > L.h2d_bytes() : p.f.off < L.h2d_bytes()) fail(std::string("the H2D and ") + p.name);
      }
      // one D2H per call kind: exactly the host-visible parts, at most (2 + nl) * 4, 34 * 4 and 44 * 4 bytes (the copies before the layouts had one definition)
      const Field plain = L.fetch(false, false), dec = L.fetch(true, false), cand = L.fetch(true, true);
      check_cover(parts, {"split", "count", "lg"}, plain.off, plain.end(), "the plain call's D2H");
      check_cover(parts, {"split", "count", "lg", "dec"}, dec.off, dec.end(), "the decision call's D2H");
      check_cover(parts, {"split", "count", "lg", "dec", "cand"}, cand.off, cand.end(), "the candidate call's D2H");
      if (L.fetch(false, true).bytes != cand.bytes) fail("a candidate call always brings the decision record");
      if (plain.bytes > (2 + nl) * 4 || dec.bytes > 34 * 4 || cand.bytes > 44 * 4) fail("a D2H grew");
      const Field sc = L.scalars();
      if (sc.off != L.poc.off || sc.end() != L.bytes()) fail("scalars() is not everything behind the planes");
    }
  const size_t trees[][3] = {{0, 0, 1}, {1, 1, 1}, {85, 21, 64}, {5461, 4096, 4096}, {1u << 20, 1u << 16, 1u << 20}};   // nodes, roots, map bytes
  for (const size_t(&t)[3] : trees)
    for (int cnd = 0; cnd < 2; ++cnd) {
      std::snprintf(tag, sizeof tag, "TreeArena nodes=%zu roots=%zu map=%zu cand=%d", t[0], t[1], t[2], cnd);
      g_what = tag;
      // the single call's shape: one picture, not packed (whatever outputs the caller wants: they come straight from the level-major parts)
      const Lay::TreeArena A(1, t[0], t[1], t[2], 48, cnd != 0, false, cnd != 0, true, cnd == 0);
      Buffer buf(A.bytes());
      const Lay::TreeArena::Ptrs P = buf.p ? A.at(buf.p) : Lay::TreeArena::Ptrs{};
      if (A.cand.on != (cnd != 0)) fail("candidate records not as asked");
      const std::vector<Part> absent = {{"entries", A.entries, 0, 256, P.entries}, {"o_nodes", A.o_nodes, 0, 256, P.o_nodes}, {"o_logits", A.o_logits, 0, 256, P.o_logits},
                                        {"o_dec", A.o_dec, 0, 256, P.o_dec}, {"o_cand", A.o_cand, 0, 256, P.o_cand}};
      for (const Part &p : absent)
        if (p.f.on || p.f.bytes || p.ptr) fail(std::string(p.name) + ": present in the single call's arena");
      check_parts({{"nodes", A.nodes, t[0] * NODE, 256, P.nodes}, {"xy", A.xy, t[0] * 8, 256, P.xy}, {"logits", A.logits, t[0] * MLT_MAX_LOGITS * 4, 256, P.logits},
                   {"dec", A.dec, t[0] * DEC, 256, P.dec}, {"cand", A.cand, t[0] * CAND, 256, P.cand}, {"roots", A.roots, t[1] * 8, 256, P.roots}, {"map", A.map, t[2], 256, P.map},
                   {"count", A.count, 4, 256, P.count}, {"pic", A.pic, t[0] * 4, 256, P.pic}, {"seg_start", A.seg_start, 4 * 4, 256, P.seg_start},
                   {"seg_n", A.seg_n, 4 * 4, 256, P.seg_n}, {"pack_base", A.pack_base, 4 * 4, 256, P.pack_base}, {"first_node", A.first_node, 2 * 4, 256, P.first_node},
                   absent[0], absent[1], absent[2], absent[3], absent[4]}, A.bytes(), buf.p);
    }
  std::printf("OK %ld layouts\n", g_checked);
  return 0;
}
