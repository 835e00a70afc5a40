// Stand-alone check of the QP-sweep buffer layouts (fastintercu-vvc_amd/csrc/mlt_layout.h: SweepStageSet, SweepGuardLay), built and run by
// tests/test_sweep_cpu.py with g++ -fsanitize=address,undefined.  Over Q in {1, 4, 32} points, capacities {1, 7, 4096}, every CU size, both logit counts and
// the record switches: every part lies inside the layout, parts are pairwise disjoint, every part starts on 256 bytes and has the size written HERE, the
// SLABS of every result part are pairwise disjoint, aligned to their element type and the last one ends inside bytes(), at(base) is base + offset, and the
// first and last byte of every slab can be written (a real allocation stands behind every layout of up to 64 MiB).
#include <cstdio>
#include <cstdlib>
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

// slabs: how many slabs of `elem`-byte elements the part holds (1: not a result part); align: of the part's start
struct Part { const char *name; Field f; size_t want_bytes, align, slabs, elem; const void *ptr; };

static void check_parts(const std::vector<Part> &parts, size_t bytes, size_t cap, char *base) {
  if (bytes % 256) fail("size is no multiple of 256");
  for (const Part &p : parts) {
    if (!p.f.on) {
      if (p.f.bytes || p.ptr) fail(std::string(p.name) + ": absent part with bytes or a pointer");
      continue;
    }
    if (p.f.bytes != p.want_bytes) fail(std::string(p.name) + ": " + std::to_string(p.f.bytes) + " bytes, expected " + std::to_string(p.want_bytes));
    if (p.f.off % p.align) fail(std::string(p.name) + ": offset " + std::to_string(p.f.off) + " not aligned to " + std::to_string(p.align));
    if (p.f.end() > bytes) fail(std::string(p.name) + ": ends at " + std::to_string(p.f.end()) + " beyond " + std::to_string(bytes));
    for (const Part &q : parts)
      if (&q != &p && q.f.on && p.f.bytes && q.f.bytes && p.f.off < q.f.end() && q.f.off < p.f.end()) fail(std::string(p.name) + " overlaps " + q.name);
    if (base && p.ptr != base + p.f.off) fail(std::string(p.name) + ": at(base) is not base + offset");
    // the slabs: slab q is [off + q * cap * elem, off + (q + 1) * cap * elem)
    const size_t slab = cap * p.elem;
    if (p.slabs * slab != p.f.bytes) fail(std::string(p.name) + ": the slabs do not fill the part");
    for (size_t q = 0; q < p.slabs; ++q) {
      const size_t lo = p.f.off + q * slab, hi = lo + slab;
      if (lo % 4) fail(std::string(p.name) + ": slab " + std::to_string(q) + " not aligned to its element type");
      if (q + 1 < p.slabs && hi != p.f.off + (q + 1) * slab) fail(std::string(p.name) + ": slabs overlap or leave a gap");
      if (hi > p.f.end() || hi > bytes) fail(std::string(p.name) + ": slab " + std::to_string(q) + " ends beyond the layout");
      if (base) { base[lo] = 1; base[hi - 1] = 1; }
    }
  }
  ++g_checked;
}

struct Buffer {   // a real allocation behind layouts of up to 64 MiB (base 256-byte aligned like hipMalloc's), none behind the larger ones
  char *p = nullptr;
  explicit Buffer(size_t bytes) { if (bytes <= (64u << 20)) p = (char *)std::aligned_alloc(256, bytes); }
  ~Buffer() { std::free(p); }
};

int main() {
  const size_t DEC = sizeof(mlt_decision), CAND = sizeof(mlt_candidates);
  if (DEC != 48 || CAND != 40 || MLT_SWEEP_MAX_QPS != 32) fail("record sizes / MLT_SWEEP_MAX_QPS");
  const size_t caps[] = {1, 7, 4096}, qs[] = {1, 4, 32}, nls[] = {9, 15}, sizes[] = {128, 64, 32, 16};
  char tag[160];
  for (size_t cap : caps) {
    for (size_t Q : qs)
      for (size_t nl : nls)
        for (size_t S : sizes)
          for (int rec = 0; rec < 2; ++rec)
            for (int cnd = 0; cnd < 2; ++cnd) {
              std::snprintf(tag, sizeof tag, "SweepStageSet(S %zu, cap %zu, nl %zu, Q %zu, rec %d, cand %d)", S, cap, nl, Q, rec, cnd);
              g_what = tag;
              const Lay::SweepStageSet l((int)S, cap, nl, Q, rec != 0, cnd != 0);
              if (l.cap != cap || l.n_qps != Q) fail("cap / n_qps");
              if (l.qp.on) fail("a sweep set has no qp part");
              Buffer buf(l.bytes());
              const Lay::SweepStageSet::Ptrs p = l.at(buf.p);
              const std::vector<Part> parts = {
                  {"org", l.org, cap * S * S * 2, 256, 1, S * S * 2, buf.p ? p.d_org : nullptr},
                  {"pred", l.pred, cap * S * S * 2, 256, 1, S * S * 2, buf.p ? p.d_pred : nullptr},
                  {"poc", l.poc, cap * 4, 256, 1, 4, buf.p ? p.d_poc : nullptr},
                  {"split", l.split, Q * cap * 4, 256, Q, 4, buf.p ? p.d_split : nullptr},
                  {"logits", l.lg, Q * cap * nl * 4, 256, Q, nl * 4, buf.p ? p.d_lg : nullptr},
                  {"records", l.dec, Q * cap * DEC, 256, Q, DEC, buf.p ? (const void *)p.d_dec : nullptr},
                  {"candidates", l.cand, Q * cap * CAND, 256, Q, CAND, buf.p ? (const void *)p.d_cand : nullptr},
              };
              if (l.dec.on != (rec != 0) || l.cand.on != (cnd != 0)) fail("record switches");
              check_parts(parts, l.bytes(), cap, buf.p);
              // bytes() covers the last slab of the last part
              const Field &last = cnd ? l.cand : rec ? l.dec : l.lg;
              if (last.off + (Q - 1) * (last.bytes / Q) + last.bytes / Q > l.bytes()) fail("bytes() does not cover the last slab");
            }
    std::snprintf(tag, sizeof tag, "SweepGuardLay(n %zu)", cap);
    g_what = tag;
    const Lay::SweepGuardLay g(cap);
    if (g.n != cap || g.lg.on || g.mag.on) fail("n / parts a sweep slot does not have");
    Buffer buf(g.bytes());
    const Lay::GuardFields::Ptrs p = g.at(buf.p);
    // (per-CU arrays: one "slab" of cap elements; the counter pair: 8 bytes whatever the capacity, written here as cap elements of 8 / cap bytes would not
    // divide, so it is checked on its own with a capacity of 1)
    const std::vector<Part> per_cu = {
        {"flat", g.flat, cap * 4, 256, 1, 4, buf.p ? p.flat : nullptr},
        {"idx", g.idx, cap * 4, 256, 1, 4, buf.p ? p.idx : nullptr},
        {"mask", g.mask, cap * 4, 256, 1, 4, buf.p ? g.mask.in<uint32_t>(buf.p) : nullptr},
    };
    const Part count = {"count", g.count, 8, 256, 1, 8, buf.p ? p.count : nullptr};
    check_parts(per_cu, g.bytes(), cap, buf.p);
    --g_checked;   // (the slot counts once)
    check_parts({count}, g.bytes(), 1, buf.p);
    for (const Part &a : per_cu)
      if (a.f.off < count.f.end() && count.f.off < a.f.end()) fail(std::string(a.name) + " overlaps count");
    if (p.lg || p.mag) fail("pointers of absent parts");
  }
  std::printf("OK %ld layouts\n", g_checked);
  return 0;
}
