// mlt_layout.h -- the buffer layouts of the host runtime, each defined ONCE.  A layout is a set of byte offsets (Field) that its constructor carves off one running end
// (Carved::put); its size (bytes()), its device pointers and its pinned-mirror pointers (at(base) serves both) all derive from those offsets.  Plain C++, no HIP
// header: tests/layouts_check.cpp walks every layout under the sanitizers.  Records are sized from the ABI's mlt_decision / mlt_candidates / mlt_tree_node and pointed
// to as the kernels' DecisionRec / CandRec / TreeNodeRec (mlt_kernels.h; mlt_runtime.h asserts they are the same bytes) -- incomplete types here.
// Alignment: the Pel planes of a staging set start on 256 bytes (the quad-fetching kernels want 8); everything else needs its own type's alignment, 4.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mltcnn.h"

struct DecisionRec;
struct CandRec;
struct TreeNodeRec;

namespace Lay {

struct Field {   // one part of a layout; !on: the layout was built without it (no bytes, NULL pointer)
  size_t off = 0, bytes = 0;
  bool on = false;
  size_t end() const { return off + bytes; }
  template <class T> T *in(char *base) const { return on ? (T *)(base + off) : nullptr; }
};
inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }
struct Carved {   // base of every layout: the running end while the constructor carves, the size afterwards
  size_t carved = 0;
  Field put(size_t bytes, size_t align = 4, bool on = true) { carved = (carved + align - 1) / align * align; const Field f{carved, on ? bytes : 0, on}; carved += f.bytes; return f; }
  size_t bytes() const { return up256(carved); }   // (a second set behind the first starts as aligned as the first)
};
// the guards' device state of one batch (GuardSlot): wherever a layout puts the five parts, the pointers come from here
struct GuardFields {
  struct Ptrs {
    int32_t *flat, *idx, *count;   // per-CU flat-content statistic | list of the flagged CUs | their count (batches: a pair of counters, GuardSlot.phase)
    float *lg, *mag;               // logits for the margin test when the caller wants none | per-CU logit magnitude (HeadArgs.mag) for the magnitude guard
  };
  Field flat, idx, count, lg, mag;
  Ptrs at(char *base) const { return Ptrs{flat.in<int32_t>(base), idx.in<int32_t>(base), count.in<int32_t>(base), lg.in<float>(base), mag.in<float>(base)}; }
};
// what a pass reads and writes per CU, as parts of one buffer (a layout that has no such part leaves it off)
struct CuFields : Carved {
  struct Ptrs { int16_t *d_org, *d_pred; int32_t *d_poc, *d_qp, *d_split; float *d_lg; DecisionRec *d_dec; CandRec *d_cand; };
  Field org, pred, poc, qp, split, lg, dec, cand;
  Ptrs at(char *b) const {
    return Ptrs{org.in<int16_t>(b), pred.in<int16_t>(b), poc.in<int32_t>(b), qp.in<int32_t>(b), split.in<int32_t>(b), lg.in<float>(b), dec.in<DecisionRec>(b), cand.in<CandRec>(b)};
  }
};

// One staging set for `cap` dense CUs in device memory: org | pred | poc | qp | split | logits [| records] [| candidate records], every part on 256 bytes.
struct StageSet : CuFields {
  StageSet(int S, size_t cap, size_t nl, bool records, bool cands = false) {
    org = put(cap * S * S * 2, 256); pred = put(cap * S * S * 2, 256); poc = put(cap * 4, 256); qp = put(cap * 4, 256); split = put(cap * 4, 256); lg = put(cap * nl * 4, 256);
    dec = put(cap * sizeof(mlt_decision), 256, records); cand = put(cap * sizeof(mlt_candidates), 256, cands);
  }
};
// A guard slot of its own (guard_slot(): batches whose results live in the caller's or a staging set's memory), for up to n CUs of nl logits.
struct GuardLay : GuardFields, Carved {
  size_t n, nl;
  GuardLay(size_t n_ = 0, size_t nl_ = 0) : n(n_), nl(nl_) { flat = put(n * 4, 256); idx = put(n * 4, 256); count = put(8, 256); lg = put(n * nl * 4, 256); mag = put(n * 4, 256); }
};
// QP sweeps (mlt_predict_at_sweep): a staging set whose result parts hold n_qps slabs of `cap` CUs each -- org | pred | poc | split | logits [| records]
// [| candidate records]; element (q, i) of a result part is entry q * cap + i (slab stride: cap).  No qp part: the points' values travel in the launch.
struct SweepStageSet : CuFields {
  size_t cap, n_qps;
  SweepStageSet(int S, size_t cap_, size_t nl, size_t n_qps_, bool records, bool cands) : cap(cap_), n_qps(n_qps_) {
    org = put(cap * S * S * 2, 256); pred = put(cap * S * S * 2, 256); poc = put(cap * 4, 256); split = put(n_qps * cap * 4, 256); lg = put(n_qps * cap * nl * 4, 256);
    dec = put(n_qps * cap * sizeof(mlt_decision), 256, records); cand = put(n_qps * cap * sizeof(mlt_candidates), 256, cands);
  }
};
// The guard slot of a sweep pass for up to n CUs: flat | idx | count (a pair of counters) | mask (per CU: bit q set = flagged under point q).  The selection is
// always the sweep heads kernel's tail: no logits or magnitudes are kept for a selection launch.
struct SweepGuardLay : GuardFields, Carved {
  size_t n;
  Field mask;
  SweepGuardLay(size_t n_ = 0) : n(n_) { flat = put(n * 4, 256); idx = put(n * 4, 256); count = put(8, 256); mask = put(n * 4, 256); }
};
// mlt_predict's staging (device buffer and its pinned mirror): org | pred | poc qp | split count logits record candidate-record | flat idx mag.  One H2D brings planes,
// poc and qp (h2d_bytes); one D2H takes the host-visible prefix from `split` on back, as far as the call's kind needs (fetch).  The guards select on g.
struct SingleLay : CuFields {
  GuardFields g;
  SingleLay(size_t S = 0, size_t nl = 0) {
    org = put(S * S * 2, 256); pred = put(S * S * 2, 256); poc = put(4); qp = put(4);
    split = put(4); g.count = put(4); lg = g.lg = put(nl * 4); dec = put(sizeof(mlt_decision)); cand = put(sizeof(mlt_candidates));
    g.flat = put(4); g.idx = put(4); g.mag = put(4);
  }
  size_t h2d_bytes() const { return qp.end(); }
  Field scalars() const { return Field{poc.off, bytes() - poc.off, true}; }   // everything behind the planes
  Field fetch(bool want_dec, bool want_cand) const { return Field{split.off, (want_cand ? cand : want_dec ? dec : lg).end() - split.off, true}; }
};
// One input set of the deferred API (device and pinned): org planes | pred planes | poc | qp for `cap` CUs, a CU's plane every `plane` bytes.
struct DeferIn : CuFields {
  size_t plane;
  DeferIn(size_t S = 0, size_t cap = 0) : plane(up256(S * S * 2)) { org = put(cap * plane, 256); pred = put(cap * plane, 256); poc = put(cap * 4); qp = put(cap * 4); }
  Field scalars() const { return Field{poc.off, qp.end() - poc.off, true}; }   // poc and qp travel in one copy
};
// One output set of the deferred API (device and pinned): split | logits | flagged count (a pair of counters in 64 bytes) | records | candidate records | flat idx mag.
// A batch always carries its CUs' decision records (whether a ticket is read with mlt_wait or mlt_wait_decision is not known at launch); the candidate records are
// filled and fetched only by batches launched once the size has a policy or has seen a candidate call.  The batch's one D2H takes the prefix fetch_bytes(cand).
struct DeferOut : CuFields {
  GuardFields g;
  DeferOut(size_t cap = 0, size_t nl = 0) {
    split = put(cap * 4); lg = g.lg = put(cap * nl * 4); g.count = put(64); dec = put(cap * sizeof(mlt_decision)); cand = put(cap * sizeof(mlt_candidates));
    g.flat = put(cap * 4); g.idx = put(cap * 4); g.mag = put(cap * 4);
  }
  size_t fetch_bytes(bool with_cand) const { return (with_cand ? cand : dec).end(); }
};
// One pinned result set of mlt_predict_batch: split | logits [| records] [| candidate records] of a sub-chunk of up to `cap` CUs.
struct ResultSet : CuFields {
  ResultSet(size_t cap, size_t nl, bool records, bool cands) {
    split = put(cap * 4); lg = put(cap * nl * 4); dec = put(cap * sizeof(mlt_decision), 4, records); cand = put(cap * sizeof(mlt_candidates), 4, cands);
  }
};
// The device arena of a tree call (mlt_predict_tree: pics = 1, !packed; mlt_predict_trees: packed) for `pics` pictures of up to n nodes each, indexed by node and
// LEVEL-major (a level of all pictures is one node range): nodes | xy | logits (kRow floats per node) | records [| candidate records] | roots | one leaf map per
// picture | count | the per-node picture index | the segment table ([kLevels][pics]: start, count, start in the output) | first_node [pics + 1]; packed: | the entry
// table (entry_bytes each) | the picture-major output: nodes [| logits] [| records] [| candidate records].
struct TreeArena : Carved {
  static const int kRow = MLT_MAX_LOGITS, kLevels = 4;
  struct Ptrs {
    TreeNodeRec *nodes; int32_t *xy; float *logits; DecisionRec *dec; CandRec *cand; int32_t *roots; uint8_t *map; int32_t *count;
    int32_t *pic, *seg_start, *seg_n, *pack_base, *first_node; char *entries;
    TreeNodeRec *o_nodes; float *o_logits; DecisionRec *o_dec; CandRec *o_cand;
  };
  Field nodes, xy, logits, dec, cand, roots, map, count, pic, seg_start, seg_n, pack_base, first_node, entries, o_nodes, o_logits, o_dec, o_cand;
  TreeArena(size_t pics, size_t n, size_t n_roots, size_t map_bytes, size_t entry_bytes, bool cands, bool packed, bool out_logits, bool out_dec, bool out_cand) {
    const size_t N = pics * n;
    nodes = put(N * sizeof(mlt_tree_node), 256); xy = put(N * 8, 256); logits = put(N * kRow * 4, 256); dec = put(N * sizeof(mlt_decision), 256);
    cand = put(N * sizeof(mlt_candidates), 256, cands); roots = put(n_roots * 8, 256); map = put(pics * map_bytes, 256); count = put(4, 256);
    pic = put(N * 4, 256); seg_start = put(kLevels * pics * 4, 256); seg_n = put(kLevels * pics * 4, 256); pack_base = put(kLevels * pics * 4, 256);
    first_node = put((pics + 1) * 4, 256); entries = put(pics * entry_bytes, 256, packed);
    o_nodes = put(N * sizeof(mlt_tree_node), 256, packed); o_logits = put(N * kRow * 4, 256, packed && out_logits); o_dec = put(N * sizeof(mlt_decision), 256, packed && out_dec);
    o_cand = put(N * sizeof(mlt_candidates), 256, packed && out_cand);
  }
  Ptrs at(char *b) const {
    return Ptrs{nodes.in<TreeNodeRec>(b), xy.in<int32_t>(b), logits.in<float>(b), dec.in<DecisionRec>(b), cand.in<CandRec>(b), roots.in<int32_t>(b), map.in<uint8_t>(b),
                count.in<int32_t>(b), pic.in<int32_t>(b), seg_start.in<int32_t>(b), seg_n.in<int32_t>(b), pack_base.in<int32_t>(b), first_node.in<int32_t>(b),
                entries.in<char>(b), o_nodes.in<TreeNodeRec>(b), o_logits.in<float>(b), o_dec.in<DecisionRec>(b), o_cand.in<CandRec>(b)};
  }
};
// The device arena of a tree SWEEP (mlt_predict_tree_sweep: pics = 1; mlt_predict_trees_sweep): the UNION of the trees of each of `pics` entries of one geometry
// under n_qps points, LEVEL-major, every level at its full capacity -- level l holds up to cap[l] = pics (W / S)(H / S) nodes from node off[l] = cap[0] + .. +
// cap[l - 1] on (n = off[levels]); inside a level entry 0's union segment, entry 1's, ... (the segment table).  Per union node: nodes | xy | alive (bit q: the node
// is part of its entry's tree q) | desc (bit q: it descends under point q).  The per-node outputs of a level are SLAB-major over the points: element (l, q, i) of
// records [| logits, kRow floats reserved per element, a level's rows dense] [| candidate records] is entry n_qps * off[l] + q * cap[l] + i -- the sweep pass
// writes level l with slab stride cap[l].  Then roots | count | idx [n_qps][n] (a node's index inside its entry's slice q) | total [pics * n_qps] | first_node
// [pics * n_qps + 1] | union_nodes [pics][kLevels] [| one leaf map per (entry, point)] | the packed output: nodes [| logits] [| records] [| candidate records],
// n_qps * n each | pic (a node's entry) | the segment table ([kLevels][pics]: start, count) [| the entry table, entry_bytes each: pics > 1].
struct TreeSweepArena : Carved {
  static const int kRow = MLT_MAX_LOGITS, kLevels = 4;
  struct Ptrs {
    TreeNodeRec *nodes; int32_t *xy; uint32_t *alive, *desc; DecisionRec *dec; float *logits; CandRec *cand; int32_t *roots, *count, *idx, *total, *first_node, *union_nodes;
    uint8_t *map; TreeNodeRec *o_nodes; float *o_logits; DecisionRec *o_dec; CandRec *o_cand;
    int32_t *pic, *seg_start, *seg_n; char *entries;
  };
  size_t n_qps, n, off[kLevels + 1], cap[kLevels], pics;
  Field nodes, xy, alive, desc, dec, logits, cand, roots, count, idx, total, first_node, union_nodes, map, o_nodes, o_logits, o_dec, o_cand, pic, seg_start, seg_n, entries;
  // lvl_cap: ONE entry's capacity per level
  TreeSweepArena(size_t n_qps_, int levels, const size_t *lvl_cap, size_t n_roots, size_t map_bytes, bool lg, bool cands, bool out_map, bool out_logits, bool out_dec,
                 bool out_cand, size_t pics_ = 1, size_t entry_bytes = 0) : n_qps(n_qps_), pics(pics_) {
    off[0] = 0;
    for (int l = 0; l < kLevels; ++l) { cap[l] = l < levels ? pics * lvl_cap[l] : 0; off[l + 1] = off[l] + cap[l]; }
    n = off[kLevels];
    const size_t QN = n_qps * n, PQ = pics * n_qps;
    nodes = put(n * sizeof(mlt_tree_node), 256); xy = put(n * 8, 256); alive = put(n * 4, 256); desc = put(n * 4, 256);
    dec = put(QN * sizeof(mlt_decision), 256); logits = put(QN * kRow * 4, 256, lg); cand = put(QN * sizeof(mlt_candidates), 256, cands);
    roots = put(n_roots * 8, 256); count = put(4, 256); idx = put(QN * 4, 256); total = put(PQ * 4, 256); first_node = put((PQ + 1) * 4, 256);
    union_nodes = put(pics * kLevels * 4, 256); map = put(PQ * map_bytes, 256, out_map);
    o_nodes = put(QN * sizeof(mlt_tree_node), 256); o_logits = put(QN * kRow * 4, 256, out_logits); o_dec = put(QN * sizeof(mlt_decision), 256, out_dec);
    o_cand = put(QN * sizeof(mlt_candidates), 256, out_cand);
    pic = put(n * 4, 256); seg_start = put(kLevels * pics * 4, 256); seg_n = put(kLevels * pics * 4, 256); entries = put(pics * entry_bytes, 256, pics > 1);
  }
  size_t slab0(int l) const { return n_qps * off[l]; }                                            // element (l, 0, 0)
  size_t element(int l, size_t q, size_t i) const { return slab0(l) + q * cap[l] + i; }   // slab stride of level l: cap[l]
  Ptrs at(char *b) const {
    return Ptrs{nodes.in<TreeNodeRec>(b), xy.in<int32_t>(b), alive.in<uint32_t>(b), desc.in<uint32_t>(b), dec.in<DecisionRec>(b), logits.in<float>(b), cand.in<CandRec>(b),
                roots.in<int32_t>(b), count.in<int32_t>(b), idx.in<int32_t>(b), total.in<int32_t>(b), first_node.in<int32_t>(b), union_nodes.in<int32_t>(b), map.in<uint8_t>(b),
                o_nodes.in<TreeNodeRec>(b), o_logits.in<float>(b), o_dec.in<DecisionRec>(b), o_cand.in<CandRec>(b),
                pic.in<int32_t>(b), seg_start.in<int32_t>(b), seg_n.in<int32_t>(b), entries.in<char>(b)};
  }
};

}  // namespace Lay
