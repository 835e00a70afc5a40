"""GPU (MI355X): partition trees of several picture pairs under several QPs each from ONE union descent -- mlt_predict_trees_sweep against its twin,
mlt_predict_trees over the P x Q entries {org_p, pred_p, poc_p, qp_p + qps[q]} in that order, on the same context.

Every assertion between the two is BYTE equality, all result buffers zero-filled first: every slice's nodes, first_node, the leaf maps, the logits (whole rows),
the decision and the candidate records.  union_nodes[p][l] must be the number of distinct positions of that size over entry p's slices.  With a[p][q] the growth
of guard_reruns under the P x Q single mlt_predict_tree calls: sum_p max_q a[p][q] <= growth under the one call <= sum_{p, q} a[p][q].
Preconditions on the content (which nodes say QT under which point) come from the CPU oracle alone and are printed, never from what the device returns."""
import ctypes as C

import numpy as np
import pytest

from tree_gpu_common import (CHUNK, LOGIT_TOL, MLT_ERR_ARG, MLT_ERR_SIZE_DISABLED, SIZES, TREE_ALL, H, W, Pair, blobs as _blobs, contexts, cut, gpu, naturals,   # noqa: F401  (fixtures)
                             open_context as _open, reruns as _reruns, same as _same)

pytestmark = pytest.mark.gpu
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def oracle_roots(pkg, weight_seed, org, pred, poc, qp):
    """The CPU oracle on the six 128 roots of a 424 x 280 picture -> (split [6], the smallest top-2 margin of the decision head); cached."""
    import oracle
    key = (weight_seed, org.tobytes()[:4096], poc, qp)
    if key not in oracle_roots.done:
        net = oracle_roots.nets.setdefault(weight_seed, oracle.Oracle(_blobs(pkg, weight_seed, (128,))[128]))
        xy = pkg.capi.tree_roots(W, H, 128, 128)
        logits, split = net.forward(cut(org, xy, 128), cut(pred, xy, 128), np.full(6, poc, np.int32), np.full(6, qp, np.int32), head_index=0)
        oracle_roots.done[key] = (split.tolist(), float(pkg.decisions.from_logits(128, logits, head_index=0)["margin"].min()))
    return oracle_roots.done[key]


oracle_roots.nets, oracle_roots.done = {}, {}
CLEAR = 4 * LOGIT_TOL   # two logits within LOGIT_TOL of the reference cannot swap over such a margin


def check(m, entries, qps, what, want=TREE_ALL, singles=True, **kw):
    """entries: [(org_pic, pred_pic, poc, qp_offset)].  mlt_predict_trees_sweep == mlt_predict_trees over the P x Q entries, byte for byte; union_nodes per
    entry; guard re-runs between sum_p max_q and sum_{p, q} of the single calls' -> the call's result[p][q]."""
    qps = [int(q) for q in qps]
    P, Q = len(entries), len(qps)
    top, mn = kw.get("top", 128), kw.get("min_size", 16)
    sizes = [s for s in SIZES if mn <= s <= top]
    pairs = [(o, p) for o, p, _, _ in entries]
    r0 = _reruns(m, sizes)
    got = m.predict_trees_sweep(pairs, [e[2] for e in entries], [e[3] for e in entries], qps, want=want, **kw)
    grown = _reruns(m, sizes) - r0
    flat = [(o, p, poc, off + q) for o, p, poc, off in entries for q in qps]
    twin = m.predict_trees([(o, p) for o, p, _, _ in flat], np.array([e[2] for e in flat], np.int32), np.array([e[3] for e in flat], np.int32), want=want, **kw)
    assert len(got) == P and all(len(row) == Q for row in got) and len(twin) == P * Q
    for p in range(P):
        for q in range(Q):
            g, t = got[p][q], twin[p * Q + q]
            assert g["first_node"] == t["first_node"], (what, p, q, g["first_node"], t["first_node"])
            assert len(g["nodes"]) == len(t["nodes"]), (what, p, q, len(g["nodes"]), len(t["nodes"]))
            for f in t["nodes"].dtype.names:
                assert np.array_equal(g["nodes"][f], t["nodes"][f], equal_nan=f == "confidence"), (what, p, q, f, np.flatnonzero(g["nodes"][f] != t["nodes"][f])[:8])
            assert _same(g["nodes"], t["nodes"]), (what, p, q)
            for k in want:
                assert _same(g[k], t[k]), (what, p, q, k)
            assert sorted(g) == sorted(["nodes", "first_node", "union_nodes"] + list(want)), sorted(g)
        union = got[p][0]["union_nodes"]
        assert union.shape == (4,) and union.dtype == np.int32 and all(np.array_equal(g["union_nodes"], union) for g in got[p])
        for l, s in enumerate(SIZES[SIZES.index(top):]):
            distinct = {(int(x), int(y)) for g in got[p] for x, y in zip(g["nodes"]["x"][g["nodes"]["size"] == s], g["nodes"]["y"][g["nodes"]["size"] == s])}
            assert union[l] == (len(distinct) if s >= mn else 0), (what, p, s, int(union[l]), len(distinct))
    if singles:
        a = []
        for o, pr, poc, off in entries:
            row = []
            for q in qps:
                r1 = _reruns(m, sizes)
                m.predict_tree(o, pr, poc, off + q, want=("leaf_map",), **kw)
                row.append(_reruns(m, sizes) - r1)
            a.append(row)
        print(f"{what}: unions {[got[p][0]['union_nodes'].tolist() for p in range(P)]}, slices {[[len(g['nodes']) for g in row] for row in got]}, "
              f"guard re-runs: the call {grown}, singles {a}")
        assert sum(max(row) for row in a) <= grown <= sum(sum(row) for row in a), (what, "guard re-runs", grown, a)
    return got


def test_diverging_descents_all_four_sizes(gpu, contexts, naturals):
    """Pair A at offset 0, pair A again at offset 32 with another poc, pair B: under (-100, 0, 32) the six 128 roots of A say QT under none / some / all points
    (the oracle), and A's second entry runs point 1 at qp 32 where, by the oracle, all six say QT -- another decided set than the first entry's at point 1."""
    pkg = gpu
    qps, off2, poc2 = (-100, 0, 32), 32, 1
    a_org, a_pred = naturals(1)
    first = [oracle_roots(pkg, 13, a_org, a_pred, 0, q) for q in qps]
    second = [oracle_roots(pkg, 13, a_org, a_pred, poc2, off2 + q) for q in qps]
    print("oracle, weight seed 13, picture seed 1: QT among the six 128 roots, entry 0 (poc 0) under", qps, "->", first, "; entry 1 (poc 1) under",
          tuple(off2 + q for q in qps), "->", second)
    assert sum(first[0][0]) == 0 and sum(first[2][0]) == 6 and 0 < sum(first[1][0]) < 6, first
    assert first[1][0] != second[1][0] and first[1][1] > CLEAR and second[1][1] > CLEAR, (first[1], second[1])
    m = contexts(13)
    with Pair(m, a_org, a_pred) as (ao, ap), Pair(m, *naturals(34791)) as (bo, bp):
        got = check(m, [(ao, ap, 0, 0), (ao, ap, poc2, off2), (bo, bp, 0, 0)], qps, "diverging")
        for e, per_point in ((0, first), (1, second)):
            for q, (split, margin) in enumerate(per_point):
                if margin > CLEAR:
                    n128 = got[e][q]["nodes"][got[e][q]["nodes"]["size"] == 128]
                    assert (n128["first_child"] >= 0).astype(int).tolist() == split, (e, q, split)
        assert not _same(got[0][1]["nodes"], got[1][1]["nodes"])
        assert len(got[0][0]["nodes"]) == 6 + 0 + 8 + 26   # entry 0's slice 0 is the roots alone while its union descends
        assert got[0][0]["union_nodes"][1] == 24 and got[1][0]["union_nodes"][1] == 24


def test_tile_chunk_and_empty_segment_boundaries(gpu, contexts, naturals):
    """ELEVEN entries of one uploaded pair, Q = 2, every class descends at 64 and 32 (descend masks 0b11), the 128 level decides by content: by the oracle every
    128 root says QT under both points of the ten outer entries (offsets 0 and 5 in turn: the points are qp 32 / 37 and 37 / 42), and none under either point of
    entry 5 (offset -132: qp -100 / -95), whose 64 segment is therefore EMPTY -- 424 x 280 has no roots at 64 -- between full ones.  The 16 level is 442 nodes per
    full entry and 58 for entry 5: 10 x 442 + 58 = 4478 nodes, a list that crosses the scan's tiles at 1024, 2048, 3072 and 4096 and the 4096-CU pass, each
    inside an entry's segment (entry 10's for 4096).  (Ten entries of which one does not descend stop at 4036 nodes, short of the pass size: hence eleven.)"""
    pkg = gpu
    qps, P, mid = (32, 37), 11, 5
    offs = [-132 if p == mid else 5 * (p % 2) for p in range(P)]
    org, pred = naturals(1)
    for off in sorted(set(offs)):
        for q in qps:
            split, margin = oracle_roots(pkg, 13, org, pred, 0, off + q)
            print(f"oracle, weight seed 13, picture seed 1, qp {off + q}: QT among the six 128 roots {split}, smallest margin {margin:.4f}")
            assert margin > CLEAR and sum(split) == (0 if off < 0 else 6), (off, q, split, margin)
    m = contexts(13)
    with Pair(m, org, pred) as (o, p):
        got = check(m, [(o, p, 0, off) for off in offs], qps, "boundaries", descend={64: 0b11, 32: 0b11})
        for e in range(P):
            assert got[e][0]["union_nodes"].tolist() == ([6, 0, 8, 26 + 32] if e == mid else [6, 24, 104, 442]), (e, got[e][0]["union_nodes"])
            for g in got[e]:
                assert len(g["nodes"]) == (6 + 8 + 58 if e == mid else 576)
        starts = np.cumsum([0] + [58 if e == mid else 442 for e in range(P)])
        assert starts[-1] == 4478 > CHUNK and all(int(b) not in starts.tolist() for b in (1024, 2048, 3072, 4096))


def test_degenerate_shapes(gpu, contexts, naturals):
    m = contexts(13)
    many = [-100, 0, 32, 0, -7, 22, 27, 37, 51, 400, -100, 5] + list(range(1, 21))
    assert len(many) == 32 and len(set(many)) < 32 and min(many) < 0
    with Pair(m, *naturals(3)) as (o, p), Pair(m, *naturals(2)) as (o2, p2):
        # P = 1, offset 0: mlt_predict_tree_sweep's bytes
        got = check(m, [(o, p, 1, 0)], (-100, 0, 32), "one entry")
        sweep = m.predict_tree_sweep(o, p, 1, (-100, 0, 32), want=TREE_ALL)
        for q in range(3):
            assert got[0][q]["first_node"] == sweep[q]["first_node"] and _same(got[0][q]["union_nodes"], sweep[q]["union_nodes"])
            for k in ("nodes",) + TREE_ALL:
                assert _same(got[0][q][k], sweep[q][k]), (q, k)
        # P = 1 with an offset: the offset is part of the points
        moved = check(m, [(o, p, 1, 32)], (-132, -32, 0), "one entry, offset 32", singles=False)
        for q in range(3):
            for k in ("nodes",) + TREE_ALL:
                assert _same(moved[0][q][k], sweep[q][k]), (q, k)
        # Q = 1: mlt_predict_trees (inside check); P = Q = 1: mlt_predict_tree
        check(m, [(o, p, 1, 0), (o2, p2, 2, 5), (o, p, 3, -20)], (27,), "one point")
        one = check(m, [(o2, p2, 2, 5)], (27,), "one entry, one point")
        single = m.predict_tree(o2, p2, 2, 32, want=TREE_ALL)
        assert one[0][0]["first_node"] == 0
        for k in ("nodes",) + TREE_ALL:
            assert _same(one[0][0][k], single[k]), k
        lean = check(m, [(o2, p2, 2, 5)], (27,), "one entry, one point, lean", want=("leaf_map",), singles=False)
        assert _same(lean[0][0]["nodes"], single["nodes"]) and _same(lean[0][0]["leaf_map"], single["leaf_map"])
        # Q = 32 (bit 31 of the masks), duplicates and negative values, two entries at different offsets
        got = check(m, [(o, p, 1, 0), (o2, p2, 0, -3)], many, "32 points", singles=False)
        assert _same(got[0][1]["nodes"], got[0][3]["nodes"]) and _same(got[1][0]["logits"], got[1][10]["logits"])   # the duplicates
        assert not _same(got[0][0]["logits"], got[0][31]["logits"])
        # fewer levels
        check(m, [(o, p, 1, 0), (o2, p2, 0, 7)], (0, 32), "top 32", top=32, min_size=16)
        flat = check(m, [(o, p, 1, 0), (o2, p2, 0, 7)], (0, 32), "top 16", top=16, min_size=16)
        assert all(len(g["nodes"]) == 26 * 17 and g["union_nodes"].tolist() == [442, 0, 0, 0] for row in flat for g in row)


def test_content_that_the_guards_take(gpu, contexts, naturals):
    """tests/test_tree_sweep_gpu.py's picture of a constant area, a +-1 LSB dither area and natural patches, twice at different offsets; then under a
    confidence gate at 64, then a (0.9, 1) policy with MLT_TREE_BY_CANDIDATES, then the policy alone with no records asked for."""
    rng = np.random.default_rng(77)
    org, pred = (a.copy() for a in naturals(1))
    org[:128, :256], pred[:128, :256] = 512, 508
    d = (600 + rng.integers(-1, 2, size=(152, 256))).astype(np.int16)
    org[128:, :256], pred[128:, :256] = d, (d + rng.integers(-1, 2, size=d.shape)).astype(np.int16)
    qps = (-100, 0, 400)
    m = contexts(13)
    thr = float(np.float32(0.9))
    with Pair(m, org, pred) as (o, p):
        entries = [(o, p, 0, 0), (o, p, 1, 16)]
        try:
            r0 = _reruns(m, SIZES)
            check(m, entries, qps, "guards")
            assert _reruns(m, SIZES) > r0, "the constant and the dither area must reach the guards"
            m.set_confidence_gate(64, thr)
            got = check(m, entries, qps, "gate at 64")
            for row in got:
                for g in row:   # a withheld split does not descend, per slice
                    n64 = g["nodes"][g["nodes"]["size"] == 64]
                    assert np.array_equal(n64["split_mode"] < 0, ~(n64["confidence"] >= np.float32(thr))) and (n64["first_child"][n64["split_mode"] < 0] == -1).all()
            m.set_confidence_gate(64, 0.0)
            for s in SIZES:
                m.set_candidate_policy(s, thr, 1)
            got = check(m, entries, qps, "by candidates", by_candidates=True)
            for row in got:
                for g in row:
                    nd = g["nodes"]
                    inner = nd["size"] > 16
                    assert np.array_equal(nd["first_child"][inner] >= 0, (nd["cand_mask"][inner] & 2) != 0)
                    assert np.array_equal(g["candidates"]["mask"], nd["cand_mask"])
            check(m, entries, qps, "policy, lean", want=("leaf_map",))
        finally:
            m.set_confidence_gate(64, 0.0)
            for s in SIZES:
                m.set_candidate_policy(s, 0.0, 0)


def test_one_trunk_pass(gpu, contexts, naturals):
    """Every class descends at every size, so every tree is the full tree and every union is one tree.  The call gathers a level once per 4096 of its nodes OVER
    ALL ENTRIES -- not per entry, not per point -- and launches the trunk kernels exactly as often as mlt_predict_trees over the P entries at ONE qp.  (A context
    without guards: an exact re-run would add trunk launches of its own on whichever nodes it flags.)"""
    pkg = gpu
    m = contexts(13, SIZES, pkg.capi.FLAG_NO_FLAT_GUARD | pkg.capi.FLAG_NO_DECISION_GUARD | pkg.capi.FLAG_NO_MAGNITUDE_GUARD)
    every = {128: 0b11, 64: 0b11, 32: 0b11}
    P, qps = 12, (22, 27, 32, 37)
    with Pair(m, *naturals(1)) as (o, p):
        try:
            m.profile_enable(True)
            got = m.predict_trees_sweep([(o, p)] * P, list(range(P)), [p % 3 for p in range(P)], qps, descend=every, want=TREE_ALL)
            call = {r["name"]: r for r in m.profile_read()}
            m.profile_enable(True)   # (clears the accumulated launches)
            m.predict_trees([(o, p)] * P, list(range(P)), 32, descend=every, want=TREE_ALL)
            trees = {r["name"]: r for r in m.profile_read()}
            m.profile_enable(False)
        finally:
            m.profile_enable(False)
    assert all(g["union_nodes"].tolist() == [6, 24, 104, 442] and len(g["nodes"]) == 576 for row in got for g in row)
    level = [P * n for n in (6, 24, 104, 442)]
    assert level[3] == 5304 > CHUNK
    outside = lambda k: "tree" in k or "gather" in k or "heads" in k
    print("the call:", {k: v["launches"] for k, v in call.items()}, "\nmlt_predict_trees, one qp:", {k: v["launches"] for k, v in trees.items()})
    assert call["picture_gather_multi"]["launches"] == sum(-(-n // CHUNK) for n in level) == 5 and "picture_gather" not in call
    assert call["heads_sweep"]["launches"] == 5 and "heads" not in call
    assert call["tree_expand_sweep"]["launches"] == 5 and call["tree_sweep_rank"]["launches"] == 1 and call["tree_sweep_pack"]["launches"] == 1
    assert "tree_expand" not in call and "tree_pack" not in call
    trunk_call, trunk_trees = ({k: v["launches"] for k, v in d.items() if not outside(k)} for d in (call, trees))
    assert trunk_call and trunk_call == trunk_trees, (trunk_call, trunk_trees)
    assert call["picture_gather_multi"]["bytes"] == pytest.approx(trees["picture_gather_multi"]["bytes"], rel=1e-6)


def test_bad_arguments_launch_nothing(gpu, contexts, naturals):
    pkg = gpu
    m = contexts(13)
    other = _open(pkg, 13, sizes=(64, 16))   # 32 is missing between 64 and 16, and 128 above
    org, pred = naturals(6)
    per = pkg.capi.tree_max_nodes(W, H)
    assert per == 576
    P, Q = 2, 3
    cap = P * Q * per
    good_qps = np.array([-100, 0, 32], np.int32)

    def call(ctx, pairs, n_pictures=P, qps=good_qps, n_qps=Q, offs=(0, 5), node_cap=cap, struct_size=None, top=128, mn=16, masks=(0, 0, 0, 0), flags=0, stride=15, null=()):
        cfg = pkg.capi.MltTreeConfig()
        cfg.struct_size = C.sizeof(pkg.capi.MltTreeConfig) if struct_size is None else struct_size
        cfg.top_size, cfg.min_size, cfg.flags, cfg.poc, cfg.qp = top, mn, flags, 2, 99
        for i, v in enumerate(masks):
            cfg.descend_mask[i] = v
        entries = (pkg.capi.MltTreePicture * 260)()
        for i in range(260):
            o, q = pairs[i % len(pairs)]
            entries[i].org, entries[i].pred, entries[i].poc, entries[i].qp = (o._h if o else None), (q._h if q else None), 2 + i, offs[i % len(offs)]
        qps = np.resize(np.asarray(qps, np.int32), 40)
        nodes = np.zeros(cap, pkg.capi.TREE_NODE_DTYPE)
        nodes["size"] = -7
        first = np.full(40, -7, np.int32)
        union = np.full((P, 4), -7, np.int32)
        lm = np.full((P * Q, H // 16, W // 16), 0x5A, np.uint8)
        lg = np.full((cap, 15), -7.0, np.float32)
        dec = np.zeros(cap, pkg.capi.DECISION_DTYPE)
        cand = np.zeros(cap, pkg.capi.CANDIDATES_DTYPE)
        dec["raw_mode"] = -7
        cand["count"] = -7
        rc = ctx._lib.mlt_predict_trees_sweep(ctx._h, n_pictures, None if "pics" in null else entries, None if "cfg" in null else C.byref(cfg),
                                              None if "qps" in null else qps.ctypes.data, n_qps, None if "nodes" in null else nodes.ctypes.data, node_cap,
                                              None if "first" in null else first.ctypes.data, union.ctypes.data, lm.ctypes.data, lg.ctypes.data, stride, dec.ctypes.data,
                                              cand.ctypes.data)
        untouched = ((first == -7).all() and (union == -7).all() and (nodes["size"] == -7).all() and (lm == 0x5A).all() and (lg == -7.0).all()
                     and (dec["raw_mode"] == -7).all() and (cand["count"] == -7).all())
        return rc, bool(untouched), nodes, first, lm, union

    smaller = m.picture(W, H - 16).upload(pred[:H - 16])
    huge = (m.picture(8208, 8208), m.picture(8208, 8208))   # 513 x 513 nodes at 16: x 256 entries x 32 points leaves int32 (never read: the call is refused)
    fo, fp = other.picture(W, H).upload(org), other.picture(W, H).upload(pred)
    with Pair(m, org, pred) as (o, p):
        good = [(o, p)]
        try:
            r0 = _reruns(m, SIZES)
            m.profile_enable(True)
            for n in (0, -1, 33):
                assert call(m, good, n_qps=n)[:2] == (MLT_ERR_ARG, True), n
            for n in (0, -1, 257):
                assert call(m, good, n_pictures=n)[:2] == (MLT_ERR_ARG, True), n
            for name in ("pics", "cfg", "qps", "nodes", "first"):
                assert call(m, good, null=(name,))[:2] == (MLT_ERR_ARG, True), name
            assert call(m, good, struct_size=C.sizeof(pkg.capi.MltTreeConfig) - 4)[:2] == (MLT_ERR_ARG, True)
            assert call(m, [(o, p), (None, p)])[:2] == (MLT_ERR_ARG, True) and call(m, [(o, p), (o, None)])[:2] == (MLT_ERR_ARG, True)   # a NULL picture in entry 1
            assert call(m, [(o, p), (o, fp)])[:2] == (MLT_ERR_ARG, True) and call(m, [(o, p), (fo, p)])[:2] == (MLT_ERR_ARG, True)       # a picture of another context
            assert call(m, [(o, p), (o, smaller)])[:2] == (MLT_ERR_ARG, True)                                                            # unequal geometry inside an entry
            assert call(m, [(o, p), (smaller, smaller)])[:2] == (MLT_ERR_ARG, True)                                                      # ... and between entries
            assert call(m, good, node_cap=cap - 1)[:2] == (MLT_ERR_ARG, True)                                # one node short of n_pictures * n_qps * max_nodes
            assert call(m, [huge], n_pictures=256, n_qps=32, node_cap=INT32_MAX, top=16)[:2] == (MLT_ERR_ARG, True)   # 256 x 32 x 263169 nodes: beyond int32
            assert call(m, good, qps=(0, INT32_MAX, 5), offs=(0, 1))[:2] == (MLT_ERR_ARG, True)             # entry 1: 1 + INT32_MAX
            assert call(m, good, qps=(0, INT32_MIN, 5), offs=(-1, 0))[:2] == (MLT_ERR_ARG, True)            # entry 0: -1 + INT32_MIN
            assert call(m, good, stride=14)[:2] == (MLT_ERR_ARG, True)
            assert call(m, good, top=48)[:2] == (MLT_ERR_ARG, True)
            assert call(m, good, top=32, mn=64)[:2] == (MLT_ERR_ARG, True)
            assert call(m, good, masks=(0, 0b100, 0, 0))[:2] == (MLT_ERR_ARG, True)                          # head 0 of the 64 model has two classes
            assert call(m, good, flags=2)[:2] == (MLT_ERR_ARG, True)
            assert call(other, [(fo, fp)], top=64)[:2] == (MLT_ERR_SIZE_DISABLED, True)                      # 32 not loaded between 64 and 16
            assert call(other, [(fo, fp)])[:2] == (MLT_ERR_SIZE_DISABLED, True)                              # 128 not loaded
            assert m.profile_read() == [] and other.profile_read() == [], "a refused call launched something"
            assert _reruns(m, SIZES) == r0
            m.profile_enable(False)
            # a following valid call is still right (cfg.poc = 2 and cfg.qp = 99 are not read: entry i takes poc 2 + i); INT32_MAX as a sum is allowed
            rc, untouched, nodes, first, lm, union = call(m, good, qps=(-100, INT32_MAX - 5, 32), offs=(0, 5))
            assert rc == 0 and not untouched and first[0] == 0 and (first[P * Q + 1:] == -7).all() and (union[:, 0] == 6).all()
            for e, off in enumerate((0, 5)):
                for q, qp in enumerate((-100, INT32_MAX - 5, 32)):
                    s = m.predict_tree(o, p, 2 + e, off + qp, want=("leaf_map",))
                    k = e * Q + q
                    assert _same(nodes[first[k]:first[k + 1]], s["nodes"]) and _same(lm[k], s["leaf_map"]), (e, q)
            assert (nodes["size"][first[P * Q]:] == -7).all()
        finally:
            m.profile_enable(False)
            smaller.close()
            for h in huge:
                h.close()
            fo.close()
            fp.close()
            other.close()
