"""GPU (MI355X): partition trees of one picture pair under several QPs from ONE union descent -- mlt_predict_tree_sweep against its twin, mlt_predict_trees over
n_qps entries {org, pred, poc, qps[q]} of the same uploaded pair, on the same context.

Every assertion between the two is BYTE equality, all result buffers zero-filled first: every slice's nodes, first_node, the leaf maps, the logits (whole rows),
the decision and the candidate records.  union_nodes[l] must be the number of distinct positions of that size over the slices.  With a[q] the growth of
guard_reruns under the n_qps single mlt_predict_tree calls: max(a) <= growth under the sweep call <= sum(a).
Preconditions on the content (which nodes say QT under which point) come from the CPU oracle alone, never from what the device returns."""
import ctypes as C

import numpy as np
import pytest

from tree_gpu_common import (CHUNK, LOGIT_TOL, MLT_ERR_ARG, MLT_ERR_SIZE_DISABLED, SIZES, TREE_ALL, UNDECIDABLE, H, W, Pair, contexts, gpu, naturals,   # noqa: F401  (fixtures)
                             oracle_level, open_context as _open, reruns as _reruns, same as _same)

pytestmark = pytest.mark.gpu


def check_sweep(m, o, p, poc, qps, what, want=TREE_ALL, **kw):
    """mlt_predict_tree_sweep == mlt_predict_trees over the n_qps entries of the pair, byte for byte; union_nodes; guard re-runs between the maximum and the sum
    of the single calls' -> the sweep call's result."""
    qps = [int(q) for q in qps]
    Q = len(qps)
    top, mn = kw.get("top", 128), kw.get("min_size", 16)
    sizes = [s for s in SIZES if mn <= s <= top]
    r0 = _reruns(m, sizes)
    got = m.predict_tree_sweep(o, p, poc, qps, want=want, **kw)
    grown = _reruns(m, sizes) - r0
    twin = m.predict_trees([(o, p)] * Q, poc, np.array(qps, np.int32), want=want, **kw)
    a = []
    for q in qps:
        r1 = _reruns(m, sizes)
        m.predict_tree(o, p, poc, q, want=("leaf_map",), **kw)
        a.append(_reruns(m, sizes) - r1)
    assert len(got) == Q == len(twin)
    for q, (g, t) in enumerate(zip(got, twin)):
        assert g["first_node"] == t["first_node"], (what, q, g["first_node"], t["first_node"])
        assert len(g["nodes"]) == len(t["nodes"]), (what, q, len(g["nodes"]), len(t["nodes"]))
        for f in t["nodes"].dtype.names:
            assert np.array_equal(g["nodes"][f], t["nodes"][f], equal_nan=f == "confidence"), (what, q, f, np.flatnonzero(g["nodes"][f] != t["nodes"][f])[:8])
        assert _same(g["nodes"], t["nodes"]), (what, q)
        for k in want:
            assert _same(g[k], t[k]), (what, q, k)
        assert sorted(g) == sorted(["nodes", "first_node", "union_nodes"] + list(want)), sorted(g)
    union = got[0]["union_nodes"]
    assert union.shape == (4,) and union.dtype == np.int32 and all(np.array_equal(g["union_nodes"], union) for g in got)
    for l, s in enumerate(SIZES[SIZES.index(top):]):
        distinct = {(int(x), int(y)) for g in got for x, y in zip(g["nodes"]["x"][g["nodes"]["size"] == s], g["nodes"]["y"][g["nodes"]["size"] == s])}
        assert union[l] == len(distinct), (what, s, int(union[l]), len(distinct))
    print(f"{what}: union {union.tolist()}, slices {[len(g['nodes']) for g in got]}, guard re-runs: sweep {grown}, singles {a}")
    assert max(a) <= grown <= sum(a), (what, "guard re-runs", grown, a)
    return got


def test_diverging_descents_all_four_sizes(gpu, contexts, naturals):
    pkg = gpu
    roots = pkg.capi.tree_roots(W, H, 128, 128)
    assert len(roots) == 6 and len(pkg.capi.tree_roots(W, H, 128, 64)) == 0
    qps = (-100, 0, 32)
    # the precondition, from the oracle alone, on picture seed 1: no QT among the six 128 roots under -100, all six under 32, a decided part of them under 0
    org, pred = naturals(1)
    qt, clear = [], []
    for qp in qps:
        split, margin = oracle_level(pkg, 13, 128, org, pred, roots, 0, qp)
        assert float(margin.min()) > UNDECIDABLE, (qp, float(margin.min()))
        qt.append(int((split == 1).sum()))
        clear.append(float(margin.min()) > 4 * LOGIT_TOL)   # two logits within LOGIT_TOL of the reference cannot swap over such a margin
    print("oracle, weight seed 13, picture seed 1: QT among the six 128 roots under", qps, "->", qt, "clear of the logit contract:", clear)
    assert qt[0] == 0 and qt[2] == 6 and 0 < qt[1] < 6, qt
    m = contexts(13)
    for seed in (1, 34791):
        with Pair(m, *naturals(seed)) as (o, p):
            got = check_sweep(m, o, p, 0, qps, f"diverging, picture seed {seed}")
            if seed == 1:
                for q in range(3):
                    if clear[q]:
                        n128 = got[q]["nodes"][got[q]["nodes"]["size"] == 128]
                        assert int((n128["first_child"] >= 0).sum()) == qt[q], (q, qt[q])
                if clear[0]:   # slice 0 is the roots alone while the union descends
                    assert len(got[0]["nodes"]) == 6 + 0 + 8 + 26
                if clear[2]:
                    assert got[0]["union_nodes"][1] == 24
    # weight seed 12, picture seed 2: the number of 64 nodes that say QT differs between the points
    org, pred = naturals(2)
    qps = (0, 37, 100, 400)
    grid64 = pkg.capi.grid_positions(W, H, 64)
    assert len(grid64) == 24
    counts = [int((oracle_level(pkg, 12, 64, org, pred, grid64, 0, qp)[0] == 1).sum()) for qp in qps]
    print("oracle, weight seed 12, picture seed 2: QT among the 24 nodes of the 64 grid under", qps, "->", counts)
    assert len(set(counts)) > 1, counts
    m = contexts(12)
    with Pair(m, org, pred) as (o, p):
        check_sweep(m, o, p, 0, qps, "diverging at 64")


def test_tile_and_chunk_boundaries_in_one_picture(gpu, contexts):
    """1072 x 1024, top 32 / min 16: the 32 level is 33 x 32 = 1056 nodes (past the scan's 1024-node tile); with descend_mask[32] = 0b11 the 16 level is 64 border
    roots + 4224 children = 4288 nodes (past the 4096-CU pass)."""
    pkg = gpu
    w, h = 1072, 1024
    assert len(pkg.capi.tree_roots(w, h, 32, 32)) == 1056 and len(pkg.capi.tree_roots(w, h, 32, 16)) == 64
    rng = np.random.default_rng(3516)
    org = rng.integers(0, 1024, size=(h, w)).astype(np.int16)
    pred = np.clip(org.astype(np.int32) + rng.integers(-24, 25, size=(h, w)), 0, 1023).astype(np.int16)
    qps = (-100, 0, 51, 400)
    # the default-mask run's precondition, from the oracle on the first 128 roots alone: decided QT and decided non-QT nodes under one point, another count
    # under another point
    roots = pkg.capi.tree_roots(w, h, 32, 32)[:128]
    per_point, mixed = [], False
    for qp in qps:
        split, margin = oracle_level(pkg, 12, 32, org, pred, roots, 0, qp)
        per_point.append(int((split == 1).sum()))
        mixed = mixed or (int(((split == 1) & (margin > UNDECIDABLE)).sum()) > 0 and int(((split != 1) & (margin > UNDECIDABLE)).sum()) > 0)
    print("oracle, weight seed 12: QT among the first 128 roots at 32 under", qps, "->", per_point)
    assert mixed and len(set(per_point)) > 1, per_point
    m = contexts(12, (32, 16))
    with Pair(m, org, pred) as (o, p):
        got = check_sweep(m, o, p, 0, (3, 9), "all descend", top=32, min_size=16, descend={32: 0b11})
        assert got[0]["union_nodes"].tolist() == [1056, 4288, 0, 0]
        for q, g in enumerate(got):
            nd = g["nodes"]
            assert g["first_node"] == q * 5344 and len(nd) == 1056 + 64 + 4224
            assert np.array_equal(nd["first_child"][:1056], 1056 + 64 + 4 * np.arange(1056)) and (nd["first_child"][1056:] == -1).all()
            assert (nd["parent"][:1120] == -1).all() and np.array_equal(nd["parent"][1120:], np.repeat(np.arange(1056), 4))
            assert (nd["flags"][:1056] == 0).all() and (nd["flags"][1056:1120] == 1).all() and (nd["flags"][1120:] == 0).all()
        got = check_sweep(m, o, p, 0, qps, "content-dependent", top=32, min_size=16)
        print("device: descending 32 nodes per point", [int((g["nodes"]["first_child"] >= 0).sum()) for g in got])


def test_thirty_two_points_and_one_point(gpu, contexts, naturals):
    """n_qps = 32 with duplicates and negative values (bit 31 of the masks); n_qps = 1 is mlt_predict_tree with that qp."""
    m = contexts(13)
    qps = [-100, 0, 32, 0, -7, 22, 27, 37, 51, 400, -100, 5] + list(range(1, 21))
    assert len(qps) == 32 and len(set(qps)) < 32 and min(qps) < 0
    with Pair(m, *naturals(3)) as (o, p):
        got = check_sweep(m, o, p, 1, qps, "32 points")
        assert _same(got[1]["nodes"], got[3]["nodes"]) and _same(got[0]["logits"], got[10]["logits"])   # the duplicates
        assert not _same(got[0]["logits"], got[31]["logits"])
        one = check_sweep(m, o, p, 1, [0], "one point")
        single = m.predict_tree(o, p, 1, 0, want=TREE_ALL)
        assert one[0]["first_node"] == 0 and _same(one[0]["nodes"], single["nodes"])
        for k in TREE_ALL:
            assert _same(one[0][k], single[k]), k
        lean = check_sweep(m, o, p, 1, [0], "one point, lean", want=("leaf_map",))
        assert _same(lean[0]["nodes"], single["nodes"]) and _same(lean[0]["leaf_map"], single["leaf_map"])


def test_content_that_the_guards_take(gpu, contexts, naturals):
    """One picture of a constant area, a +-1 LSB dither area and natural patches; then under a confidence gate at 64, then a (0.9, 1) policy with
    MLT_TREE_BY_CANDIDATES, then the policy alone with no records asked for."""
    rng = np.random.default_rng(77)
    org, pred = (a.copy() for a in naturals(1))
    org[:128, :256], pred[:128, :256] = 512, 508
    d = (600 + rng.integers(-1, 2, size=(152, 256))).astype(np.int16)
    org[128:, :256], pred[128:, :256] = d, (d + rng.integers(-1, 2, size=d.shape)).astype(np.int16)
    qps = (-100, 0, 400)
    m = contexts(13)
    thr = float(np.float32(0.9))
    with Pair(m, org, pred) as (o, p):
        try:
            r0 = _reruns(m, SIZES)
            check_sweep(m, o, p, 0, qps, "guards")
            assert _reruns(m, SIZES) > r0, "the constant and the dither area must reach the guards"
            m.set_confidence_gate(64, thr)
            got = check_sweep(m, o, p, 0, qps, "gate at 64")
            for g in got:   # a withheld split does not descend, per slice
                n64 = g["nodes"][g["nodes"]["size"] == 64]
                assert np.array_equal(n64["split_mode"] < 0, ~(n64["confidence"] >= np.float32(thr))) and (n64["first_child"][n64["split_mode"] < 0] == -1).all()
            m.set_confidence_gate(64, 0.0)
            for s in SIZES:
                m.set_candidate_policy(s, thr, 1)
            got = check_sweep(m, o, p, 0, qps, "by candidates", by_candidates=True)
            for g in got:
                nd = g["nodes"]
                inner = nd["size"] > 16
                assert np.array_equal(nd["first_child"][inner] >= 0, (nd["cand_mask"][inner] & 2) != 0)
                assert np.array_equal(g["candidates"]["mask"], nd["cand_mask"])
            check_sweep(m, o, p, 0, qps, "policy, lean", want=("leaf_map",))
        finally:
            m.set_confidence_gate(64, 0.0)
            for s in SIZES:
                m.set_candidate_policy(s, 0.0, 0)


def test_one_trunk_pass(gpu, contexts, naturals):
    """The sweep call gathers every union node once (picture_gather, once per level and chunk) and runs the sweep heads; mlt_predict_trees with the same entries
    gathers every node of every slice."""
    m = contexts(13)
    with Pair(m, *naturals(1)) as (o, p):
        try:
            for qps in ((-100, 0, 32), (7, 7, 7, 7)):
                Q = len(qps)
                m.profile_enable(True)
                got = m.predict_tree_sweep(o, p, 0, qps, want=TREE_ALL)
                sweep = {r["name"]: r for r in m.profile_read()}
                m.profile_enable(True)   # (clears the accumulated launches)
                twin = m.predict_trees([(o, p)] * Q, 0, np.array(qps, np.int32), want=TREE_ALL)
                trees = {r["name"]: r for r in m.profile_read()}
                m.profile_enable(False)
                union = got[0]["union_nodes"]
                print(qps, "sweep:", {k: v["launches"] for k, v in sweep.items() if "tree" in k or "gather" in k or "heads" in k},
                      "trees:", {k: v["launches"] for k, v in trees.items() if "tree" in k or "gather" in k or "heads" in k})
                assert sweep["picture_gather"]["launches"] == sum(-(-int(n) // CHUNK) for n in union), (sweep["picture_gather"], union)
                assert "picture_gather_multi" not in sweep and "heads" not in sweep and sweep["heads_sweep"]["launches"] >= int((union > 0).sum())
                assert sweep["tree_expand_sweep"]["launches"] == 5 and sweep["tree_sweep_pack"]["launches"] == 1 and "tree_expand" not in sweep and "tree_pack" not in sweep
                assert "picture_gather" not in trees and "heads_sweep" not in trees
                # the gather's algorithmic bytes: both planes of a CU read and written (+ the entry's poc / qp written by the multi-entry gather)
                cus = sum(len(t["nodes"]) for t in twin)
                assert sweep["picture_gather"]["bytes"] == pytest.approx(sum(int(n) * s * s * 8 for n, s in zip(union, SIZES)), rel=1e-6)
                assert trees["picture_gather_multi"]["bytes"] == pytest.approx(sum(int(s) ** 2 * 8 + 12 for t in twin for s in t["nodes"]["size"]), rel=1e-6)
                assert cus > int(union.sum())
                if len(set(qps)) == 1:   # the same tree n_qps times: exactly n_qps times as many CUs gathered
                    assert cus == Q * int(union.sum())
                    assert trees["picture_gather_multi"]["bytes"] == pytest.approx(Q * (sweep["picture_gather"]["bytes"] + 12 * int(union.sum())), rel=1e-6)
        finally:
            m.profile_enable(False)


def test_bad_arguments_launch_nothing(gpu, contexts, naturals):
    pkg = gpu
    m = contexts(13)
    other = _open(pkg, 13, sizes=(64, 16))   # 32 is missing between 64 and 16, and 128 above
    org, pred = naturals(6)
    per = pkg.capi.tree_max_nodes(W, H)
    assert per == 576
    Q = 3
    cap = Q * per
    good_qps = np.array([-100, 0, 32], np.int32)

    def call(ctx, o, q, n_qps=Q, node_cap=cap, struct_size=None, top=128, mn=16, masks=(0, 0, 0, 0), flags=0, stride=15, null=()):
        cfg = pkg.capi.MltTreeConfig()
        cfg.struct_size = C.sizeof(pkg.capi.MltTreeConfig) if struct_size is None else struct_size
        cfg.top_size, cfg.min_size, cfg.flags, cfg.poc, cfg.qp = top, mn, flags, 2, 99
        for i, v in enumerate(masks):
            cfg.descend_mask[i] = v
        qps = np.resize(good_qps, 40)
        nodes = np.zeros(cap, pkg.capi.TREE_NODE_DTYPE)
        nodes["size"] = -7
        first = np.full(40, -7, np.int32)
        union = np.full(4, -7, np.int32)
        lm = np.full((Q, H // 16, W // 16), 0x5A, np.uint8)
        lg = np.full((cap, 15), -7.0, np.float32)
        dec = np.zeros(cap, pkg.capi.DECISION_DTYPE)
        cand = np.zeros(cap, pkg.capi.CANDIDATES_DTYPE)
        dec["raw_mode"] = -7
        cand["count"] = -7
        rc = ctx._lib.mlt_predict_tree_sweep(ctx._h, o._h if o else None, q._h if q else None, None if "cfg" in null else C.byref(cfg),
                                             None if "qps" in null else qps.ctypes.data, n_qps, None if "nodes" in null else nodes.ctypes.data, node_cap,
                                             None if "first" in null else first.ctypes.data, union.ctypes.data, lm.ctypes.data, lg.ctypes.data, stride, dec.ctypes.data,
                                             cand.ctypes.data)
        untouched = ((first == -7).all() and (union == -7).all() and (nodes["size"] == -7).all() and (lm == 0x5A).all() and (lg == -7.0).all()
                     and (dec["raw_mode"] == -7).all() and (cand["count"] == -7).all())
        return rc, bool(untouched), nodes, first, lm

    smaller = m.picture(W, H - 16).upload(pred[:H - 16])
    fo, fp = other.picture(W, H).upload(org), other.picture(W, H).upload(pred)
    with Pair(m, org, pred) as (o, p):
        try:
            m.profile_enable(True)
            for n in (0, -1, 33):
                assert call(m, o, p, n_qps=n)[:2] == (MLT_ERR_ARG, True), n
            for name in ("cfg", "qps", "nodes", "first"):
                assert call(m, o, p, null=(name,))[:2] == (MLT_ERR_ARG, True), name
            assert call(m, o, p, struct_size=C.sizeof(pkg.capi.MltTreeConfig) - 4)[:2] == (MLT_ERR_ARG, True)
            assert call(m, None, p)[:2] == (MLT_ERR_ARG, True) and call(m, o, None)[:2] == (MLT_ERR_ARG, True)   # a NULL picture
            assert call(m, o, fp)[:2] == (MLT_ERR_ARG, True) and call(m, fo, p)[:2] == (MLT_ERR_ARG, True)       # a picture of another context
            assert call(m, o, smaller)[:2] == (MLT_ERR_ARG, True)                                                # unequal geometry
            assert call(m, o, p, node_cap=cap - 1)[:2] == (MLT_ERR_ARG, True)                                    # one node short of n_qps * max_nodes
            assert call(m, o, p, stride=14)[:2] == (MLT_ERR_ARG, True)
            assert call(m, o, p, top=48)[:2] == (MLT_ERR_ARG, True)
            assert call(m, o, p, top=32, mn=64)[:2] == (MLT_ERR_ARG, True)
            assert call(m, o, p, masks=(0, 0b100, 0, 0))[:2] == (MLT_ERR_ARG, True)                              # head 0 of the 64 model has two classes
            assert call(m, o, p, flags=2)[:2] == (MLT_ERR_ARG, True)
            assert call(other, fo, fp, top=64)[:2] == (MLT_ERR_SIZE_DISABLED, True)                              # 32 not loaded between 64 and 16
            assert call(other, fo, fp)[:2] == (MLT_ERR_SIZE_DISABLED, True)                                      # 128 not loaded
            assert m.profile_read() == [], "a refused call launched something"
            m.profile_enable(False)
            # a following valid call is still right (cfg.qp = 99 is not read)
            rc, untouched, nodes, first, lm = call(m, o, p)
            assert rc == 0 and not untouched and first[0] == 0 and (first[Q + 1:] == -7).all()
            for q, qp in enumerate(good_qps):
                s = m.predict_tree(o, p, 2, int(qp), want=("leaf_map",))
                assert _same(nodes[first[q]:first[q + 1]], s["nodes"]) and _same(lm[q], s["leaf_map"]), q
            assert (nodes["size"][first[Q]:] == -7).all()
        finally:
            m.profile_enable(False)
            smaller.close()
            fo.close()
            fp.close()
            other.close()
