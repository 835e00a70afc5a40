"""GPU (MI355X): partition trees of several pictures in one call -- mlt_predict_trees against P single mlt_predict_tree calls on the same context.

Every assertion between the two is BYTE equality, both result buffers zero-filled first: picture p's node slice, leaf map, decision and candidate records are the
single call's for (pics[p].org, pics[p].pred, pics[p].poc, pics[p].qp); the logits are the single call's as capi returns them ([n, 15], zeros behind the size's
logit count -- the batched call writes those zeros itself, the single call leaves them to the zero-filled buffer).  guard_reruns must grow by the same amount.
Preconditions on the content (which pictures descend at which level) come from the CPU oracle alone, never from what the device returns."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tree_host import host_tree   # the descent driven from the host (build_tree over predict_at)
from tree_gpu_common import (LOGIT_TOL, MLT_ERR_ARG, MLT_ERR_SIZE_DISABLED, SIZES, TREE_ALL, UNDECIDABLE, H, W, contexts, gpu, naturals, oracle_level,   # noqa: F401  (fixtures)
                             open_context as _open, reruns as _reruns, same as _same)

pytestmark = pytest.mark.gpu
POC_QP = list(itertools.product((0, 1, 2), (0, 1)))
# 24 distinct picture seeds for the 424 x 280 cases; picture i carries POC_QP[i % 6].  The seeded 128 model's head 0 says QT for a natural patch unless the patch is
# dark (mean below ~285 ten-bit steps): seeds 34791 and 41262 are the first two whose six whole 128 patches are all dark -- no QT among their 128 nodes, so their
# 64 segment is EMPTY (424 x 280 has no 64 roots); every other seed has 2 .. 6 QT nodes.  Found by the CPU oracle; the test asserts it from the oracle again.
PIC_SEEDS = [34791, 41262] + list(range(1, 23))


def check_batched_is_singles(m, pairs, poc, qp, what, want=TREE_ALL, **kw):
    """mlt_predict_trees == the P mlt_predict_tree calls, byte for byte, guard re-runs included -> the batched result."""
    top, mn = kw.get("top", 128), kw.get("min_size", 16)
    sizes = [s for s in SIZES if mn <= s <= top]
    r0 = _reruns(m, sizes)
    got = m.predict_trees(pairs, poc, qp, want=want, **kw)
    r1 = _reruns(m, sizes)
    singles = [m.predict_tree(o, p, int(poc[i]), int(qp[i]), want=want, **kw) for i, (o, p) in enumerate(pairs)]
    r2 = _reruns(m, sizes)
    assert len(got) == len(pairs)
    first = 0
    for i, (g, s) in enumerate(zip(got, singles)):
        assert g["first_node"] == first, (what, i, g["first_node"], first)
        first += len(s["nodes"])
        assert len(g["nodes"]) == len(s["nodes"]), (what, i, len(g["nodes"]), len(s["nodes"]))
        for f in s["nodes"].dtype.names:
            assert np.array_equal(g["nodes"][f], s["nodes"][f], equal_nan=f == "confidence"), (what, i, f, np.flatnonzero(g["nodes"][f] != s["nodes"][f])[:8])
        assert _same(g["nodes"], s["nodes"]), (what, i)
        for k in want:
            assert _same(g[k], s[k]), (what, i, k)
    assert r1 - r0 == r2 - r1, (what, "guard re-runs", r1 - r0, r2 - r1)
    return got


def upload_all(m, pictures, w=W, h=H):
    return [(m.picture(w, h).upload(o), m.picture(w, h).upload(p)) for o, p in pictures]


def close_all(pairs):
    for o, p in pairs:
        o.close()
        p.close()


def test_mixed_decisions_with_the_streaming_threshold_crossed_at_128(gpu, contexts, naturals):
    """24 pictures, all four sizes, weight seed 13: the 128 level is 144 CUs in one pass (6 per single call); two pictures have an empty 64 segment."""
    pkg = gpu
    poc = np.array([POC_QP[i % 6][0] for i in range(24)], np.int32)
    qp = np.array([POC_QP[i % 6][1] for i in range(24)], np.int32)
    assert len(set(PIC_SEEDS)) == 24 and set(zip(poc.tolist(), qp.tolist())) == set(POC_QP)
    # the precondition, from the oracle alone: QT (class 1) among the six 128 roots of every picture under the (poc, qp) it carries
    roots = pkg.capi.tree_roots(W, H, 128, 128)
    assert len(roots) == 6 and len(pkg.capi.tree_roots(W, H, 128, 64)) == 0
    qt, clear = [], []
    for i, (org, pred) in enumerate(naturals(s) for s in PIC_SEEDS):
        split, margin = oracle_level(pkg, 13, 128, org, pred, roots, int(poc[i]), int(qp[i]))
        assert float(margin.min()) > UNDECIDABLE, (i, PIC_SEEDS[i], float(margin.min()))
        qt.append(int((split == 1).sum()))
        clear.append(float(margin.min()) > 4 * LOGIT_TOL)   # two logits within LOGIT_TOL of the reference cannot swap over such a margin
    print("oracle: QT nodes among the six 128 roots, per picture:", qt)
    zero = [i for i in range(24) if poc[i] == 0 and qp[i] == 0]
    assert any(q == 0 for q in qt) and any(q > 0 for q in qt)
    assert any(qt[i] == 0 for i in zero) and any(qt[i] > 0 for i in zero), [qt[i] for i in zero]
    assert any(q == 0 and c for q, c in zip(qt, clear)), "no picture without QT at 128 whose margins clear the logit contract"
    m = contexts(13)
    pairs = upload_all(m, [naturals(s) for s in PIC_SEEDS])
    try:
        got = check_batched_is_singles(m, pairs, poc, qp, "mixed")
        # the device agrees with the oracle about which pictures descend at 128 wherever the margins clear the logit contract, so the empty 64 segments were
        # really there
        for i, g in enumerate(got):
            if not clear[i]:
                continue
            n128 = g["nodes"][g["nodes"]["size"] == 128]
            assert int((n128["first_child"] >= 0).sum()) == qt[i], (i, qt[i])
            assert int((g["nodes"]["size"] == 64).sum()) == 4 * qt[i]
    finally:
        close_all(pairs)


def test_the_streaming_threshold_on_the_single_pass_tier(gpu, contexts, naturals):
    """Weight seed 10, 128 only, top = min = 128: the batched call's one pass of 144 CUs runs layer0_stream_kernel, a single call's 6 CUs do not; same bytes."""
    m = contexts(10, (128,))
    a = m.arithmetic(128)
    assert a["exact"] == 0 and a["w2_units"] == 0 and a["x_units"] == 0 and a["w2_stages"] == 0 and a["x_stages"] == 0, a   # the single pass
    poc = np.array([POC_QP[i % 6][0] for i in range(24)], np.int32)
    qp = np.array([POC_QP[i % 6][1] for i in range(24)], np.int32)
    pairs = upload_all(m, [naturals(s) for s in PIC_SEEDS])
    try:
        check_batched_is_singles(m, pairs, poc, qp, "single pass", top=128, min_size=128)
        m.profile_enable(True)
        m.predict_trees(pairs, poc, qp, top=128, min_size=128, want=TREE_ALL)
        batched = {p["name"]: p["launches"] for p in m.profile_read()}
        m.profile_enable(True)   # (clears the accumulated launches)
        for i, (o, p) in enumerate(pairs[:3]):
            m.predict_tree(o, p, int(poc[i]), int(qp[i]), top=128, min_size=128, want=TREE_ALL)
        single = {p["name"]: p["launches"] for p in m.profile_read()}
        m.profile_enable(False)
        print("batched:", batched, "\nsingle:", single)
        assert any(k.startswith("layer0_stream") for k in batched), batched
        assert not any(k.startswith("layer0_stream") for k in single), single
        assert batched.get("picture_gather_multi") == 1 and batched.get("tree_expand") == 2 and batched.get("tree_pack") == 1 and batched.get("tree_raster") == 1, batched
        assert "picture_gather_multi" not in single and "tree_pack" not in single and single.get("tree_expand") == 6 and single.get("picture_gather") == 3, single
    finally:
        m.profile_enable(False)
        close_all(pairs)


def test_tile_and_chunk_boundaries_inside_segments(gpu, contexts):
    """35 pictures of 208 x 176, top 32 / min 16: 30 roots at 32 and 23 border roots at 16 per picture; the 32 level is 1050 nodes (the scan's 1024-node tile ends
    inside picture 34's segment); with descend_mask[32] = 0b11 the 16 level is 35 x 143 = 5005 nodes (the 4096-CU pass ends inside picture 28's segment)."""
    pkg = gpu
    w, h, P = 208, 176, 35
    assert len(pkg.capi.tree_roots(w, h, 32, 32)) == 30 and len(pkg.capi.tree_roots(w, h, 32, 16)) == 23
    rng = np.random.default_rng(3516)
    org = rng.integers(0, 1024, size=(P, h, w)).astype(np.int16)
    pred = np.clip(org.astype(np.int32) + rng.integers(-24, 25, size=(P, h, w)), 0, 1023).astype(np.int16)
    poc, qp = np.arange(P, dtype=np.int32) % 3, np.arange(P, dtype=np.int32) % 2
    # run (b)'s precondition, from the oracle alone: weight seed 13 descends everywhere on this content, seed 12 mixes -- some decided QT and some decided non-QT
    # nodes at 32 over the call, and pictures whose 32 nodes descend nowhere beside pictures where some do
    roots = pkg.capi.tree_roots(w, h, 32, 32)
    sure_qt = sure_no = 0
    per_picture = []
    for p in range(P):
        split, margin = oracle_level(pkg, 12, 32, org[p], pred[p], roots, int(poc[p]), int(qp[p]))
        sure_qt += int(((split == 1) & (margin > UNDECIDABLE)).sum())
        sure_no += int(((split != 1) & (margin > UNDECIDABLE)).sum())
        per_picture.append(int((split == 1).sum()))
    print("oracle, seed 12: QT nodes of 30 per picture", per_picture)
    assert sure_qt > 0 and sure_no > 0 and 0 in per_picture and max(per_picture) >= 2
    m = contexts(12, (32, 16))
    pairs = upload_all(m, list(zip(org, pred)), w, h)
    try:
        # (a) every 32 node descends: everything in closed form
        got = check_batched_is_singles(m, pairs, poc, qp, "all descend", top=32, min_size=16, descend={32: 0b11})
        for p, g in enumerate(got):
            nd = g["nodes"]
            assert g["first_node"] == p * 173 and len(nd) == 30 + 23 + 120
            assert np.array_equal(nd["first_child"][:30], 30 + 23 + 4 * np.arange(30)) and (nd["first_child"][30:] == -1).all()
            assert (nd["parent"][:53] == -1).all() and np.array_equal(nd["parent"][53:], np.repeat(np.arange(30), 4))
            assert (nd["flags"][:30] == 0).all() and (nd["flags"][30:53] == 1).all() and (nd["flags"][53:] == 0).all()
        # (b) the default mask: content-dependent ranks
        got = check_batched_is_singles(m, pairs, poc, qp, "content-dependent", top=32, min_size=16)
        desc = [int((g["nodes"]["first_child"] >= 0).sum()) for g in got]
        print("device: descending 32 nodes per picture", desc)
        assert 0 in desc and max(desc) >= 1
        # the batched and the single call share the descent and its kernels, so (b) is also held against the descent driven from the HOST through predict_at:
        # picture 0, picture 28 (the end of the 4096-CU pass) and picture 34 (the end of the scan's 1024-node tile), byte for byte
        for p in (0, 28, 34):
            nodes, leaf_map, rec, host_reruns = host_tree(pkg, m, pairs[p][0], pairs[p][1], w, h, top=32, min_size=16, poc=int(poc[p]), qp=int(qp[p]))
            assert _same(got[p]["nodes"], nodes) and _same(got[p]["leaf_map"], leaf_map), p
            for k in ("logits", "decisions", "candidates"):
                assert _same(got[p][k], rec[k]), (p, k)
            # guard re-runs: the batched call's are the sum of the single calls' (check_batched_is_singles); a single call's are the host descent's
            r0 = _reruns(m, (32, 16))
            m.predict_tree(pairs[p][0], pairs[p][1], int(poc[p]), int(qp[p]), top=32, min_size=16, want=("leaf_map",))
            assert _reruns(m, (32, 16)) - r0 == host_reruns, (p, host_reruns)
    finally:
        close_all(pairs)


def test_content_that_the_guards_take(gpu, contexts, naturals):
    """A constant and a +-1 LSB dither picture among four natural ones; then under a confidence gate at 64, then a (0.9, 1) policy with MLT_TREE_BY_CANDIDATES."""
    rng = np.random.default_rng(77)
    const = (np.full((H, W), 512, np.int16), np.full((H, W), 508, np.int16))
    d_org = (600 + rng.integers(-1, 2, size=(H, W))).astype(np.int16)
    dither = (d_org, (d_org + rng.integers(-1, 2, size=(H, W))).astype(np.int16))
    pictures = [naturals(PIC_SEEDS[2]), const, naturals(PIC_SEEDS[0]), naturals(PIC_SEEDS[9]), dither, naturals(PIC_SEEDS[5])]
    poc, qp = np.zeros(6, np.int32), np.zeros(6, np.int32)
    m = contexts(13)
    pairs = upload_all(m, pictures)
    thr = float(np.float32(0.9))
    try:
        r0 = _reruns(m, SIZES)
        check_batched_is_singles(m, pairs, poc, qp, "guards")
        assert _reruns(m, SIZES) > r0, "the constant and the dither picture must reach the guards"
        m.set_confidence_gate(64, thr)
        got = check_batched_is_singles(m, pairs, poc, qp, "gate at 64")
        n64 = np.concatenate([g["nodes"][g["nodes"]["size"] == 64] for g in got])
        assert np.array_equal(n64["split_mode"] < 0, ~(n64["confidence"] >= np.float32(thr))) and (n64["first_child"][n64["split_mode"] < 0] == -1).all()
        m.set_confidence_gate(64, 0.0)
        for s in SIZES:
            m.set_candidate_policy(s, thr, 1)
        got = check_batched_is_singles(m, pairs, poc, qp, "by candidates", by_candidates=True)
        nd = np.concatenate([g["nodes"] for g in got])
        inner = nd["size"] > 16
        assert np.array_equal(nd["first_child"][inner] >= 0, (nd["cand_mask"][inner] & 2) != 0)
        assert np.array_equal(np.concatenate([g["candidates"]["mask"] for g in got]), nd["cand_mask"])
        # the policy alone, no records asked for: cand_mask still follows the policy
        check_batched_is_singles(m, pairs, poc, qp, "policy, lean", want=("leaf_map",))
    finally:
        m.set_confidence_gate(64, 0.0)
        for s in SIZES:
            m.set_candidate_policy(s, 0.0, 0)
        close_all(pairs)


def _wrap(m, plane, offset_elems, pitch):
    """plane [H, W] in a torch int16 tensor of offset_elems + H * pitch elements, sample (0, 0) at element offset_elems -> wrapped picture (the tensor is kept)."""
    import torch
    h, w = plane.shape
    host = np.random.default_rng(99).integers(0, 1024, size=offset_elems + h * pitch).astype(np.int16)
    host[offset_elems:offset_elems + h * pitch].reshape(h, pitch)[:, :w] = plane
    t = torch.from_numpy(host).to(torch.device("cuda", 0))
    assert t.data_ptr() % 16 == 0
    return m.wrap_picture(t.data_ptr() + 2 * offset_elems, pitch, w, h, keep=t)


def test_sources_of_different_alignment_in_one_call(gpu, contexts, naturals):
    """Entry 1: wrapped planes, odd stride, base 2 bytes off a 16-byte boundary (element path).  Entry 3: wrapped planes with both ends on 16 bytes (vector
    paths).  The others are library-owned.  Entries 0 and 4 share one org picture against different preds."""
    m = contexts(13)
    (o0, p0), (o1, p1), (o2, p2), (o3, p3), (_, p4) = (naturals(s) for s in PIC_SEEDS[3:8])
    # both ends on 16 bytes: (H - 1) pitch + W = 0 mod 8 elements; H - 1 is odd and W = 0 mod 8, so the pitch is a multiple of 8 (no odd stride can do it here)
    pitch = W + 8
    assert ((H - 1) * pitch + W) % 8 == 0
    own = upload_all(m, [(o0, p0), (o2, p2)])
    extra = m.picture(W, H).upload(p4)
    rough = (_wrap(m, o1, 1, W + 5), _wrap(m, p1, 9, W + 7))       # base 2 bytes (and 18 bytes) past a 16-byte boundary, odd strides
    smooth = (_wrap(m, o3, 0, pitch), _wrap(m, p3, 8, pitch))      # both ends aligned
    pairs = [own[0], rough, own[1], smooth, (own[0][0], extra)]
    poc, qp = np.array([0, 1, 2, 0, 0], np.int32), np.array([0, 0, 1, 1, 0], np.int32)
    try:
        got = check_batched_is_singles(m, pairs, poc, qp, "alignment")
        # the same org against two preds: two different trees or at least two different sets of logits
        assert not _same(got[0]["logits"], got[4]["logits"])
    finally:
        close_all(own + [rough, smooth])
        extra.close()


def test_one_picture_is_predict_tree(gpu, contexts, naturals):
    m = contexts(13)
    pairs = upload_all(m, [naturals(s) for s in PIC_SEEDS[4:5]])
    try:
        full = check_batched_is_singles(m, pairs, np.array([1], np.int32), np.array([0], np.int32), "P = 1")
        lean = check_batched_is_singles(m, pairs, np.array([1], np.int32), np.array([0], np.int32), "P = 1, lean", want=("leaf_map",))
        assert _same(lean[0]["nodes"], full[0]["nodes"]) and _same(lean[0]["leaf_map"], full[0]["leaf_map"]) and full[0]["first_node"] == 0
        assert sorted(lean[0]) == ["first_node", "leaf_map", "nodes"]
    finally:
        close_all(pairs)


def test_bad_arguments_launch_nothing(gpu, contexts, naturals):
    pkg = gpu
    m = contexts(13)
    other = _open(pkg, 13, sizes=(64, 16))   # 32 is missing between 64 and 16, and 128 above
    pairs = upload_all(m, [naturals(s) for s in PIC_SEEDS[6:9]])
    smaller = m.picture(W, H - 16).upload(naturals(PIC_SEEDS[6])[1][:H - 16])
    smaller_o = m.picture(W, H - 16).upload(naturals(PIC_SEEDS[6])[0][:H - 16])
    foreign = upload_all(other, [naturals(s) for s in PIC_SEEDS[6:9]])
    per = pkg.capi.tree_max_nodes(W, H)
    assert per == 576
    P = 3
    cap = P * per

    def call(ctx, prs, n=None, node_cap=cap, struct_size=None, top=128, mn=16, masks=(0, 0, 0, 0), flags=0, stride=15, null=()):
        n = len(prs) if n is None else n
        entries = (pkg.capi.MltTreePicture * max(len(prs), 1))()
        for i, (o, q) in enumerate(prs):
            entries[i].org, entries[i].pred, entries[i].poc, entries[i].qp = (o._h if o else None), (q._h if q else None), i % 3, i % 2
        cfg = pkg.capi.MltTreeConfig()
        cfg.struct_size = C.sizeof(pkg.capi.MltTreeConfig) if struct_size is None else struct_size
        cfg.top_size, cfg.min_size, cfg.flags = top, mn, flags
        for i, v in enumerate(masks):
            cfg.descend_mask[i] = v
        nodes = np.zeros(cap, pkg.capi.TREE_NODE_DTYPE)
        nodes["size"] = -7
        first = np.full(P + 1, -7, np.int32)
        lm = np.full((P, H // 16, W // 16), 0x5A, np.uint8)
        lg = np.full((cap, 15), -7.0, np.float32)
        dec = np.zeros(cap, pkg.capi.DECISION_DTYPE)
        cand = np.zeros(cap, pkg.capi.CANDIDATES_DTYPE)
        dec["raw_mode"] = -7
        cand["count"] = -7
        rc = ctx._lib.mlt_predict_trees(ctx._h, n, None if "pics" in null else entries, None if "cfg" in null else C.byref(cfg),
                                        None if "nodes" in null else nodes.ctypes.data, node_cap, None if "first" in null else first.ctypes.data, lm.ctypes.data,
                                        lg.ctypes.data, stride, dec.ctypes.data, cand.ctypes.data)
        untouched = ((first == -7).all() and (nodes["size"] == -7).all() and (lm == 0x5A).all() and (lg == -7.0).all() and (dec["raw_mode"] == -7).all()
                     and (cand["count"] == -7).all())
        return rc, bool(untouched), nodes, first, lm

    try:
        assert call(m, pairs, n=0)[:2] == (MLT_ERR_ARG, True)
        assert call(m, pairs, n=-1)[:2] == (MLT_ERR_ARG, True)
        assert call(m, pairs, n=257)[:2] == (MLT_ERR_ARG, True)
        for name in ("pics", "cfg", "nodes", "first"):
            assert call(m, pairs, null=(name,))[:2] == (MLT_ERR_ARG, True), name
        assert call(m, pairs, struct_size=C.sizeof(pkg.capi.MltTreeConfig) - 4)[:2] == (MLT_ERR_ARG, True)
        assert call(m, pairs[:2] + [(pairs[2][0], None)])[:2] == (MLT_ERR_ARG, True)                       # a NULL picture
        assert call(m, pairs[:2] + [(pairs[2][0], foreign[2][1])])[:2] == (MLT_ERR_ARG, True)              # a picture of another context in the last entry
        assert call(m, pairs[:2] + [(pairs[2][0], smaller)])[:2] == (MLT_ERR_ARG, True)                    # unequal geometry inside a pair
        assert call(m, pairs[:2] + [(smaller_o, smaller)])[:2] == (MLT_ERR_ARG, True)                      # ... and between entries
        assert call(m, pairs, node_cap=cap - 1)[:2] == (MLT_ERR_ARG, True)                                 # one node short
        assert call(m, pairs, stride=14)[:2] == (MLT_ERR_ARG, True)
        assert call(m, pairs, top=48)[:2] == (MLT_ERR_ARG, True)
        assert call(m, pairs, top=32, mn=64)[:2] == (MLT_ERR_ARG, True)
        assert call(m, pairs, masks=(0, 0b100, 0, 0))[:2] == (MLT_ERR_ARG, True)                           # head 0 of the 64 model has two classes
        assert call(m, pairs, flags=2)[:2] == (MLT_ERR_ARG, True)
        assert call(other, foreign, top=64)[:2] == (MLT_ERR_SIZE_DISABLED, True)                           # 32 not loaded between 64 and 16
        assert call(other, foreign)[:2] == (MLT_ERR_SIZE_DISABLED, True)                                   # 128 not loaded
        # a following valid call is still right
        rc, untouched, nodes, first, lm = call(m, pairs)
        assert rc == 0 and not untouched and first[0] == 0
        for i, (o, q) in enumerate(pairs):
            s = m.predict_tree(o, q, i % 3, i % 2, want=("leaf_map",))
            assert _same(nodes[first[i]:first[i + 1]], s["nodes"]) and _same(lm[i], s["leaf_map"]), i
    finally:
        close_all(pairs + [(smaller, smaller_o)])
        other.close()
