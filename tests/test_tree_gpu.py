"""GPU (MI355X): partition trees of a picture -- mlt_predict_tree against the same descent driven from the host through mlt_predict_at, and against the CPU oracle.

Between the two library paths every assertion is BYTE equality: the tree's network launches are mlt_predict_at's.  Against the oracle the bounds are the project's own,
none taken from what the device returns:
  LOGIT_TOL = 1e-3      the logit contract (tests/test_hip_parity.py)
  UNDECIDABLE = 4e-5    helpers.check_splits' band (2 x the exact arithmetic's noise): a reference top-2 margin at or below it is a tie of the reference's own
                        fp32 arithmetic.  The cases are chosen so that NO visited node of the reference tree lies inside it (cap 0) -- the test computes that from
                        the oracle alone and fails naming the node if this numpy build's FFTs (synth.natural_patches) move a margin into the band.
  CONF_TOL = 5e-4       two logits within LOGIT_TOL of the reference move a softmax probability by at most LOGIT_TOL / 2 (csrc/mlt_kernels.h: MLT_CONF_BAND_FRAC)
Structure (positions, order, parent / first_child, split_mode, cand_mask) and the leaf map must EQUAL the oracle's.

Contexts: all four sizes, head_index 0 at every size (lvl1, the reference's default for the CU models), descend_mask default, poc = qp = 0.  Seeded weights answer
almost constantly once the poc / qp terms enter; with poc = qp = 0 head 0 is mixed for weight seeds 12 and 13.  Picture 424 x 280: twelve natural patches of
128 x 128 tiled 4 x 3 and cropped (org from the org patches, pred from the pred patches): 6 roots at 128, none at 64, 8 at 32, 26 at 16."""
import ctypes as C

import numpy as np
import pytest

from tree_gpu_common import (LOGIT_TOL, MLT_ERR_ARG, MLT_ERR_SIZE_DISABLED, SIZES, TREE_ALL, UNDECIDABLE, H, W, blobs as _blobs, contexts, cut, gpu,   # noqa: F401  (fixtures)
                             natural_picture, open_context as _open, reruns as _reruns, same as _same)
from tree_host import host_tree   # the host descent (build_tree over predict_at)

pytestmark = pytest.mark.gpu
CONF_TOL = 5e-4
#        pic seed, weight seed
CASES = {"A": (8, 13), "B": (7, 12), "C": (7, 13)}


def device_tree(m, p_org, p_pred, want=TREE_ALL, sizes=SIZES, **kw):
    r0 = _reruns(m, sizes)
    out = m.predict_tree(p_org, p_pred, 0, 0, want=want, **kw)
    return out, _reruns(m, sizes) - r0


def check_device_is_host(pkg, m, p_org, p_pred, width, height, what, **kw):
    """mlt_predict_tree == build_tree over predict_at, byte for byte, guard re-runs included -> (device result, host nodes)."""
    sizes = [s for s in SIZES if kw.get("min_size", 16) <= s <= kw.get("top", 128)]
    nodes, leaf_map, rec, host_reruns = host_tree(pkg, m, p_org, p_pred, width, height, **kw)
    out, dev_reruns = device_tree(m, p_org, p_pred, sizes=sizes, **kw)
    assert out["nodes"].dtype == pkg.capi.TREE_NODE_DTYPE == nodes.dtype
    assert len(out["nodes"]) == len(nodes), (what, len(out["nodes"]), len(nodes))
    for f in nodes.dtype.names:
        assert np.array_equal(out["nodes"][f], nodes[f]), (what, f, np.flatnonzero(out["nodes"][f] != nodes[f])[:8])
    assert _same(out["nodes"], nodes), what
    assert _same(out["leaf_map"], leaf_map), what
    for k in ("logits", "decisions", "candidates"):
        assert _same(out[k], rec[k]), (what, k)
    assert dev_reruns == host_reruns, (what, dev_reruns, host_reruns)
    return out, nodes


def oracle_tree(pkg, blobs, org, pred, top=128, min_size=16):
    """build_tree driven by the CPU oracle -> (nodes, leaf_map, per-node logits [n, 15], per-node decision-head margin)."""
    import oracle
    nets = {s: oracle.Oracle(blobs[s]) for s in SIZES if min_size <= s <= top}
    lg_rows, margins = [], []

    def decide(size, xy):
        z = np.zeros(len(xy), np.int32)
        logits, split = nets[size].forward(cut(org, xy, size), cut(pred, xy, size), z, z, head_index=0)
        d = pkg.decisions.from_logits(size, logits, head_index=0)
        assert np.array_equal(d["raw_mode"], split)
        row = np.zeros((len(xy), 15), np.float32)
        row[:, :logits.shape[1]] = logits
        lg_rows.append(row)
        margins.append(d["margin"])
        return split, d["confidence"].astype(np.float32), (np.uint32(1) << split.astype(np.uint32))

    nodes, leaf_map = pkg.decisions.build_tree(org.shape[1], org.shape[0], top, min_size, None, decide)
    return nodes, leaf_map, np.concatenate(lg_rows), np.concatenate(margins)


def per_level(nodes):
    return [int((nodes["depth"] == d).sum()) for d in range(4)], [int(((nodes["depth"] == d) & (nodes["first_child"] >= 0)).sum()) for d in range(3)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_tree_is_the_host_descent_and_the_oracles(gpu, contexts, case):
    pkg = gpu
    pic_seed, weight_seed = CASES[case]
    org, pred = natural_picture(pkg, pic_seed)
    # the reference tree first, and the precondition on it: computed from the oracle alone
    ref_nodes, ref_map, ref_logits, ref_margin = oracle_tree(pkg, _blobs(pkg, weight_seed), org, pred)
    levels, descents = per_level(ref_nodes)
    print(f"case {case}: oracle nodes per level {levels}, descents {descents}, smallest top-2 margin {float(ref_margin.min()):.2e}")
    inside = np.flatnonzero(ref_margin <= UNDECIDABLE)
    assert len(inside) == 0, (f"case {case}: the reference cannot decide node {int(inside[0])} "
                              f"({int(ref_nodes['size'][inside[0]])} at {int(ref_nodes['x'][inside[0]])}, {int(ref_nodes['y'][inside[0]])}): margin {float(ref_margin[inside[0]]):.2e}")
    m = contexts(weight_seed)
    p_org, p_pred = m.picture(W, H).upload(org), m.picture(W, H).upload(pred)
    try:
        out, _ = check_device_is_host(pkg, m, p_org, p_pred, W, H, f"case {case}")
        # without candidate records the heads launch is not asked for them: cand_mask = 1 << raw_mode comes from the expand kernel, same bytes
        lean, _ = device_tree(m, p_org, p_pred, want=("leaf_map",))
        assert _same(lean["nodes"], out["nodes"]) and _same(lean["leaf_map"], out["leaf_map"])
        # the reference
        nodes = out["nodes"]
        assert len(nodes) == len(ref_nodes), (case, per_level(nodes), per_level(ref_nodes))
        for f in ("x", "y", "size", "depth", "flags", "parent", "first_child", "split_mode", "cand_mask"):
            assert np.array_equal(nodes[f], ref_nodes[f]), (case, f, np.flatnonzero(nodes[f] != ref_nodes[f])[:8])
        assert _same(out["leaf_map"], ref_map)
        err = float(np.abs(out["logits"] - ref_logits).max())
        dconf = float(np.abs(nodes["confidence"].astype(np.float64) - ref_nodes["confidence"]).max())
        print(f"case {case}: {len(nodes)} nodes, max|dlogit| vs oracle {err:.2e}, max|dconfidence| {dconf:.2e}")
        assert err <= LOGIT_TOL, err
        assert dconf <= CONF_TOL, dconf
    finally:
        p_org.close()
        p_pred.close()


def test_cases_together_mix_decisions_at_every_descending_level(gpu):
    """What the three cases are chosen for, from the oracle alone: at 128, 64 and 32 some node descends and some node does not."""
    pkg = gpu
    some, none = [False] * 3, [False] * 3
    for case, (pic_seed, weight_seed) in CASES.items():
        org, pred = natural_picture(pkg, pic_seed)
        nodes = oracle_tree(pkg, _blobs(pkg, weight_seed), org, pred)[0]
        levels, descents = per_level(nodes)
        for d in range(3):
            some[d] = some[d] or descents[d] > 0
            none[d] = none[d] or descents[d] < levels[d]
    assert all(some) and all(none), (some, none)


def test_a_level_longer_than_one_pass(gpu, contexts):
    """top 32 / min 16 with descend_mask[32] = 0b11 on 1056 x 1024: 1056 roots, 4224 children -- more than a pass of 4096 CUs holds."""
    pkg = gpu
    w, h = 1056, 1024
    rng = np.random.default_rng(3216)
    org = rng.integers(0, 1024, size=(h, w)).astype(np.int16)
    pred = np.clip(org.astype(np.int32) + rng.integers(-24, 25, size=(h, w)), 0, 1023).astype(np.int16)
    m = contexts(13)
    p_org, p_pred = m.picture(w, h).upload(org), m.picture(w, h).upload(pred)
    try:
        out, _ = check_device_is_host(pkg, m, p_org, p_pred, w, h, "long level", top=32, min_size=16, descend={32: 0b11})
        nodes = out["nodes"]
        assert len(nodes) == 1056 + 4224 and (nodes["size"][:1056] == 32).all() and (nodes["first_child"][:1056] == 1056 + 4 * np.arange(1056)).all()
        leaves = nodes[1056:]
        assert (leaves["size"] == 16).all() and (leaves["first_child"] == -1).all() and (leaves["flags"] == 0).all()
        want = np.zeros((h // 16, w // 16), np.uint8)
        want[leaves["y"] // 16, leaves["x"] // 16] = (leaves["split_mode"] + 1) << 4
        assert _same(out["leaf_map"], want) and ((out["leaf_map"] & 15) == 0).all()
    finally:
        p_org.close()
        p_pred.close()


def test_gate_and_candidates(gpu, contexts):
    """Case A under a confidence gate at 64 (withheld nodes are leaves), then under a (0.9, 1) policy with MLT_TREE_BY_CANDIDATES (unsure nodes descend)."""
    pkg = gpu
    pic_seed, weight_seed = CASES["A"]
    org, pred = natural_picture(pkg, pic_seed)
    m = contexts(weight_seed)
    p_org, p_pred = m.picture(W, H).upload(org), m.picture(W, H).upload(pred)
    thr = float(np.float32(0.9))
    # a second threshold that SPLITS the 64 level, from the oracle alone: the middle of the widest gap between the reference confidences of its 20 nodes (the gate at
    # 64 does not change which 64 nodes are visited); the gap must clear the confidence contract on both sides
    ref_nodes = oracle_tree(pkg, _blobs(pkg, weight_seed), org, pred)[0]
    c64 = np.sort(ref_nodes["confidence"][ref_nodes["size"] == 64].astype(np.float64))
    g = int(np.argmax(np.diff(c64)))
    assert c64[g + 1] - c64[g] > 4 * CONF_TOL, "the reference confidences at 64 leave no gap for a threshold"
    mid = float(np.float32(0.5 * (c64[g] + c64[g + 1])))
    try:
        for t, expect in ((thr, None), (mid, len(c64) - g - 1)):
            m.set_confidence_gate(64, t)
            out, nodes = check_device_is_host(pkg, m, p_org, p_pred, W, H, f"gate {t}")
            n64 = out["nodes"][out["nodes"]["size"] == 64]
            withheld = n64["split_mode"] < 0
            print(f"gate {t} at 64: {int(withheld.sum())} of {len(n64)} nodes withheld")
            assert len(n64) == len(c64) and np.array_equal(withheld, ~(n64["confidence"] >= np.float32(t)))
            assert expect is None or int((~withheld).sum()) == expect, (int((~withheld).sum()), expect)
            assert (n64["first_child"][withheld] == -1).all()
            sure_qt = ~withheld & (n64["split_mode"] == 1)
            assert (n64["first_child"][sure_qt] >= 0).all()
            for by, x in zip(*np.nonzero((out["leaf_map"] >> 4) == 0)):   # map bytes of withheld leaves: split_mode + 1 == 0
                assert (out["leaf_map"][by, x] & 15) == 2
        m.set_confidence_gate(64, 0.0)
        for s in SIZES:
            m.set_candidate_policy(s, thr, 1)
        out, nodes = check_device_is_host(pkg, m, p_org, p_pred, W, H, "by candidates", by_candidates=True)
        nd = out["nodes"]
        inner = nd["size"] > 16
        unsure = inner & (nd["cand_mask"] == 0b11)   # head 0 has two classes at every size
        print(f"policy ({thr}, 1): {int(unsure.sum())} of {int(inner.sum())} inner nodes keep every class")
        assert (nd["first_child"][unsure] >= 0).all()
        assert np.array_equal(nd["first_child"][inner] >= 0, (nd["cand_mask"][inner] & 2) != 0)
        assert np.array_equal(out["candidates"]["mask"], nd["cand_mask"])
        # the policy alone (no BY_CANDIDATES, no candidate records asked for): cand_mask still follows the policy
        lean, _ = device_tree(m, p_org, p_pred, want=("leaf_map",))
        hn, hm, _, _ = host_tree(pkg, m, p_org, p_pred, W, H)
        assert _same(lean["nodes"], hn) and _same(lean["leaf_map"], hm)
    finally:
        m.set_confidence_gate(64, 0.0)
        for s in SIZES:
            m.set_candidate_policy(s, 0.0, 0)
        p_org.close()
        p_pred.close()


def test_top_64_min_32(gpu, contexts):
    pkg = gpu
    org, pred = natural_picture(pkg, CASES["A"][0])
    m = contexts(13)
    p_org, p_pred = m.picture(W, H).upload(org), m.picture(W, H).upload(pred)
    try:
        out, _ = check_device_is_host(pkg, m, p_org, p_pred, W, H, "64..32", top=64, min_size=32)
        nd = out["nodes"]
        assert set(np.unique(nd["size"])) == {64, 32}
        roots = nd[nd["parent"] < 0]
        assert (roots["size"] == 64).sum() == 24 and (roots["flags"][roots["size"] == 64] == 0).all()
        border = roots[roots["size"] == 32]
        assert len(border) == 8 and (border["flags"] == 1).all() and (border["x"] == 384).all() and border["y"].tolist() == list(range(0, 256, 32))
        assert (nd["flags"][nd["parent"] >= 0] == 0).all()
        lm = out["leaf_map"]
        assert lm.shape == (17, 26) and (lm[16, :] == 0xFF).all() and (lm[:16, :] != 0xFF).all()   # the row y = 256 holds complete 16-blocks only
    finally:
        p_org.close()
        p_pred.close()


def test_bad_arguments_launch_nothing(gpu, contexts):
    pkg = gpu
    org, pred = natural_picture(pkg, CASES["A"][0])
    m = contexts(13)
    other = _open(pkg, 13, sizes=(64, 16))   # 32 is missing between 64 and 16
    p_org, p_pred = m.picture(W, H).upload(org), m.picture(W, H).upload(pred)
    smaller = m.picture(W, H - 16).upload(pred[:H - 16])
    f_org, f_pred = other.picture(W, H).upload(org), other.picture(W, H).upload(pred)
    cap = pkg.capi.tree_max_nodes(W, H)
    assert cap == 6 + 24 + 104 + 442

    def call(ctx, a, b, node_cap=cap, struct_size=None, top=128, mn=16, masks=(0, 0, 0, 0), flags=0, stride=15, nodes_null=False):
        cfg = pkg.capi.MltTreeConfig()
        cfg.struct_size = C.sizeof(pkg.capi.MltTreeConfig) if struct_size is None else struct_size
        cfg.top_size, cfg.min_size, cfg.flags = top, mn, flags
        for i, v in enumerate(masks):
            cfg.descend_mask[i] = v
        nodes = np.zeros(cap, pkg.capi.TREE_NODE_DTYPE)
        nodes["size"] = -7
        lm = np.full((H // 16, W // 16), 0x5A, np.uint8)
        lg = np.full((cap, 15), -7.0, np.float32)
        dec = np.zeros(cap, pkg.capi.DECISION_DTYPE)
        cand = np.zeros(cap, pkg.capi.CANDIDATES_DTYPE)
        dec["raw_mode"] = -7
        cand["count"] = -7
        n = C.c_int(-7)
        rc = ctx._lib.mlt_predict_tree(ctx._h, a._h, b._h, C.byref(cfg), None if nodes_null else nodes.ctypes.data, node_cap, C.byref(n), lm.ctypes.data,
                                       lg.ctypes.data, stride, dec.ctypes.data, cand.ctypes.data)
        untouched = (n.value == -7 and (nodes["size"] == -7).all() and (lm == 0x5A).all() and (lg == -7.0).all() and (dec["raw_mode"] == -7).all()
                     and (cand["count"] == -7).all())
        return rc, untouched, nodes[:max(n.value, 0)], lm

    try:
        assert call(m, p_org, p_pred, node_cap=cap - 1)[:2] == (MLT_ERR_ARG, True)                      # one node short
        assert call(other, f_org, f_pred, top=64)[:2] == (MLT_ERR_SIZE_DISABLED, True)                  # 32 not loaded between 64 and 16
        assert call(other, f_org, f_pred)[:2] == (MLT_ERR_SIZE_DISABLED, True)                          # 128 not loaded
        assert call(m, p_org, f_pred)[:2] == (MLT_ERR_ARG, True)                                        # a picture of another context
        assert call(m, p_org, smaller)[:2] == (MLT_ERR_ARG, True)                                       # pictures of different geometry
        assert call(m, p_org, p_pred, masks=(0, 0b100, 0, 0))[:2] == (MLT_ERR_ARG, True)                # head 0 of the 64 model has two classes
        assert call(m, p_org, p_pred, struct_size=C.sizeof(pkg.capi.MltTreeConfig) - 4)[:2] == (MLT_ERR_ARG, True)
        assert call(m, p_org, p_pred, top=32, mn=64)[:2] == (MLT_ERR_ARG, True)
        assert call(m, p_org, p_pred, top=48)[:2] == (MLT_ERR_ARG, True)
        assert call(m, p_org, p_pred, stride=14)[:2] == (MLT_ERR_ARG, True)
        assert call(m, p_org, p_pred, flags=2)[:2] == (MLT_ERR_ARG, True)
        assert call(m, p_org, p_pred, nodes_null=True)[:2] == (MLT_ERR_ARG, True)
        # a following valid call is still right
        rc, untouched, nodes, lm = call(m, p_org, p_pred)
        hn, hm, _, _ = host_tree(pkg, m, p_org, p_pred, W, H)
        assert rc == 0 and not untouched and _same(nodes, hn) and _same(lm, hm)
    finally:
        for p in (p_org, p_pred, smaller):
            p.close()
        other.close()


def test_two_device_context_returns_the_single_device_bytes(gpu, contexts):
    pkg = gpu
    org, pred = natural_picture(pkg, CASES["A"][0])
    m1 = contexts(13)
    a, b = m1.picture(W, H).upload(org), m1.picture(W, H).upload(pred)
    one = m1.predict_tree(a, b, 0, 0, want=TREE_ALL)
    a.close()
    b.close()
    m2 = _open(pkg, 13, devices=[0, 0])
    try:
        assert m2.num_devices() == 2
        two = m2.predict_tree(m2.picture(W, H).upload(org), m2.picture(W, H).upload(pred), 0, 0, want=TREE_ALL)
        for k in ("nodes",) + TREE_ALL:
            assert _same(one[k], two[k]), k
    finally:
        m2.close()
