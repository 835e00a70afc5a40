"""Host restatement of the device's decision records (include/mltcnn.h: mlt_decision), in float64.

`from_logits` turns an [n, num_logits] array of head logits (lvl1..lvlN concatenated, as every entry point returns them) into the records
heads_kernel writes: per head the first-max argmax (torch.argmax) and its softmax probability, the decision head's top-2 margin, and the
confidence gate.  It is what the tests compare the device against, the way synth.flat_quad_fraction restates the flat statistic, and what
tools/confidence_sweep.py evaluates on a call dump.

`candidates_from_logits` restates the candidate records (include/mltcnn.h: mlt_candidates) the same way: rank, softmax, prefix sums, kept count, cap, mask,
with the device's tie and NaN rules; tools/candidate_sweep.py evaluates it on a call dump.

`build_tree` restates the partition tree of a picture (include/mltcnn.h: mlt_predict_tree): levels, border roots, node order, descent rule and leaf map, with the
network behind a callback -- the device's tree driven from the host, or any other decider's.  `build_trees_sweep` restates the union descent of
mlt_predict_trees_sweep (several entries, several points each) the same way; `build_tree_sweep` (mlt_predict_tree_sweep) is that with one entry."""
from __future__ import annotations

import numpy as np

HEAD_CLASSES = {128: (2, 3, 4), 64: (2, 3, 4, 6), 32: (2, 3, 4, 6), 16: (2, 3, 4, 6)}
# float64 twin of capi.DECISION_DTYPE (same field names and shapes)
DTYPE = np.dtype([("split_mode", "<i4"), ("raw_mode", "<i4"), ("confidence", "<f8"), ("margin", "<f8"),
                  ("level_mode", "<i4", (4,)), ("level_conf", "<f8", (4,))])


def default_head(size: int) -> int:
    """The reference's decision head: element [2] for the 128 model, [0] otherwise (EncCu.cpp:913-919)."""
    return 2 if size == 128 else 0


def from_logits(size: int, logits, head_index: int | None = None, min_confidence: float = 0.0) -> np.ndarray:
    """The decision records of [n, num_logits] logits.  The margin is defined for finite logits: the device starts its top-2 scan from -3.4e38 and a NaN never
    wins a comparison there, so a -inf logit gives a margin of 3.4e38 on the device and inf here, and a row with a NaN the margin of its other classes on the
    device and NaN here (its argmax is np.argmax's here, the NaN, and the comparison scan's on the device)."""
    classes = HEAD_CLASSES[size]
    lg = np.asarray(logits, np.float64)
    if lg.ndim == 1:
        lg = lg[None, :]
    assert lg.ndim == 2 and lg.shape[1] == sum(classes), (lg.shape, classes)
    dh = default_head(size) if head_index is None or head_index < 0 else head_index
    assert 0 <= dh < len(classes)
    out = np.zeros((lg.shape[0],), DTYPE)
    out["level_mode"] = -1
    rows = np.arange(lg.shape[0])
    lo = 0
    for h, k in enumerate(classes):
        l = lg[:, lo:lo + k]
        lo += k
        best = np.argmax(l, axis=1)   # first maximal index
        e = np.exp(l - l[rows, best][:, None])
        s = np.zeros(lg.shape[0])
        for c in range(k):            # class order, like the device
            s = s + e[:, c]
        out["level_mode"][:, h] = best
        out["level_conf"][:, h] = 1.0 / s
        if h == dh:
            top = np.sort(l, axis=1)
            out["raw_mode"] = best
            out["confidence"] = 1.0 / s
            out["margin"] = top[:, -1] - top[:, -2]
    passed = out["confidence"] >= min_confidence if min_confidence > 0.0 else np.ones(lg.shape[0], bool)   # (a NaN confidence gates)
    out["split_mode"] = np.where(passed, out["raw_mode"], -1)
    return out


# float64 twin of capi.CANDIDATES_DTYPE (same leading fields), followed by what the record is derived from: the prefix sums in rank order (0 beyond K), the
# kept count before the cap, and the logit gap between the last kept and the first dropped class (inf when nothing is dropped)
CAND_DTYPE = np.dtype([("mask", "<u4"), ("count", "<i4"), ("order", "i1", (8,)), ("prob", "<f8", (6,)),
                       ("cum", "<f8", (6,)), ("n", "<i4"), ("gap", "<f8")])


def candidates_from_logits(size: int, logits, head_index: int | None = None, coverage: float = 0.0, max_modes: int = 0) -> np.ndarray:
    """Candidate set of the decision head per CU: classes ranked by logit (descending, equal logits in class order), softmax summed in class order, prefix
    sums in rank order, the shortest prefix with cum >= coverage (all K if none reaches it), all K when that prefix is longer than max_modes > 0 or a logit
    of the head is NaN (order then lists the classes in class order)."""
    classes = HEAD_CLASSES[size]
    lg = np.asarray(logits, np.float64)
    if lg.ndim == 1:
        lg = lg[None, :]
    assert lg.ndim == 2 and lg.shape[1] == sum(classes), (lg.shape, classes)
    dh = default_head(size) if head_index is None or head_index < 0 else head_index
    assert 0 <= dh < len(classes)
    K = classes[dh]
    assert 0.0 <= coverage < 1.0 and 0 <= max_modes <= K, (coverage, max_modes)
    lo = sum(classes[:dh])
    l = lg[:, lo:lo + K]
    n_cu = l.shape[0]
    rows = np.arange(n_cu)
    nan = np.isnan(l).any(axis=1)
    order = np.argsort(-np.where(np.isnan(l), -np.inf, l), axis=1, kind="stable")   # descending, equal logits keep class order
    order[nan] = np.arange(K)
    best = np.zeros(n_cu, np.int64)     # first-max argmax the way the device finds it (a NaN never wins a comparison)
    for k in range(1, K):
        best = np.where(l[:, k] > l[rows, best], k, best)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(l - l[rows, best][:, None])
        s = np.zeros(n_cu)
        for c in range(K):              # class order, like the device
            s = s + e[:, c]
        prob = e / s[:, None]
    out = np.zeros((n_cu,), CAND_DTYPE)
    out["order"] = -1
    out["order"][:, :K] = order
    out["prob"][:, :K] = prob
    cum = np.zeros(n_cu)
    kept = np.full(n_cu, K, np.int32)
    found = np.zeros(n_cu, bool)
    for r in range(K):                  # rank order
        cum = cum + prob[rows, order[:, r]]
        out["cum"][:, r] = cum
        hit = ~found & (cum >= coverage)
        kept[hit] = r + 1
        found |= hit
    out["n"] = kept
    full = nan | ((kept > max_modes) if max_modes > 0 else np.zeros(n_cu, bool))
    count = np.where(full, K, kept)
    mask = np.zeros(n_cu, np.uint32)
    for r in range(K):
        mask |= np.where(r < count, np.uint32(1) << order[:, r].astype(np.uint32), np.uint32(0)).astype(np.uint32)
    out["mask"] = mask
    out["count"] = count
    srt = l[rows[:, None], order]
    gap = np.full(n_cu, np.inf)
    drop = count < K
    with np.errstate(invalid="ignore"):
        gap[drop] = srt[drop, count[drop] - 1] - srt[drop, np.minimum(count[drop], K - 1)]
    out["gap"] = gap
    return out


# the layout of capi.TREE_NODE_DTYPE (include/mltcnn.h: mlt_tree_node), restated here so that this module stays free of the library
TREE_NODE_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("size", "<i2"), ("depth", "i1"), ("flags", "u1"), ("parent", "<i4"), ("first_child", "<i4"),
                            ("split_mode", "<i4"), ("confidence", "<f4"), ("cand_mask", "<u4")])
TREE_SIZES = (128, 64, 32, 16)


def tree_roots(width: int, height: int, top: int, size: int) -> np.ndarray:
    """[count, 2] int32 {x, y}, raster order: at `top` the complete CUs of the aligned grid; below, the complete size-aligned CUs whose enclosing 2 x size-aligned
    block is not complete (mlt_tree_roots)."""
    if top not in TREE_SIZES or size not in TREE_SIZES or size > top:
        return np.zeros((0, 2), np.int32)
    ys, xs = np.meshgrid(np.arange(height // size, dtype=np.int32) * size, np.arange(width // size, dtype=np.int32) * size, indexing="ij")
    xy = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32).reshape(-1, 2)
    if size == top:
        return xy
    p = 2 * size
    whole = (xy[:, 0] // p * p + p <= width) & (xy[:, 1] // p * p + p <= height)
    return xy[~whole]


def tree_max_nodes(width: int, height: int, top: int = 128, min_size: int = 16) -> int:
    if top not in TREE_SIZES or min_size not in TREE_SIZES or min_size > top or not (16 <= width <= 16384 and 16 <= height <= 16384):
        return 0
    return sum((width // s) * (height // s) for s in TREE_SIZES if min_size <= s <= top)


def build_tree(width: int, height: int, top: int, min_size: int, descend_mask, decide, by_candidates: bool = False):
    """The partition tree in the contract's order, on the host.  descend_mask: {size: mask} (a missing or zero entry: 1 << 1).  decide(size, xy) -> (split_mode,
    confidence, cand_mask), one entry per row of the [n, 2] int32 position list -- called once per level with at least one node, top level first.
    -> (nodes TREE_NODE_DTYPE [n], leaf_map uint8 [height // 16, width // 16])."""
    assert top in TREE_SIZES and min_size in TREE_SIZES and min_size <= top
    levels = [s for s in TREE_SIZES if min_size <= s <= top]
    leaf_map = np.full((height // 16, width // 16), 0xFF, np.uint8)
    done = []
    start = 0
    prev = None          # the previous level's nodes (first_child filled in as their children are emitted)
    for depth, size in enumerate(levels):
        roots = tree_roots(width, height, top, size)
        lvl = np.zeros((len(roots),), TREE_NODE_DTYPE)
        lvl["x"], lvl["y"], lvl["parent"], lvl["flags"] = roots[:, 0], roots[:, 1], -1, (0 if size == top else 1)
        if prev is not None:
            par = np.flatnonzero(prev["_descends"])
            kids = np.zeros((4 * len(par),), TREE_NODE_DTYPE)
            for j in range(4):   # z-order: TL, TR, BL, BR
                kids["x"][j::4] = prev["nodes"]["x"][par] + (j & 1) * size
                kids["y"][j::4] = prev["nodes"]["y"][par] + (j >> 1) * size
                kids["parent"][j::4] = prev["start"] + par
            prev["nodes"]["first_child"][par] = start + len(roots) + 4 * np.arange(len(par))
            lvl = np.concatenate([lvl, kids])
        lvl["size"], lvl["depth"], lvl["first_child"] = size, depth, -1
        descends = np.zeros(len(lvl), bool)
        if len(lvl):
            xy = np.stack([lvl["x"], lvl["y"]], axis=1).astype(np.int32)
            split, conf, cmask = decide(size, xy)
            lvl["split_mode"], lvl["confidence"], lvl["cand_mask"] = np.asarray(split), np.asarray(conf), np.asarray(cmask)
            if size > min_size:
                mask = int((descend_mask or {}).get(size, 0)) or 2
                if by_candidates:
                    descends = (lvl["cand_mask"] & np.uint32(mask)) != 0
                else:
                    sm = lvl["split_mode"].astype(np.int64)
                    descends = (sm >= 0) & (((mask >> np.clip(sm, 0, 31)) & 1) != 0)
        prev = {"nodes": lvl, "_descends": descends, "start": start}
        done.append(lvl)
        start += len(lvl)
    nodes = np.concatenate(done) if done else np.zeros((0,), TREE_NODE_DTYPE)
    for size in levels:   # leaves are disjoint: every block of a leaf takes (log2(size) - 4) | ((split_mode + 1) << 4)
        lv = nodes[(nodes["first_child"] < 0) & (nodes["size"] == size)]
        val = ((size.bit_length() - 5) | ((lv["split_mode"] + 1) << 4)).astype(np.uint8)
        for dy in range(size // 16):
            for dx in range(size // 16):
                leaf_map[lv["y"] // 16 + dy, lv["x"] // 16 + dx] = val
    return nodes, leaf_map


def build_tree_sweep(width: int, height: int, top: int, min_size: int, descend_mask, decide, n_points: int, by_candidates: bool = False):
    """The union descent of mlt_predict_tree_sweep restated on the host: the trees of one picture under n_points points from ONE descent over their union.
    decide(size, xy) -> (split_mode, confidence, cand_mask), each [n_points, n]: the records of EVERY point for the [n, 2] position list -- called once per
    level with at least one union node.  A union node carries `alive` (bit q: part of tree q) and `desc` (bit q: it descends under point q, build_tree's rule on
    point q's record); it descends in the union iff desc != 0 and its four children are alive under desc; roots are alive under every point.  Tree q is then
    the ordered compaction of every union level by bit q, parent / first_child renumbered inside the slice.
    -> ([(nodes TREE_NODE_DTYPE [n_q], leaf_map uint8 [height // 16, width // 16]) per point], union_nodes int32 [4]: union nodes per level from `top` down)."""
    (trees, counts), = build_trees_sweep(width, height, top, min_size, descend_mask, lambda size, pic, xy: decide(size, xy), 1, n_points, by_candidates=by_candidates)
    return trees, counts


def build_trees_sweep(width: int, height: int, top: int, min_size: int, descend_mask, decide, n_pictures: int, n_points: int, by_candidates: bool = False):
    """The union descent of mlt_predict_trees_sweep restated on the host: the trees of n_pictures entries of one geometry under n_points points each from ONE
    descent.  A level is one list over all entries -- entry 0's union segment (its border roots, then four children per node with desc != 0), entry 1's, ... --
    and decide(size, pic_index, xy) -> (split_mode, confidence, cand_mask), each [n_points, n], gives the records of EVERY point for that list (pic_index [n]
    int32, xy [n, 2] int32); it is called once per level with at least one node.  Inside an entry the rules are build_tree_sweep's.
    -> [(trees, union_nodes) per entry], each as build_tree_sweep returns them."""
    assert top in TREE_SIZES and min_size in TREE_SIZES and min_size <= top and 1 <= n_points <= 32 and n_pictures >= 1
    P, Q = n_pictures, n_points
    levels = [s for s in TREE_SIZES if min_size <= s <= top]
    everyone = np.uint32((1 << Q) - 1)   # (Python integers: no shift by 32)
    unions = [[] for _ in range(P)]      # per entry, per level: build_tree_sweep's level
    for size in levels:
        roots = tree_roots(width, height, top, size)
        segs = []
        for p in range(P):
            prev = unions[p][-1] if unions[p] else None
            x, y = roots[:, 0].astype(np.int32), roots[:, 1].astype(np.int32)
            parent = np.full(len(roots), -1, np.int64)
            alive = np.full(len(roots), everyone, np.uint32)
            flags = np.full(len(roots), 0 if size == top else 1, np.uint8)
            if prev is not None:
                par = np.flatnonzero(prev["desc"] != 0)
                prev["first"][par] = len(roots) + 4 * np.arange(len(par))
                j = np.tile(np.arange(4), len(par))   # z-order: TL, TR, BL, BR
                x = np.concatenate([x, np.repeat(prev["x"][par], 4) + (j & 1) * size]).astype(np.int32)
                y = np.concatenate([y, np.repeat(prev["y"][par], 4) + (j >> 1) * size]).astype(np.int32)
                parent = np.concatenate([parent, np.repeat(par, 4)])
                alive = np.concatenate([alive, np.repeat(prev["desc"][par], 4)]).astype(np.uint32)
                flags = np.concatenate([flags, np.zeros(4 * len(par), np.uint8)])
            n = len(x)
            segs.append({"size": size, "x": x, "y": y, "flags": flags, "parent": parent, "alive": alive, "desc": np.zeros(n, np.uint32), "first": np.full(n, -1, np.int64),
                         "split": np.zeros((Q, n), np.int32), "conf": np.zeros((Q, n), np.float32), "cmask": np.zeros((Q, n), np.uint32)})
        total = sum(len(s["x"]) for s in segs)
        if total:
            xy = np.stack([np.concatenate([s["x"] for s in segs]), np.concatenate([s["y"] for s in segs])], axis=1).astype(np.int32)
            pic = np.concatenate([np.full(len(s["x"]), p, np.int32) for p, s in enumerate(segs)])
            split, conf, cmask = (np.asarray(a).reshape(Q, total) for a in decide(size, pic, xy))
            at = 0
            for lvl in segs:
                n = len(lvl["x"])
                lvl["split"], lvl["conf"], lvl["cmask"] = split[:, at:at + n].astype(np.int32), conf[:, at:at + n].astype(np.float32), cmask[:, at:at + n].astype(np.uint32)
                at += n
                if size > min_size and n:
                    mask = int((descend_mask or {}).get(size, 0)) or 2
                    for q in range(Q):
                        if by_candidates:
                            d = (lvl["cmask"][q] & np.uint32(mask)) != 0
                        else:
                            sm = lvl["split"][q].astype(np.int64)
                            d = (sm >= 0) & (((mask >> np.clip(sm, 0, 31)) & 1) != 0)
                        d &= ((lvl["alive"] >> np.uint32(q)) & np.uint32(1)) != 0
                        lvl["desc"] |= (d.astype(np.uint32) << np.uint32(q)).astype(np.uint32)
        for p in range(P):
            unions[p].append(segs[p])
    return [(_slices_of_union(unions[p], Q, width, height, levels), _union_counts(unions[p])) for p in range(P)]


def _union_counts(union) -> np.ndarray:
    counts = np.zeros(4, np.int32)
    counts[:len(union)] = [len(l["x"]) for l in union]
    return counts


def _slices_of_union(union, Q: int, width: int, height: int, levels):
    """Tree q of a union (build_tree_sweep's levels): the ordered compaction of every level by bit q of alive, parent / first_child renumbered inside the slice,
    and its leaf map."""
    trees = []
    for q in range(Q):
        bit = lambda m: ((m >> np.uint32(q)) & np.uint32(1)) != 0
        idx, base = [], 0     # per level: a union node's index inside slice q (-1: not part of it)
        for lvl in union:
            on = bit(lvl["alive"])
            idx.append(np.where(on, base + np.cumsum(on) - 1, -1))
            base += int(on.sum())
        nodes = np.zeros(base, TREE_NODE_DTYPE)
        for l, lvl in enumerate(union):
            on = np.flatnonzero(bit(lvl["alive"]))
            if not len(on):
                continue
            r = nodes[idx[l][on]]
            r["x"], r["y"], r["size"], r["depth"], r["flags"] = lvl["x"][on], lvl["y"][on], lvl["size"], l, lvl["flags"][on]
            p = lvl["parent"][on]
            r["parent"] = np.where(p >= 0, idx[l - 1][np.maximum(p, 0)], -1) if l and (p >= 0).any() else -1
            down = bit(lvl["desc"][on])
            r["first_child"] = np.where(down, idx[l + 1][np.maximum(lvl["first"][on], 0)], -1) if l + 1 < len(union) and down.any() else -1
            r["split_mode"], r["confidence"], r["cand_mask"] = lvl["split"][q][on], lvl["conf"][q][on], lvl["cmask"][q][on]
            nodes[idx[l][on]] = r
        leaf_map = np.full((height // 16, width // 16), 0xFF, np.uint8)
        for size in levels:
            lv = nodes[(nodes["first_child"] < 0) & (nodes["size"] == size)]
            val = ((size.bit_length() - 5) | ((lv["split_mode"] + 1) << 4)).astype(np.uint8)
            for dy in range(size // 16):
                for dx in range(size // 16):
                    leaf_map[lv["y"] // 16 + dy, lv["x"] // 16 + dx] = val
        trees.append((nodes, leaf_map))
    return trees
