"""CPU: partition trees of a picture -- the new exports, mlt_tree_roots / mlt_tree_max_nodes against numpy, the NULL-context error path, decisions.build_tree on
scripted deciders (order, parent / first_child, tiling, map bytes) and the argument handling of tools/picture_map.py --tree.  No device call here."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mlt_tree_max_nodes", "mlt_tree_roots", "mlt_predict_tree")
SIZES = (128, 64, 32, 16)
MLT_ERR_ARG = 1
GEOMETRIES = ((424, 280), (1920, 1080), (832, 480), (16, 16), (129, 257), (16384, 48))


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build.build_lib()
    return pkg.capi.load_library()


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("picture_map", os.path.join(ROOT, "tools", "picture_map.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def numpy_roots(w, h, top, s):
    """The contract, spelt out: complete s-aligned CUs in raster order; below the top level only those whose enclosing 2s-aligned block is not complete."""
    out = []
    for y in range(0, h - s + 1, s):
        for x in range(0, w - s + 1, s):
            bx, by = x // (2 * s) * 2 * s, y // (2 * s) * 2 * s
            if s == top or bx + 2 * s > w or by + 2 * s > h:
                out.append((x, y))
    return np.array(out, np.int32).reshape(-1, 2)


def test_new_names_are_exported_and_declared(pkg, lib):
    header = open(os.path.join(ROOT, "include", "mltcnn.h")).read()
    declared = set(re.findall(r"\b(mlt_[a-z_0-9]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in mltcnn.h"
        assert name in pkg.capi.EXPORTS, f"{name} is missing from capi.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert getattr(lib, name).argtypes is not None, f"{name} has no argtypes"
    assert "} mlt_tree_config;" in header and "} mlt_tree_node;" in header and "#define MLT_TREE_BY_CANDIDATES 0x1u" in header
    assert lib.mlt_abi_version() == 4
    assert pkg.capi.TREE_NODE_DTYPE.itemsize == 32 and pkg.capi.TREE_NODE_DTYPE == pkg.decisions.TREE_NODE_DTYPE
    assert [pkg.capi.TREE_NODE_DTYPE.fields[f][1] for f in ("x", "y", "size", "depth", "flags", "parent", "first_child", "split_mode", "confidence", "cand_mask")] == \
        [0, 4, 8, 10, 11, 12, 16, 20, 24, 28]
    assert C.sizeof(pkg.capi.MltTreeConfig) == 40
    assert callable(pkg.capi.tree_roots) and callable(pkg.capi.tree_max_nodes) and hasattr(pkg.capi.MltCnn, "predict_tree")


def test_roots_and_max_nodes_against_numpy(pkg, lib):
    assert [len(pkg.capi.tree_roots(424, 280, 128, s)) for s in SIZES] == [6, 0, 8, 26]
    assert (pkg.capi.tree_roots(424, 280, 128, 32)[:, 0] == 384).all() and (pkg.capi.tree_roots(424, 280, 128, 16)[:, 1] == 256).all()
    assert pkg.capi.tree_max_nodes(1920, 1080) == 120 + 480 + 1980 + 8040
    for w, h in GEOMETRIES:
        for top in SIZES:
            for s in SIZES:
                got = pkg.capi.tree_roots(w, h, top, s)
                want = numpy_roots(w, h, top, s) if s <= top else np.zeros((0, 2), np.int32)
                assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (w, h, top, s)
                assert np.array_equal(pkg.decisions.tree_roots(w, h, top, s), want), (w, h, top, s)
            for mn in SIZES:
                want = sum((w // s) * (h // s) for s in SIZES if mn <= s <= top) if mn <= top else 0
                assert lib.mlt_tree_max_nodes(w, h, top, mn) == want == pkg.decisions.tree_max_nodes(w, h, top, mn), (w, h, top, mn)
    # 0 stands for the defaults (128 / 16); anything else that is no CU size, or a picture outside 16 .. 16384, gives 0
    assert lib.mlt_tree_max_nodes(424, 280, 0, 0) == lib.mlt_tree_max_nodes(424, 280, 128, 16) == 576
    assert lib.mlt_tree_roots(424, 280, 0, 128, None, 0) == 6
    for top, mn in ((48, 16), (128, 8), (256, 16), (-128, 16), (32, 64)):
        assert lib.mlt_tree_max_nodes(424, 280, top, mn) == 0, (top, mn)
    for w, h in ((15, 200), (200, 15), (16385, 64)):
        assert lib.mlt_tree_max_nodes(w, h, 128, 16) == 0
        assert all(lib.mlt_tree_roots(w, h, 128, s, None, 0) == 0 for s in SIZES)
    for s in (8, 0, 24, 256):
        assert lib.mlt_tree_roots(424, 280, 128, s, None, 0) == 0, s
    assert lib.mlt_tree_roots(424, 280, 32, 64, None, 0) == 0   # a level above the top
    # a cap below the count: only `cap` entries are written, the count is still returned
    full = numpy_roots(424, 280, 128, 16)
    buf = np.full((len(full), 2), -7, np.int32)
    assert lib.mlt_tree_roots(424, 280, 128, 16, buf.ctypes.data, 10) == len(full) == 26
    assert np.array_equal(buf[:10], full[:10]) and (buf[10:] == -7).all()


@pytest.mark.parametrize("top", SIZES)
def test_roots_of_all_levels_tile_the_complete_16_blocks(pkg, lib, top):
    for w, h in GEOMETRIES[:5] + ((100, 36), (271, 143)):
        cover = np.zeros((h // 16, w // 16), np.int32)
        for s in (x for x in SIZES if x <= top):
            for x, y in pkg.capi.tree_roots(w, h, top, s):
                assert x % s == 0 and y % s == 0 and x + s <= w and y + s <= h
                cover[y // 16:(y + s) // 16, x // 16:(x + s) // 16] += 1
        assert (cover == 1).all(), (w, h, top)


def test_null_context_is_an_argument_error_and_touches_nothing(pkg, lib):
    cfg = pkg.capi.MltTreeConfig()
    cfg.struct_size = C.sizeof(pkg.capi.MltTreeConfig)
    nodes = np.zeros(8, pkg.capi.TREE_NODE_DTYPE)
    nodes["size"] = -7
    lm = np.full((4, 4), 0x5A, np.uint8)
    n = C.c_int(-7)
    assert lib.mlt_predict_tree(None, None, None, C.byref(cfg), nodes.ctypes.data, 8, C.byref(n), lm.ctypes.data, None, 0, None, None) == MLT_ERR_ARG
    assert n.value == -7 and (nodes["size"] == -7).all() and (lm == 0x5A).all()


# ---- decisions.build_tree on scripted deciders ----

def _decider(rule):
    """rule(size, x, y) -> (split_mode, cand_mask); confidence = a number that names the node."""
    def decide(size, xy):
        sm = np.array([rule(size, int(x), int(y))[0] for x, y in xy], np.int32)
        cm = np.array([rule(size, int(x), int(y))[1] for x, y in xy], np.uint32)
        conf = (xy[:, 0] + 1000.0 * xy[:, 1] + size / 1024.0).astype(np.float32)
        return sm, conf, cm
    return decide


def check_tree(nodes, leaf_map, w, h, top, mn, descends):
    """Everything the contract says about a node array, whatever the decider: level order, roots first in raster order, children by parent in z-order, links, tiling, map."""
    levels = [s for s in SIZES if mn <= s <= top]
    assert nodes.dtype.itemsize == 32
    assert (np.diff(nodes["depth"]) >= 0).all() and all(levels[d] == s for d, s in zip(nodes["depth"], nodes["size"]))
    cover = np.zeros((h // 16, w // 16), np.int32)
    want_map = np.full((h // 16, w // 16), 0xFF, np.uint8)
    start = 0
    for d, s in enumerate(levels):
        lvl = np.flatnonzero(nodes["depth"] == d)
        assert len(lvl) == 0 or (lvl[0] == start and lvl[-1] == start + len(lvl) - 1)
        roots = numpy_roots(w, h, top, s)
        r = nodes[start:start + len(roots)]
        assert np.array_equal(np.stack([r["x"], r["y"]], 1), roots) and (r["parent"] == -1).all() and (r["flags"] == (0 if s == top else 1)).all()
        kids = nodes[start + len(roots):start + len(lvl)]
        assert len(kids) % 4 == 0 and (kids["flags"] == 0).all()
        if len(kids):
            par = kids["parent"][::4]
            assert (np.diff(par) > 0).all() and (np.repeat(par, 4) == kids["parent"]).all()                 # parents' order, four each
            assert (nodes["depth"][par] == d - 1).all()
            assert np.array_equal(nodes["first_child"][par], start + len(roots) + 4 * np.arange(len(par)))
            for j in range(4):
                assert np.array_equal(kids["x"][j::4], nodes["x"][par] + (j & 1) * s) and np.array_equal(kids["y"][j::4], nodes["y"][par] + (j >> 1) * s)
            # exactly the descending nodes of the level above have children
            above = np.flatnonzero(nodes["depth"] == d - 1)
            assert np.array_equal(above[[descends(nodes[i]) for i in above]], par)
        elif d > 0:
            above = np.flatnonzero(nodes["depth"] == d - 1)
            assert not any(descends(nodes[i]) for i in above)
        start += len(lvl)
    assert start == len(nodes)
    assert (nodes["first_child"][nodes["size"] == mn] == -1).all()
    for nd in nodes[nodes["first_child"] < 0]:
        b = nd["size"] // 16
        cover[nd["y"] // 16:nd["y"] // 16 + b, nd["x"] // 16:nd["x"] // 16 + b] += 1
        want_map[nd["y"] // 16:nd["y"] // 16 + b, nd["x"] // 16:nd["x"] // 16 + b] = {16: 0, 32: 1, 64: 2, 128: 3}[int(nd["size"])] | ((int(nd["split_mode"]) + 1) << 4)
    covered = np.zeros_like(cover)
    for s in levels:
        for x, y in numpy_roots(w, h, top, s):
            covered[y // 16:(y + s) // 16, x // 16:(x + s) // 16] = 1
    assert np.array_equal(cover, covered)            # the leaves tile exactly what the roots cover
    assert leaf_map.dtype == np.uint8 and np.array_equal(leaf_map, want_map)
    assert ((leaf_map == 0xFF) == (covered == 0)).all()


def test_build_tree_never_and_always(pkg):
    w, h = 424, 280
    never = _decider(lambda s, x, y: (0, 1))
    nodes, lm = pkg.decisions.build_tree(w, h, 128, 16, None, never)
    check_tree(nodes, lm, w, h, 128, 16, lambda nd: False)
    assert len(nodes) == 6 + 0 + 8 + 26 and (nodes["parent"] == -1).all() and (nodes["first_child"] == -1).all()
    assert sorted(np.unique(lm).tolist()) == [0 | 1 << 4, 1 | 1 << 4, 3 | 1 << 4]
    assert nodes["confidence"][7] == np.float32(384 + 1000.0 * 32 + 32 / 1024.0)   # the decider's values reach the node they were given for
    always = _decider(lambda s, x, y: (1, 2))
    nodes, lm = pkg.decisions.build_tree(w, h, 128, 16, None, always)
    check_tree(nodes, lm, w, h, 128, 16, lambda nd: nd["size"] > 16)
    assert len(nodes) == pkg.decisions.tree_max_nodes(w, h) == 576 and (lm == (0 | 2 << 4)).all()
    assert [int((nodes["depth"] == d).sum()) for d in range(4)] == [6, 24, 104, 442]
    # the first CTU's subtree: children in z-order
    assert nodes["first_child"][0] == 6 and [(int(n["x"]), int(n["y"])) for n in nodes[6:10]] == [(0, 0), (64, 0), (0, 64), (64, 64)]
    # other classes and masks: class 2 descends only where the mask names it
    two = _decider(lambda s, x, y: (2, 4))
    assert len(pkg.decisions.build_tree(w, h, 128, 16, None, two)[0]) == 40
    nodes, lm = pkg.decisions.build_tree(w, h, 128, 16, {128: 0b100, 64: 0b110}, two)
    check_tree(nodes, lm, w, h, 128, 16, lambda nd: nd["size"] >= 64)
    assert [int((nodes["depth"] == d).sum()) for d in range(4)] == [6, 24, 104, 26]


@pytest.mark.parametrize("geometry", [(424, 280), (129, 257), (832, 480)])
def test_build_tree_checkerboard(pkg, geometry):
    w, h = geometry
    rule = lambda s, x, y: (1, 2) if ((x // s) + (y // s)) % 2 == 0 else (0, 1)
    nodes, lm = pkg.decisions.build_tree(w, h, 128, 16, None, _decider(rule))
    check_tree(nodes, lm, w, h, 128, 16, lambda nd: nd["size"] > 16 and ((nd["x"] // nd["size"]) + (nd["y"] // nd["size"])) % 2 == 0)
    assert (nodes["first_child"] >= 0).any() and ((nodes["first_child"] < 0) & (nodes["size"] > 16)).any()
    # a top below 128 and a min above 16
    nodes, lm = pkg.decisions.build_tree(w, h, 64, 32, None, _decider(rule))
    check_tree(nodes, lm, w, h, 64, 32, lambda nd: nd["size"] == 64 and ((nd["x"] // 64) + (nd["y"] // 64)) % 2 == 0)


def test_build_tree_gated_nodes_in_both_rule_modes(pkg):
    """A node the gate withholds (split -1) that keeps every class: a leaf under the default rule, descends with by_candidates."""
    w, h = 424, 280
    gated = lambda s, x, y: (x // s) % 2 == 1
    rule = lambda s, x, y: (-1, 0b11) if gated(s, x, y) else (1, 2)
    nodes, lm = pkg.decisions.build_tree(w, h, 128, 16, None, _decider(rule))
    check_tree(nodes, lm, w, h, 128, 16, lambda nd: nd["size"] > 16 and not gated(nd["size"], nd["x"], nd["y"]))
    leaves = nodes[nodes["first_child"] < 0]
    assert ((leaves["split_mode"] == -1) & (leaves["size"] > 16)).any()
    assert (lm[0, 8:16] == (3 | 0 << 4)).all()       # the CTU at x = 128 is withheld: one 128 leaf, (split + 1) = 0
    by_nodes, by_lm = pkg.decisions.build_tree(w, h, 128, 16, None, _decider(rule), by_candidates=True)
    check_tree(by_nodes, by_lm, w, h, 128, 16, lambda nd: nd["size"] > 16)
    assert len(by_nodes) == 576 and len(nodes) < 576
    # ... and a sure "no split" keeps one class that the mask does not name: a leaf in both modes
    rule2 = lambda s, x, y: (0, 1)
    assert len(pkg.decisions.build_tree(w, h, 128, 16, None, _decider(rule2), by_candidates=True)[0]) == 40


def test_min_size_64_leaves_blocks_uncovered(pkg):
    w, h = 424, 280
    nodes, lm = pkg.decisions.build_tree(w, h, 128, 64, None, _decider(lambda s, x, y: (1, 2)))
    check_tree(nodes, lm, w, h, 128, 64, lambda nd: nd["size"] == 128)
    assert len(nodes) == 6 + 24 and lm.shape == (17, 26)
    assert (lm[:16, :24] == (2 | 2 << 4)).all() and (lm[16, :] == 0xFF).all() and (lm[:, 24:] == 0xFF).all()
    assert int((lm == 0xFF).sum()) == 17 * 26 - 16 * 24


def test_picture_map_tree_arguments(tool, capsys):
    base = ["org.npy", "pred.npy", "--synthetic", "10", "--out", "o"]
    a = tool.parse_args(base + ["--tree"])
    assert a.tree and a.min_size == 16 and a.size_list == (128, 64, 32, 16)
    a = tool.parse_args(base + ["--tree", "--min-size", "32", "--sizes", "16"])
    assert a.min_size == 32 and a.size_list == (128, 64, 32)        # the levels of the descent, whatever --sizes says
    a = tool.parse_args(base + ["--sizes", "64,32"])
    assert not a.tree and a.size_list == (64, 32)
    for bad in (["--tree", "--min-size", "24"], ["--min-size", "32"], ["--tree", "--min-size", "256"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    capsys.readouterr()
    assert tool.tree_sizes(64) == (128, 64)
    with pytest.raises(ValueError):
        tool.tree_sizes(8)
    nodes = np.zeros(7, np.dtype([("size", "<i2"), ("first_child", "<i4")]))
    nodes["size"] = [128, 128, 64, 64, 64, 64, 16]
    nodes["first_child"] = [2, -1, -1, -1, -1, -1, -1]
    assert tool.tree_summary(nodes) == [(128, 2, 1), (64, 4, 0), (16, 1, 0)]
