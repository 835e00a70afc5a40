"""CPU: partition trees of several pictures under several QPs each (mlt_predict_trees_sweep) -- the new export and its signature, the error paths that need no
context, the host restatement of the union descent over several entries (decisions.build_trees_sweep) against one decisions.build_tree run per (entry, point)
with scripted deciders, the grown union arena's layout under the sanitizers (tests/trees_sweep_layout_check.cpp, a stand-alone program run as a child process) and
the --gop-qps / --qp-offsets handling of tools/picture_map.py.  No device call here."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MLT_ERR_ARG = 1


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


def test_the_new_name_is_exported_and_declared(pkg, lib):
    header = open(os.path.join(ROOT, "include", "mltcnn.h")).read()
    declared = set(re.findall(r"\b(mlt_[a-z_0-9]+)\s*\(", header))
    assert "mlt_predict_trees_sweep" in declared, "mlt_predict_trees_sweep is not declared in mltcnn.h"
    assert "mlt_predict_trees_sweep" in pkg.capi.EXPORTS
    vp, i32 = C.c_void_p, C.c_int
    assert hasattr(lib, "mlt_predict_trees_sweep")
    assert lib.mlt_predict_trees_sweep.argtypes == [vp, i32, C.POINTER(pkg.capi.MltTreePicture), C.POINTER(pkg.capi.MltTreeConfig), vp, i32, vp, i32, vp, vp, vp, vp, i32,
                                                    vp, vp]
    assert "#define MLT_SWEEP_MAX_QPS 32" in header and "#define MLT_TREES_MAX_PICTURES 256" in header
    assert "#define MLT_ABI_VERSION 4" in header and lib.mlt_abi_version() == 4
    assert C.sizeof(pkg.capi.MltTreePicture) == 24 and C.sizeof(pkg.capi.MltTreeConfig) == 40   # no struct changes
    assert hasattr(pkg.capi.MltCnn, "predict_trees_sweep") and callable(pkg.decisions.build_trees_sweep)
    for doc in ("INTEGRATION.md", os.path.join("include", "mltcnn.h")):
        assert "Not there: several pictures times several QPs" not in open(os.path.join(ROOT, doc)).read().replace("**", ""), doc


def test_null_context_is_an_argument_error_and_touches_nothing(pkg, lib):
    """Without a context nothing else is looked at: whatever the counts and the points are (good, n_qps 0 / 33, n_pictures 257, a QP sum beyond int32), the answer
    is MLT_ERR_ARG and every output keeps its sentinel.  (The same cases WITH a context are in tests/test_trees_sweep_gpu.py: they need one.)"""
    cfg = pkg.capi.MltTreeConfig()
    cfg.struct_size = C.sizeof(pkg.capi.MltTreeConfig)
    entries = (pkg.capi.MltTreePicture * 257)()
    entries[0].qp = 1
    for n_pictures, n_qps, qp0 in ((2, 2, 22), (2, 0, 22), (2, 33, 22), (257, 2, 22), (2, 2, 2 ** 31 - 1)):
        qps = np.resize(np.array([qp0, 37], np.int32), 40)
        nodes = np.zeros(8, pkg.capi.TREE_NODE_DTYPE)
        nodes["size"] = -7
        first = np.full(5, -7, np.int32)
        union = np.full((2, 4), -7, np.int32)
        lm = np.full((4, 4, 4), 0x5A, np.uint8)
        lg = np.full((8, 15), -7.0, np.float32)
        dec = np.zeros(8, pkg.capi.DECISION_DTYPE)
        cand = np.zeros(8, pkg.capi.CANDIDATES_DTYPE)
        dec["raw_mode"] = -7
        cand["count"] = -7
        rc = lib.mlt_predict_trees_sweep(None, n_pictures, entries, C.byref(cfg), qps.ctypes.data, n_qps, nodes.ctypes.data, 8, first.ctypes.data, union.ctypes.data,
                                         lm.ctypes.data, lg.ctypes.data, 15, dec.ctypes.data, cand.ctypes.data)
        assert rc == MLT_ERR_ARG, (n_pictures, n_qps, qp0)
        assert (first == -7).all() and (union == -7).all() and (nodes["size"] == -7).all() and (lm == 0x5A).all() and (lg == -7.0).all()
        assert (dec["raw_mode"] == -7).all() and (cand["count"] == -7).all()


# ---- decisions.build_trees_sweep against one build_tree run per (entry, point) ----

def _scripted(rule, n_pictures, n_points):
    """rule(p, q, size, x, y) -> (split_mode, cand_mask) for one node of entry p under point q -> (the call's decider, one build_tree decider per (entry, point),
    the list of the decider's calls).  The confidence is a function of (p, q, size, x, y) too, so a record that lands in the wrong slab, at the wrong node or in
    the wrong entry shows."""
    def one(p, q, size, xy):
        sm = np.array([rule(p, q, size, int(x), int(y))[0] for x, y in xy], np.int32)
        cm = np.array([rule(p, q, size, int(x), int(y))[1] for x, y in xy], np.uint32)
        conf = ((xy[:, 0] * 3 + xy[:, 1] * 7 + size + 1000 * q + 77 * p) % 1013 / 1013.0).astype(np.float32)
        return sm, conf, cm
    calls = []

    def sweep(size, pic, xy):
        pic = np.asarray(pic)
        assert pic.shape == (len(xy),) and (np.diff(pic) >= 0).all(), "a level is entry 0's segment, entry 1's, ..."
        calls.append((size, [int((pic == p).sum()) for p in range(n_pictures)], [(int(p), int(x), int(y)) for p, (x, y) in zip(pic, xy)]))
        out = [np.zeros((n_points, len(xy)), np.int32), np.zeros((n_points, len(xy)), np.float32), np.zeros((n_points, len(xy)), np.uint32)]
        for p in range(n_pictures):
            at = np.flatnonzero(pic == p)
            for q in range(n_points):
                for k, v in enumerate(one(p, q, size, xy[at])):
                    out[k][q, at] = v
        return tuple(out)
    singles = [[(lambda size, xy, p=p, q=q: one(p, q, size, xy)) for q in range(n_points)] for p in range(n_pictures)]
    return sweep, singles, calls


def _check(pkg, w, h, top, mn, rule, n_pictures, n_points, mask=None, by_candidates=False):
    sweep, singles, calls = _scripted(rule, n_pictures, n_points)
    res = pkg.decisions.build_trees_sweep(w, h, top, mn, mask, sweep, n_pictures, n_points, by_candidates=by_candidates)
    assert len(res) == n_pictures
    levels = [s for s in (128, 64, 32, 16) if mn <= s <= top]
    for p, (trees, counts) in enumerate(res):
        assert len(trees) == n_points and counts.shape == (4,)
        for q, (nodes, leaf_map) in enumerate(trees):
            w_nodes, w_map = pkg.decisions.build_tree(w, h, top, mn, mask, singles[p][q], by_candidates=by_candidates)
            assert nodes.dtype == w_nodes.dtype and len(nodes) == len(w_nodes), (p, q, len(nodes), len(w_nodes))
            for f in nodes.dtype.names:
                assert np.array_equal(nodes[f], w_nodes[f]), (p, q, f, np.flatnonzero(nodes[f] != w_nodes[f])[:8])
            assert nodes.tobytes() == w_nodes.tobytes() and np.array_equal(leaf_map, w_map), (p, q)
        for l, s in enumerate(levels):   # an entry's union of a level: the distinct positions of that size over its slices
            distinct = {(int(x), int(y)) for nodes, _ in trees for x, y in zip(nodes["x"][nodes["size"] == s], nodes["y"][nodes["size"] == s])}
            assert counts[l] == len(distinct), (p, s, counts[l], len(distinct))
        assert (counts[len(levels):] == 0).all()
    # the decider: once per level that has a node, with exactly the unions' nodes -- per entry the count above, every (entry, position) once
    want_calls = [(s, [int(res[p][1][l]) for p in range(n_pictures)]) for l, s in enumerate(levels) if sum(int(res[p][1][l]) for p in range(n_pictures))]
    assert [(s, per) for s, per, _ in calls] == want_calls, ([(s, per) for s, per, _ in calls], want_calls)
    for l, (s, per, seen) in enumerate(calls):
        assert len(set(seen)) == len(seen), (s, "a node was handed to the decider twice")
        for p in range(n_pictures):
            trees = res[p][0]
            distinct = {(p, int(x), int(y)) for nodes, _ in trees for x, y in zip(nodes["x"][nodes["size"] == s], nodes["y"][nodes["size"] == s])}
            assert {t for t in seen if t[0] == p} == distinct, (s, p)
    return res


W, H = 424, 280   # six 128 roots, no 64 roots, 8 roots at 32 (the column x = 384), 26 at 16 (the row y = 256)


def test_non_nested_descents_that_differ_per_picture(pkg):
    """Entry p, point q descends only into the 128 root number (2 p + q) % 6, all the way down: no tree holds another, inside an entry or across entries."""
    def rule(p, q, size, x, y):
        r = (2 * p + q) % 6
        inside = (x // 128, y // 128) == (r % 3, r // 3)
        return (1 if inside else 0), (2 if inside else 1)
    res = _check(pkg, W, H, 128, 16, rule, 3, 2)
    for p, (trees, counts) in enumerate(res):
        assert list(counts) == [6, 8, 8 + 32, 26 + 128], (p, list(counts))
        a, b = ({(int(n["x"]), int(n["y"]), int(n["size"])) for n in t[0]} for t in trees)
        assert a - b and b - a
    assert res[0][0][1][0].tobytes() != res[1][0][1][0].tobytes()


def test_an_entry_that_never_descends_between_two_that_descend_everywhere(pkg):
    """The middle entry's 64 segment is EMPTY (no roots at 64 in this geometry and nothing descended) between two full ones."""
    res = _check(pkg, W, H, 128, 16, lambda p, q, size, x, y: ((0, 1) if p == 1 else (1, 2)), 3, 2)
    assert [list(c) for _, c in res] == [[6, 24, 104, 442], [6, 0, 8, 26], [6, 24, 104, 442]]
    assert all(len(t[0]) == 576 for p in (0, 2) for t in res[p][0]) and all(len(t[0]) == 40 for t in res[1][0])
    # ... and the first and the last entry empty, the middle one full
    res = _check(pkg, W, H, 128, 16, lambda p, q, size, x, y: ((1, 2) if p == 1 and q == 1 else (0, 1)), 3, 2)
    assert [list(c) for _, c in res] == [[6, 0, 8, 26], [6, 24, 104, 442], [6, 0, 8, 26]]


def test_thirty_two_points_with_bit_31_alone(pkg):
    """With 32 points only the last one descends somewhere (bit 31), and only in entry 1."""
    res = _check(pkg, 208, 176, 32, 16, lambda p, q, size, x, y: ((1, 2) if q == 31 and p == 1 and x == 64 else (0, 1)), 2, 32)
    assert list(res[0][1]) == [30, 23, 0, 0] and list(res[1][1]) == [30, 23 + 20, 0, 0]
    assert len(res[1][0][31][0]) == 30 + 23 + 4 * 5 and all(len(t[0]) == 53 for t in res[1][0][:31]) and all(len(t[0]) == 53 for t in res[0][0])
    _check(pkg, W, H, 128, 16, lambda p, q, size, x, y: ((1, 2) if (x // size + y // size + (q % 2) + p) % 2 else (0, 1)), 2, 3)   # points 0 and 2 are one point


def test_by_candidates_and_a_withheld_split(pkg):
    """A gate-withheld split (-1) does not descend by split_mode, but its candidate mask may still hold the class: by_candidates descends there."""
    def rule(p, q, size, x, y):
        withheld = q == p % 2 and (x // size) % 2 == 0
        return (-1 if withheld else 1 if (y // size + q + p) % 2 else 0), (3 if withheld else 2 if (y // size + q + p) % 2 else 1)
    for by in (False, True):
        res = _check(pkg, W, H, 128, 16, rule, 2, 2, by_candidates=by)
        for p in range(2):
            n0 = res[p][0][p % 2][0]
            gated = n0[(n0["split_mode"] < 0) & (n0["size"] > 16)]
            assert len(gated) and ((gated["first_child"] >= 0) == by).all()


def test_lower_level_roots_and_a_wider_mask(pkg):
    """208 x 176 at 32 / 16 (30 roots, 23 border roots) and 424 x 280 at 64 / 32 with a two-class mask at 64: the border roots are alive under every point of
    every entry."""
    rule = lambda p, q, size, x, y: ((x // size + 2 * q + p) % 3, 1 << ((x // size + 2 * q + p) % 3))
    res = _check(pkg, 208, 176, 32, 16, rule, 3, 3)
    for trees, _ in res:
        for nodes, _ in trees:
            assert int((nodes["flags"] == 1).sum()) == 23
    _check(pkg, W, H, 64, 32, rule, 2, 4, mask={64: 0b101})
    _check(pkg, W, H, 16, 16, rule, 2, 2)   # one level: nothing descends, every tree is the grid


def test_one_picture_is_build_tree_sweep_and_one_point_is_build_tree(pkg):
    rule = lambda p, q, size, x, y: ((1, 2) if (x // size + y // size + q + 3 * p) % 3 else (0, 1))
    # P = 1: build_tree_sweep with the same decider
    sweep, _, _ = _scripted(rule, 1, 3)
    (trees, counts), = pkg.decisions.build_trees_sweep(W, H, 128, 16, None, sweep, 1, 3)
    w_trees, w_counts = pkg.decisions.build_tree_sweep(W, H, 128, 16, None, lambda size, xy: sweep(size, np.zeros(len(xy), np.int32), xy), 3)
    assert np.array_equal(counts, w_counts) and len(trees) == len(w_trees) == 3
    for (n, m), (wn, wm) in zip(trees, w_trees):
        assert n.tobytes() == wn.tobytes() and np.array_equal(m, wm)
    # Q = 1: per entry, build_tree (inside _check), and the union is the tree
    res = _check(pkg, W, H, 128, 16, rule, 3, 1)
    for trees, counts in res:
        assert int(counts.sum()) == len(trees[0][0])


def test_union_arena_layout_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "this test needs g++"
    src = os.path.join(ROOT, "tests", "trees_sweep_layout_check.cpp")
    includes = [l.split('"')[1] for l in open(src) if l.startswith("#include \"")]
    assert includes == ["../fastintercu-vvc_amd/csrc/mlt_layout.h", "../include/mltcnn.h"], includes
    exe = str(tmp_path / "trees_sweep_layout_check")
    # (the sanitizers' runtimes are linked into the program: nothing is preloaded)
    c = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g", "-O1",
                        src, "-o", exe], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 3 entry counts (1, 2, 5) x 3 point counts (1, 2, 32) x 3 geometries x 36 combinations of the optional parts
    assert r.stdout.split() == ["OK", "972", "arenas"], r.stdout


def test_picture_map_gop_qps_arguments(tool, capsys):
    base = ["org.npy", "pred.npy", "--synthetic", "10", "--out", "o"]
    a = tool.parse_args(base + ["--tree", "--frames", "3", "--gop-qps", "22,27,32,37"])
    assert a.tree and a.frames == 3 and a.gop_qp_list == (22, 27, 32, 37) and a.qp_offset_list == (0, 0, 0) and a.tree_qp_list is None
    assert a.size_list == (128, 64, 32, 16)
    a = tool.parse_args(base + ["--tree", "--frames", "3", "--gop-qps=-4,22,22", "--qp-offsets=0,-3,4", "--min-size", "32"])
    assert a.gop_qp_list == (-4, 22, 22) and a.qp_offset_list == (0, -3, 4) and a.size_list == (128, 64, 32)
    plain = tool.parse_args(base + ["--tree", "--frames", "3"])
    assert plain.gop_qp_list is None and plain.qp_offset_list is None
    many = ",".join(str(q) for q in range(33))
    for bad in (["--gop-qps", "22,27"],                                                        # without --tree
                ["--tree", "--gop-qps", "22,27"],                                              # without --frames
                ["--frames", "2", "--gop-qps", "22,27"],
                ["--tree", "--frames", "2", "--gop-qps", ""],
                ["--tree", "--frames", "2", "--gop-qps", many],
                ["--tree", "--frames", "2", "--gop-qps", "22,x"],
                ["--tree", "--frames", "2", "--gop-qps", "22", "--qp-offsets", "1"],            # one offset per frame
                ["--tree", "--frames", "2", "--gop-qps", "22", "--qp-offsets", "1,2,3"],
                ["--tree", "--frames", "2", "--gop-qps", "22", "--qp-offsets", "1,y"],
                ["--tree", "--frames", "2", "--gop-qps", "2147483647", "--qp-offsets", "0,1"],  # the sum leaves int32
                ["--tree", "--frames", "2", "--qp-offsets", "1,2"],                             # offsets without --gop-qps
                ["--tree", "--qp-offsets", "1"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    assert len(tool.parse_args(base + ["--tree", "--frames", "2", "--gop-qps", many[:-3]]).gop_qp_list) == 32
    capsys.readouterr()
    with pytest.raises(SystemExit):   # --tree --frames N --tree-qps stays refused
        tool.parse_args(base + ["--tree", "--frames", "2", "--tree-qps", "22,27"])
    assert "--tree-qps goes with --tree and not with --frames" in capsys.readouterr().err
