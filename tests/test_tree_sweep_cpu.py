"""CPU: partition trees of one picture under several QPs (mlt_predict_tree_sweep) -- the new export and its signature, the NULL-context error path, the host
restatement of the union descent (decisions.build_tree_sweep) against one decisions.build_tree run per point with scripted deciders, the union arena's layout
under the sanitizers (tests/tree_sweep_layout_check.cpp, a stand-alone program run as a child process) and the --tree-qps handling of tools/picture_map.py.
No device call here."""
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
    assert "mlt_predict_tree_sweep" in declared, "mlt_predict_tree_sweep is not declared in mltcnn.h"
    assert "mlt_predict_tree_sweep" in pkg.capi.EXPORTS
    vp, i32 = C.c_void_p, C.c_int
    assert hasattr(lib, "mlt_predict_tree_sweep")
    assert lib.mlt_predict_tree_sweep.argtypes == [vp, vp, vp, C.POINTER(pkg.capi.MltTreeConfig), vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp]
    assert len(lib.mlt_predict_tree_sweep.argtypes) == 15
    assert "#define MLT_SWEEP_MAX_QPS 32" in header and "#define MLT_ABI_VERSION 4" in header and lib.mlt_abi_version() == 4
    assert hasattr(pkg.capi.MltCnn, "predict_tree_sweep") and callable(pkg.decisions.build_tree_sweep)
    assert "a TREE sweep does not exist" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_context_is_an_argument_error_and_touches_nothing(pkg, lib):
    cfg = pkg.capi.MltTreeConfig()
    cfg.struct_size = C.sizeof(pkg.capi.MltTreeConfig)
    qps = np.array([22, 37], np.int32)
    nodes = np.zeros(8, pkg.capi.TREE_NODE_DTYPE)
    nodes["size"] = -7
    first = np.full(3, -7, np.int32)
    union = np.full(4, -7, np.int32)
    lm = np.full((2, 4, 4), 0x5A, np.uint8)
    lg = np.full((8, 15), -7.0, np.float32)
    dec = np.zeros(8, pkg.capi.DECISION_DTYPE)
    cand = np.zeros(8, pkg.capi.CANDIDATES_DTYPE)
    dec["raw_mode"] = -7
    cand["count"] = -7
    rc = lib.mlt_predict_tree_sweep(None, None, None, C.byref(cfg), qps.ctypes.data, 2, nodes.ctypes.data, 8, first.ctypes.data, union.ctypes.data, lm.ctypes.data,
                                    lg.ctypes.data, 15, dec.ctypes.data, cand.ctypes.data)
    assert rc == MLT_ERR_ARG
    assert (first == -7).all() and (union == -7).all() and (nodes["size"] == -7).all() and (lm == 0x5A).all() and (lg == -7.0).all()
    assert (dec["raw_mode"] == -7).all() and (cand["count"] == -7).all()


# ---- decisions.build_tree_sweep against one build_tree run per point ----

def _scripted(rule, n_points):
    """rule(q, size, x, y) -> (split_mode, cand_mask) for one node under point q -> (the sweep's decider, one build_tree decider per point).  The confidence is a
    function of (q, size, x, y) too, so a record that lands in the wrong slab or at the wrong node shows."""
    def one(q, size, xy):
        sm = np.array([rule(q, size, int(x), int(y))[0] for x, y in xy], np.int32)
        cm = np.array([rule(q, size, int(x), int(y))[1] for x, y in xy], np.uint32)
        conf = ((xy[:, 0] * 3 + xy[:, 1] * 7 + size + 1000 * q) % 1013 / 1013.0).astype(np.float32)
        return sm, conf, cm
    calls = []

    def sweep(size, xy):
        calls.append((size, len(xy)))
        per = [one(q, size, xy) for q in range(n_points)]
        return tuple(np.stack([p[k] for p in per]) for k in range(3))
    return sweep, [lambda size, xy, q=q: one(q, size, xy) for q in range(n_points)], calls


def _check(pkg, w, h, top, mn, rule, n_points, mask=None, by_candidates=False):
    sweep, singles, calls = _scripted(rule, n_points)
    trees, counts = pkg.decisions.build_tree_sweep(w, h, top, mn, mask, sweep, n_points, by_candidates=by_candidates)
    assert len(trees) == n_points and counts.shape == (4,)
    want = [pkg.decisions.build_tree(w, h, top, mn, mask, d, by_candidates=by_candidates) for d in singles]
    for q, ((nodes, leaf_map), (w_nodes, w_map)) in enumerate(zip(trees, want)):
        assert nodes.dtype == w_nodes.dtype and len(nodes) == len(w_nodes), (q, len(nodes), len(w_nodes))
        for f in nodes.dtype.names:
            assert np.array_equal(nodes[f], w_nodes[f]), (q, f, np.flatnonzero(nodes[f] != w_nodes[f])[:8])
        assert nodes.tobytes() == w_nodes.tobytes() and np.array_equal(leaf_map, w_map), q
    levels = [s for s in (128, 64, 32, 16) if mn <= s <= top]
    for l, s in enumerate(levels):   # the union of a level: the distinct positions of that size over the slices; the decider saw each of them once
        distinct = {(int(x), int(y)) for nodes, _ in trees for x, y in zip(nodes["x"][nodes["size"] == s], nodes["y"][nodes["size"] == s])}
        assert counts[l] == len(distinct), (s, counts[l], len(distinct))
    assert (counts[len(levels):] == 0).all()
    assert calls == [(s, int(counts[l])) for l, s in enumerate(levels) if counts[l]], calls
    return trees, counts


W, H = 424, 280   # six 128 roots, no 64 roots, 8 roots at 32 (the column x = 384), 26 at 16 (the row y = 256)


def test_non_nested_descents(pkg):
    """Point 0 descends only into the root at (0, 0), point 1 only into the root at (128, 0), all the way down: neither tree holds the other."""
    def rule(q, size, x, y):
        inside = (x // 128, y // 128) == ((0, 0) if q == 0 else (1, 0))
        return (1 if inside else 0), (2 if inside else 1)
    trees, counts = _check(pkg, W, H, 128, 16, rule, 2)
    assert list(counts) == [6, 8, 8 + 32, 26 + 128]
    assert [len(t[0]) for t in trees] == [6 + 4 + 8 + 16 + 26 + 64] * 2
    a, b = ({(int(n["x"]), int(n["y"]), int(n["size"])) for n in t[0]} for t in trees)
    assert a - b and b - a


def test_a_point_that_never_descends_beside_one_that_descends_everywhere(pkg):
    trees, counts = _check(pkg, W, H, 128, 16, lambda q, size, x, y: ((1, 2) if q == 1 else (0, 1)), 2)
    assert len(trees[0][0]) == 6 + 0 + 8 + 26 and len(trees[1][0]) == pkg.decisions.tree_max_nodes(W, H) == 576
    assert list(counts) == [6, 24, 104, 442]   # the union is the full tree; the roots of the lower levels are part of both


def test_duplicate_points_and_thirty_two_points(pkg):
    """Points 0 and 2 are the same point; with 32 points the last one is alone in descending somewhere (bit 31)."""
    _check(pkg, W, H, 128, 16, lambda q, size, x, y: ((1, 2) if (x // size + y // size + (q % 2)) % 2 else (0, 1)), 3)
    trees, counts = _check(pkg, 208, 176, 32, 16, lambda q, size, x, y: ((1, 2) if q == 31 and x == 64 else (0, 1)), 32)
    assert len(trees[31][0]) == 30 + 23 + 4 * 5 and all(len(t[0]) == 53 for t in trees[:31]) and list(counts) == [30, 23 + 20, 0, 0]


def test_by_candidates_and_a_withheld_split(pkg):
    """A gate-withheld split (-1) does not descend by split_mode, but its candidate mask may still hold the class: by_candidates descends there."""
    def rule(q, size, x, y):
        withheld = q == 0 and (x // size) % 2 == 0
        return (-1 if withheld else 1 if (y // size + q) % 2 else 0), (3 if withheld else 2 if (y // size + q) % 2 else 1)
    for by in (False, True):
        trees, _ = _check(pkg, W, H, 128, 16, rule, 2, by_candidates=by)
        n0 = trees[0][0]
        gated = n0[(n0["split_mode"] < 0) & (n0["size"] > 16)]
        assert len(gated) and ((gated["first_child"] >= 0) == by).all()


def test_lower_level_roots_and_a_wider_mask(pkg):
    """208 x 176 at 32 / 16 (30 roots, 23 border roots) and 424 x 280 at 64 / 32 with a two-class mask at 64: the border roots are alive under every point."""
    rule = lambda q, size, x, y: ((x // size + 2 * q) % 3, 1 << ((x // size + 2 * q) % 3))
    trees, counts = _check(pkg, 208, 176, 32, 16, rule, 3)
    for nodes, _ in trees:
        assert int((nodes["flags"] == 1).sum()) == 23
    _check(pkg, W, H, 64, 32, rule, 4, mask={64: 0b101})
    _check(pkg, W, H, 16, 16, rule, 2)   # one level: nothing descends, every tree is the grid


def test_union_arena_layout_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "this test needs g++"
    src = os.path.join(ROOT, "tests", "tree_sweep_layout_check.cpp")
    includes = [l.split('"')[1] for l in open(src) if l.startswith("#include \"")]
    assert includes == ["../fastintercu-vvc_amd/csrc/mlt_layout.h", "../include/mltcnn.h"], includes
    exe = str(tmp_path / "tree_sweep_layout_check")
    # (the sanitizers' runtimes are linked into the program: nothing is preloaded)
    c = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g", "-O1",
                        src, "-o", exe], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 3 point counts (1, 2, 32) x 3 geometries x 36 combinations: logits slabs (and, with them, the logits output) x candidate slabs (and the candidate output)
    # x leaf maps x the decision output
    assert r.stdout.split() == ["OK", "324", "arenas"], r.stdout


def test_picture_map_tree_qps_arguments(tool, capsys):
    base = ["org.npy", "pred.npy", "--synthetic", "10", "--out", "o"]
    a = tool.parse_args(base + ["--tree", "--tree-qps", "22,27,32,37"])
    assert a.tree and a.tree_qp_list == (22, 27, 32, 37) and a.qp_list is None and a.size_list == (128, 64, 32, 16)
    assert tool.parse_args(base + ["--tree", "--tree-qps=-4,22,22", "--min-size", "32"]).tree_qp_list == (-4, 22, 22)
    assert tool.parse_args(base + ["--tree"]).tree_qp_list is None
    many = ",".join(str(q) for q in range(33))
    for bad in (["--tree-qps", "22,27"], ["--tree", "--frames", "2", "--tree-qps", "22,27"], ["--tree", "--tree-qps", ""], ["--tree", "--tree-qps", many],
                ["--tree", "--tree-qps", "22,x"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    assert len(tool.parse_args(base + ["--tree", "--tree-qps", many[:-3]]).tree_qp_list) == 32
    with pytest.raises(SystemExit):   # --qps with --tree stays refused
        tool.parse_args(base + ["--tree", "--qps", "22,27"])
    assert "--qps does not go with --tree" in capsys.readouterr().err
