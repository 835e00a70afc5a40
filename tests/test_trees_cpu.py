"""CPU: partition trees of several pictures in one call (mlt_predict_trees) -- the new export and its structure, the NULL-context error path, the device arena's
layout under the sanitizers (tests/trees_layout_check.cpp, a stand-alone program run as a child process) and the --frames handling of tools/picture_map.py.
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
    assert "mlt_predict_trees" in declared, "mlt_predict_trees is not declared in mltcnn.h"
    assert "mlt_predict_trees" in pkg.capi.EXPORTS
    assert hasattr(lib, "mlt_predict_trees") and lib.mlt_predict_trees.argtypes is not None and len(lib.mlt_predict_trees.argtypes) == 12
    assert "#define MLT_TREES_MAX_PICTURES 256" in header and "} mlt_tree_picture;" in header
    assert pkg.capi.TREES_MAX_PICTURES == 256
    assert C.sizeof(pkg.capi.MltTreePicture) == 24
    assert [getattr(pkg.capi.MltTreePicture, f).offset for f in ("org", "pred", "poc", "qp")] == [0, 8, 16, 20]
    assert lib.mlt_abi_version() == 4
    assert hasattr(pkg.capi.MltCnn, "predict_trees")


def test_null_context_is_an_argument_error_and_touches_nothing(pkg, lib):
    cfg = pkg.capi.MltTreeConfig()
    cfg.struct_size = C.sizeof(pkg.capi.MltTreeConfig)
    pics = (pkg.capi.MltTreePicture * 2)()
    nodes = np.zeros(8, pkg.capi.TREE_NODE_DTYPE)
    nodes["size"] = -7
    first = np.full(3, -7, np.int32)
    lm = np.full((2, 4, 4), 0x5A, np.uint8)
    lg = np.full((8, 15), -7.0, np.float32)
    dec = np.zeros(8, pkg.capi.DECISION_DTYPE)
    cand = np.zeros(8, pkg.capi.CANDIDATES_DTYPE)
    dec["raw_mode"] = -7
    cand["count"] = -7
    rc = lib.mlt_predict_trees(None, 2, pics, C.byref(cfg), nodes.ctypes.data, 8, first.ctypes.data, lm.ctypes.data, lg.ctypes.data, 15, dec.ctypes.data, cand.ctypes.data)
    assert rc == MLT_ERR_ARG
    assert (first == -7).all() and (nodes["size"] == -7).all() and (lm == 0x5A).all() and (lg == -7.0).all() and (dec["raw_mode"] == -7).all() and (cand["count"] == -7).all()


def test_trees_arena_layout_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "this test needs g++"
    src = os.path.join(ROOT, "tests", "trees_layout_check.cpp")
    includes = [l.split('"')[1] for l in open(src) if l.startswith("#include \"")]
    assert includes == ["../fastintercu-vvc_amd/csrc/mlt_layout.h", "../include/mltcnn.h"], includes
    exe = str(tmp_path / "trees_layout_check")
    # (the sanitizers' runtimes are linked into the program: nothing is preloaded)
    c = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g", "-O1",
                        src, "-o", exe], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 3 picture counts (1, 2, 256) x 3 geometries x (candidate records in the arena or not) x 8 combinations of requested outputs
    assert r.stdout.split() == ["OK", "144", "arenas"], r.stdout


def test_picture_map_frames_arguments(tool, tmp_path, capsys):
    base = ["org.npy", "pred.npy", "--synthetic", "10", "--out", "o"]
    a = tool.parse_args(base + ["--tree", "--frames", "8", "--poc", "16"])
    assert a.tree and a.frames == 8 and a.poc == 16 and a.size_list == (128, 64, 32, 16)
    assert tool.parse_args(base + ["--tree"]).frames is None
    for bad in (["--frames", "4"], ["--tree", "--frames", "0"], ["--tree", "--frames", "257"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    capsys.readouterr()
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 1024, size=(3, 32, 48)).astype(np.int16)
    npy, raw = str(tmp_path / "f.npy"), str(tmp_path / "f.yuv")
    np.save(npy, frames)
    frames.astype("<u2").tofile(raw)
    assert np.array_equal(tool.read_frames(npy, 3), frames) and np.array_equal(tool.read_frames(npy, 3, 48, 32), frames)
    assert np.array_equal(tool.read_frames(raw, 3, 48, 32), frames)
    assert np.array_equal(tool.read_frames(raw, 2, 48, 32), frames[:2])        # the first planes of a longer file
    one = str(tmp_path / "one.npy")
    np.save(one, frames[0])
    assert np.array_equal(tool.read_frames(one, 1), frames[:1])                # a 2-D array is one frame
    for args in ((npy, 2), (npy, 3, 64, 32), (raw, 4, 48, 32), (raw, 3), (npy, 0)):
        with pytest.raises(ValueError):
            tool.read_frames(*args)
