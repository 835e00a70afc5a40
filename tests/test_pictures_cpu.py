"""CPU: device-resident pictures -- the new exports, mlt_grid_positions against numpy, the NULL-context error paths, and the host logic of
tools/picture_map.py (file reading, grid).  No device call here."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mlt_picture_create", "mlt_picture_upload", "mlt_picture_wrap_device", "mlt_picture_destroy", "mlt_predict_at", "mlt_grid_positions")
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


def _numpy_grid(w, h, s):
    return np.array([(x, y) for y in range(0, h - s + 1, s) for x in range(0, w - s + 1, s)], np.int32).reshape(-1, 2)


def test_new_names_are_exported_and_declared(pkg, lib):
    header = open(os.path.join(ROOT, "include", "mltcnn.h")).read()
    declared = set(re.findall(r"\b(mlt_[a-z_0-9]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in mltcnn.h"
        assert name in pkg.capi.EXPORTS, f"{name} is missing from capi.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert getattr(lib, name).argtypes is not None, f"{name} has no argtypes"
    assert "typedef struct mlt_picture mlt_picture;" in header
    assert lib.mlt_abi_version() == 4
    assert callable(pkg.capi.grid_positions) and hasattr(pkg.capi.MltCnn, "picture") and hasattr(pkg.capi.MltCnn, "wrap_picture") and hasattr(pkg.capi.MltCnn, "predict_at")


def test_grid_positions_against_numpy(pkg, lib):
    counts = {s: len(pkg.capi.grid_positions(1920, 1080, s)) for s in (128, 64, 32, 16)}
    assert counts == {128: 120, 64: 480, 32: 1980, 16: 8040}
    for w, h in ((1920, 1080), (832, 480), (416, 240), (16, 16), (129, 257)):
        for s in (128, 64, 32, 16):
            got = pkg.capi.grid_positions(w, h, s)
            want = _numpy_grid(w, h, s)
            assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (w, h, s)
            assert lib.mlt_grid_positions(w, h, s, None, 0) == (w // s) * (h // s)
    assert pkg.capi.grid_positions(16, 16, 16).tolist() == [[0, 0]]
    assert lib.mlt_grid_positions(15, 200, 16, None, 0) == 0 and len(pkg.capi.grid_positions(15, 200, 16)) == 0
    assert lib.mlt_grid_positions(200, 15, 16, None, 0) == 0
    for s in (8, 0, -16, 24, 256):
        assert lib.mlt_grid_positions(1920, 1080, s, None, 0) == 0, s
    # a cap below the count: only `cap` entries are written, the count is still returned
    full = _numpy_grid(832, 480, 64)
    buf = np.full((len(full), 2), -7, np.int32)
    assert lib.mlt_grid_positions(832, 480, 64, buf.ctypes.data, 10) == len(full) == 13 * 7
    assert np.array_equal(buf[:10], full[:10]) and (buf[10:] == -7).all()
    assert lib.mlt_grid_positions(832, 480, 64, buf.ctypes.data, 0) == len(full) and (buf[10:] == -7).all()


def test_null_context_is_an_argument_error_and_touches_nothing(pkg, lib):
    h = C.c_void_p(0x1234)
    assert lib.mlt_picture_create(None, 64, 64, C.byref(h)) == MLT_ERR_ARG and h.value == 0x1234
    plane = np.full((64, 64), 5, np.int16)
    assert lib.mlt_picture_upload(None, None, plane.ctypes.data, 64) == MLT_ERR_ARG and (plane == 5).all()
    assert lib.mlt_picture_wrap_device(None, C.c_void_p(0x1000), 64, 64, 64, C.byref(h)) == MLT_ERR_ARG and h.value == 0x1234
    assert lib.mlt_picture_destroy(None, None) == MLT_ERR_ARG
    n = 3
    xy = np.zeros((n, 2), np.int32)
    poc = np.zeros(n, np.int32)
    qp = np.full(n, 32, np.int32)
    split = np.full(n, -7, np.int32)
    logits = np.full((n, 9), -7.0, np.float32)
    dec = np.zeros(n, pkg.capi.DECISION_DTYPE)
    cand = np.zeros(n, pkg.capi.CANDIDATES_DTYPE)
    dec["split_mode"] = -7
    cand["count"] = -7
    assert lib.mlt_predict_at(None, 128, None, None, n, xy.ctypes.data, poc.ctypes.data, qp.ctypes.data, split.ctypes.data, logits.ctypes.data,
                              dec.ctypes.data, cand.ctypes.data) == MLT_ERR_ARG
    assert (split == -7).all() and (logits == -7.0).all() and (dec["split_mode"] == -7).all() and (cand["count"] == -7).all()


def test_picture_map_reads_raw_and_npy_and_its_grid_is_the_librarys(pkg, lib, tool, tmp_path):
    rng = np.random.default_rng(7)
    w, h = 77, 35
    frames = rng.integers(0, 1024, size=(2, h, w)).astype(np.int16)
    raw = tmp_path / "two_frames.yuv"
    frames.astype("<u2").tofile(raw)
    got = tool.read_picture(str(raw), w, h)
    assert got.dtype == np.int16 and got.shape == (h, w) and got.flags["C_CONTIGUOUS"] and np.array_equal(got, frames[0])
    with pytest.raises(ValueError):
        tool.read_picture(str(raw), w, 3 * h)              # more samples than the file holds
    with pytest.raises(ValueError):
        tool.read_picture(str(raw))                        # a raw file without geometry
    npy = tmp_path / "frame.npy"
    np.save(npy, frames[1])
    assert np.array_equal(tool.read_picture(str(npy)), frames[1]) and np.array_equal(tool.read_picture(str(npy), w, h), frames[1])
    with pytest.raises(ValueError):
        tool.read_picture(str(npy), w + 1, h)
    np.save(npy, frames[1].astype(np.int32))
    with pytest.raises(ValueError):
        tool.read_picture(str(npy))
    for pw, ph in ((1920, 1080), (832, 480), (16, 16), (15, 200)):
        for s in (128, 64, 32, 16, 8):
            g = tool.grid(pw, ph, s)
            assert g.dtype == np.int32 and np.array_equal(g, pkg.capi.grid_positions(pw, ph, s)), (pw, ph, s)
    m = tool.to_map(np.arange(15 * 8), 1920, 1080, 128)
    assert m.shape == (8, 15) and m[1, 0] == 15
    assert tool.histogram(np.array([0, 1, 1, -1, 3]), 4) == {0: 1, 1: 2, 2: 0, 3: 1, -1: 1}
