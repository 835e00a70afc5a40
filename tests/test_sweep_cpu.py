"""CPU: QP sweeps (include/mltcnn.h: mlt_predict_batch_device_sweep, mlt_predict_at_sweep) -- what needs no device: the two new buffer layouts of
fastintercu-vvc_amd/csrc/mlt_layout.h walked by tests/sweep_layouts_check.cpp (a stand-alone program under the address and undefined-behaviour sanitizers, run
as a child process), the exports and their ctypes signatures, the NULL-context answers, and tools/picture_map.py refusing --qps with --tree."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_EXPORTS = ("mlt_predict_batch_device_sweep", "mlt_predict_at_sweep")


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build.build_lib()
    return pkg.capi.load_library()


def test_sweep_layouts_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "this test needs g++"
    src = os.path.join(ROOT, "tests", "sweep_layouts_check.cpp")
    includes = [l.split('"')[1] for l in open(src) if l.startswith("#include \"")]
    assert includes == ["../fastintercu-vvc_amd/csrc/mlt_layout.h", "../include/mltcnn.h"], includes
    exe = str(tmp_path / "sweep_layouts_check")
    # (the sanitizers' runtimes are linked into the program: nothing is preloaded)
    c = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g", "-O1",
                        src, "-o", exe], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 3 capacities x (3 point counts x 2 logit counts x 4 CU sizes x 4 record switches staging sets + 1 guard slot)
    assert r.stdout.split() == ["OK", str(3 * (3 * 2 * 4 * 4 + 1)), "layouts"], r.stdout


def test_exports_and_signatures(pkg, lib):
    assert pkg.capi.SWEEP_MAX_QPS == 32
    header = open(os.path.join(ROOT, "include", "mltcnn.h")).read()
    assert "#define MLT_SWEEP_MAX_QPS 32" in header and "#define MLT_ABI_VERSION 4" in header
    vp, i32 = C.c_void_p, C.c_int
    want = {"mlt_predict_batch_device_sweep": [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp],
            "mlt_predict_at_sweep": [vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]}
    for name in SWEEP_EXPORTS:
        assert name in pkg.capi.EXPORTS and name in header, name
        assert getattr(lib, name).argtypes == want[name], name
    assert lib.mlt_abi_version() == 4
    assert callable(pkg.MltCnn.predict_at_sweep) and callable(pkg.MltCnn.predict_batch_device_sweep)


def test_null_context_is_an_argument_error(lib):
    qps = np.array([22, 27], np.int32)
    out = np.full(8, -7, np.int32)
    assert lib.mlt_predict_batch_device_sweep(None, 1, 128, None, None, None, qps.ctypes.data, 2, out.ctypes.data, None, None, None) == 1      # MLT_ERR_ARG
    assert lib.mlt_predict_at_sweep(None, 128, None, None, 1, None, None, qps.ctypes.data, 2, out.ctypes.data, None, None, None) == 1
    assert (out == -7).all()


def test_picture_map_refuses_qps_with_tree(tmp_path):
    a = str(tmp_path / "a.npy")
    np.save(a, np.zeros((128, 128), np.int16))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "picture_map.py"), a, a, "--synthetic", "10", "--qps", "22,27", "--tree", "--out", str(tmp_path / "o")],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--qps does not go with --tree" in r.stderr, (r.returncode, r.stderr[-600:])
    assert os.listdir(tmp_path) == ["a.npy"]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import picture_map
    finally:
        sys.path.pop(0)
    args = picture_map.parse_args([a, a, "--synthetic", "10", "--qps", "22,27,32,37", "--sizes", "128,64", "--out", "o"])
    assert args.qp_list == (22, 27, 32, 37) and args.size_list == (128, 64)
    assert picture_map.parse_args([a, a, "--synthetic", "10", "--out", "o"]).qp_list is None
    with pytest.raises(ValueError):
        picture_map.parse_qps(",".join(["30"] * 33))
