"""CPU: the host runtime's buffer layouts (fastintercu-vvc_amd/csrc/mlt_layout.h) -- tests/layouts_check.cpp, a stand-alone program that includes only that
header and include/mltcnn.h, built with the address and undefined-behaviour sanitizers and run as a child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layouts_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "this test needs g++"
    src = os.path.join(ROOT, "tests", "layouts_check.cpp")
    includes = [l.split('"')[1] for l in open(src) if l.startswith("#include \"")]
    assert includes == ["../fastintercu-vvc_amd/csrc/mlt_layout.h", "../include/mltcnn.h"], includes
    header = open(os.path.join(ROOT, "fastintercu-vvc_amd", "csrc", "mlt_layout.h")).read()
    assert "hip/" not in header and [l for l in header.splitlines() if l.startswith("#include \"")] == ['#include "../../include/mltcnn.h"']
    exe = str(tmp_path / "layouts_check")
    # (the sanitizers' runtimes are linked into the program: nothing is preloaded, and nothing the environment preloads comes before them)
    c = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g", "-O1",
                        src, "-o", exe], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 6 capacities x 2 logit counts x (16 staging sets + 4 result sets + 1 guard slot + 1 deferred output set + 4 deferred input sets) + 8 single-CU blocks + 10 arenas
    assert r.stdout.split() == ["OK", "330", "layouts"], r.stdout
