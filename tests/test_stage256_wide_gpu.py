"""GPU (MI355X): the whole 256-channel stage with both cout passes per wave (stage256_wide_kernel, the default form of the single-pass whole-stage
launch) against the form that runs one cout pass at a time (chain_kernel; MLT_TUNING=1 MLT_NO_STAGE256_WIDE=1): logits and split modes byte for byte.
The switch is read once per process, so the old form runs in ONE fresh child process that evaluates all batches.

Seed-10 weights, calibration and guards off (every logit comes from the kernels under test), one network pass per batch (the device entry point).
CU counts: 257 -- the smallest batch that takes the whole-stage launch (n * 64 output pixels > 16384), 129 tiles of two CUs the last of which is ragged;
258 -- whole tiles only; 600 -- 300 tiles on 256 workgroups, so 44 workgroups carry the weight ring, the patch rotation and their registers across a
tile boundary.  Texture content with one all-zero CU between all-1023 CUs: next to it in the batch (one of them shares its tile) and one grid stride
(256 tiles = 512 CUs) away -- whatever a persistent workgroup left in LDS or registers from the tile before would show."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, COUNTS = 128, (257, 258, 600)
TAG = "both cout passes per wave"
STAGE_256 = "stage_256_h8(s2+sc,conv2,conv1,conv2)"


def zero_cu(n):
    """an even index (first CU of its tile) whose tile has a successor one grid stride later where the batch is long enough"""
    return 44 if n >= 600 else (n // 2) & ~1


def make_inputs(pkg, n):
    org, pred = pkg.synth.make_patches_bulk(SIZE, n, 9000 + n)
    poc, qp = pkg.synth.make_scalars(n, 9000 + n)
    z = zero_cu(n)
    for i in (z - 1, z + 1, z + 512, z + 513):   # its neighbours in the batch (z + 1: in its tile) and the tile its workgroup walks next
        if 0 <= i < n:
            org[i], pred[i] = 1023, 1023
    org[z], pred[z] = 0, 0
    return org, pred, poc, qp


def plan_lines(pkg, n):
    lib = pkg.capi.load_library()
    lib.mlt_plan_describe.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_char_p, C.c_size_t]
    blob = pkg.weights.synthetic_blob(pkg.synth.arch_for_size(SIZE), 10)
    buf = C.create_string_buffer(1 << 15)
    k = lib.mlt_plan_describe(blob, len(blob), SIZE, n, 0, 0, 0, 1, buf, 1 << 15)
    assert k > 0
    return buf.value.decode().splitlines()


def run_batches(pkg):
    """{n: (split, logits)} of one device-entry pass per CU count"""
    import torch
    blob = pkg.weights.synthetic_blob(0, 10)
    F = pkg.capi
    m = pkg.MltCnn(device=0, sizes=(SIZE,), blobs={SIZE: blob}, flags=F.FLAG_NO_CALIBRATION | F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD)
    dev = torch.device("cuda", 0)
    out = {}
    for n in COUNTS:
        t_in = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in make_inputs(pkg, n)]
        d_split = torch.full((n,), -7, dtype=torch.int32, device=dev)
        d_lg = torch.zeros((n, 9), dtype=torch.float32, device=dev)
        m.predict_batch_device(n, SIZE, *[t.data_ptr() for t in t_in], d_split.data_ptr(), d_lg.data_ptr())
        m.synchronize()
        out[n] = (d_split.cpu().numpy(), d_lg.cpu().numpy())
    m.close()
    return out


CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import mltcnn_pkg
import test_stage256_wide_gpu as T
pkg = mltcnn_pkg.load()
out = T.run_batches(pkg)
np.savez({dst!r}, plan=np.array(T.plan_lines(pkg, 600)), **{{f"split{{n}}": s for n, (s, l) in out.items()}}, **{{f"logits{{n}}": l for n, (s, l) in out.items()}})
"""


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


@pytest.fixture(scope="module")
def wide_form(gpu):
    assert not os.environ.get("MLT_TUNING"), "the test process must run the default form"
    return run_batches(gpu)


@pytest.fixture(scope="module")
def old_form(gpu, tmp_path_factory):
    dst = str(tmp_path_factory.mktemp("wide") / "old_form.npz")
    script = tmp_path_factory.mktemp("wide_child") / "old_form.py"
    script.write_text(CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), dst=dst))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, MLT_TUNING="1", MLT_NO_STAGE256_WIDE="1"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return np.load(dst)


def test_the_default_form_is_the_wide_one_and_the_switch_selects_the_old_one(gpu, wide_form, old_form):
    """both forms run under the same launch name; the plan record of this process carries the tag, the child's (with the switch) does not"""
    here = [l for l in plan_lines(gpu, 600) if l.startswith(STAGE_256)]
    there = [l for l in old_form["plan"].tolist() if l.startswith(STAGE_256)]
    assert len(here) == 1 and TAG in here[0], here
    assert len(there) == 1 and TAG not in there[0], there


@pytest.mark.parametrize("n", COUNTS)
def test_logits_and_split_modes_are_the_old_forms_bytes(wide_form, old_form, n):
    split, logits = wide_form[n]
    assert np.isfinite(logits).all() and (split >= 0).all()
    z = zero_cu(n)
    assert len({logits[i].tobytes() for i in (z - 1, z, z - 2)}) == 3      # the zero CU, its all-1023 neighbour and a texture CU differ: content reaches the logits
    diff = np.flatnonzero((logits.view(np.uint32) != old_form[f"logits{n}"].view(np.uint32)).any(axis=1))
    print(f"n = {n}: {len(diff)} CUs with different logit bytes, max |d| = {np.abs(logits - old_form[f'logits{n}']).max():.3e}")
    assert len(diff) == 0, diff[:16]
    assert split.tobytes() == old_form[f"split{n}"].tobytes()
