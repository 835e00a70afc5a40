"""GPU (MI355X): the streaming pair that hands layer1's projection shortcut over as its INPUT (layer0_stream_xs_kernel -> layer1_stream_xs_kernel, the
default for batches of 128 x 128 CUs from 128 CUs on) against the pair that hands over the shortcut itself (MLT_TUNING=1 MLT_NO_XS_HANDOFF=1): logits and
split modes byte for byte.  The switch is read once per process, so the old pair runs in ONE fresh child process that evaluates all batches.

Seed-10 weights, calibration and guards off (every logit comes from the kernels under test), one network pass per batch (the device entry point).
CU counts: 128 -- the smallest streaming batch, one CU per persistent workgroup; 129 -- one more than that; 600 -- 256 workgroups, 88 of which walk three
CUs and 168 two, so the Sc slot parity, the row numbering and the loader waves' register slots run across CU boundaries.  Texture content with one
all-zero CU between all-1023 CUs, both next to it in the batch and next to it in its workgroup's walk (256 CUs apart): whatever a persistent workgroup
left in LDS or registers from the CU before would show."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, COUNTS = 128, (128, 129, 600)


def make_inputs(pkg, n):
    org, pred = pkg.synth.make_patches_bulk(SIZE, n, 7000 + n)
    poc, qp = pkg.synth.make_scalars(n, 7000 + n)
    z = n // 2
    for i in (z - 1, z + 1, z - 256, z + 256):
        if 0 <= i < n:
            org[i], pred[i] = 1023, 1023
    org[z], pred[z] = 0, 0
    return org, pred, poc, qp


def run_batches(pkg, profile=False):
    """{n: (split, logits)} of one device-entry pass per CU count; with `profile`, also the profile entries of the last batch"""
    import torch
    blob = pkg.weights.synthetic_blob(0, 10)
    F = pkg.capi
    m = pkg.MltCnn(device=0, sizes=(SIZE,), blobs={SIZE: blob}, flags=F.FLAG_NO_CALIBRATION | F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD)
    dev = torch.device("cuda", 0)
    out, prof = {}, None
    for n in COUNTS:
        t_in = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in make_inputs(pkg, n)]
        d_split = torch.full((n,), -7, dtype=torch.int32, device=dev)
        d_lg = torch.zeros((n, 9), dtype=torch.float32, device=dev)
        if profile and n == COUNTS[-1]:
            m.profile_enable(True)
        m.predict_batch_device(n, SIZE, *[t.data_ptr() for t in t_in], d_split.data_ptr(), d_lg.data_ptr())
        m.synchronize()
        if profile and n == COUNTS[-1]:
            prof = m.profile_read()
            m.profile_enable(False)
        out[n] = (d_split.cpu().numpy(), d_lg.cpu().numpy())
    m.close()
    return out, prof


CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import mltcnn_pkg
import test_xs_handoff_gpu as T
pkg = mltcnn_pkg.load()
out, prof = T.run_batches(pkg, profile=True)
np.savez({dst!r}, front_bytes=[e["bytes"] for e in prof if e["name"].startswith("layer0_stream_h64")], **{{f"split{{n}}": s for n, (s, l) in out.items()}}, **{{f"logits{{n}}": l for n, (s, l) in out.items()}})
"""


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


@pytest.fixture(scope="module")
def new_pair(gpu):
    assert not os.environ.get("MLT_TUNING"), "the test process must run the default pair"
    return run_batches(gpu, profile=True)


@pytest.fixture(scope="module")
def old_pair(gpu, tmp_path_factory):
    dst = str(tmp_path_factory.mktemp("xs") / "old_pair.npz")
    script = tmp_path_factory.mktemp("xs_child") / "old_pair.py"
    script.write_text(CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), dst=dst))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, MLT_TUNING="1", MLT_NO_XS_HANDOFF="1"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return np.load(dst)


def front_bytes(n, handed_channels):
    """the algorithmic bytes the dispatcher books for the five-stage front launch: raw planes in, t (64 channels) and the hand-off out"""
    return n * 128 * 128 * 4 + n * 32 * 32 * (64 + handed_channels) * 2


def test_the_default_pair_is_the_xs_pair_and_the_switch_selects_the_old_one(new_pair, old_pair):
    """One profiled pass each: both pairs profile under the same two names, but the front launch is booked with the bytes of what it hands over --
    32 channels per pixel (xs) in this process, 64 (sc) in the child with the switch."""
    _, prof = new_pair
    n = COUNTS[-1]
    names = [e["name"] for e in prof]
    assert names[:2] == ["layer0_stream_h64(stem+layer0+layer1.0.conv1+sc)"[:47], "layer1_stream_h32(conv2+conv1+conv2)"], names
    assert prof[0]["launches"] == 1 and prof[0]["bytes"] == front_bytes(n, 32), prof[0]
    assert list(old_pair["front_bytes"]) == [front_bytes(n, 64)], old_pair["front_bytes"]


@pytest.mark.parametrize("n", COUNTS)
def test_logits_and_split_modes_are_the_old_pairs_bytes(new_pair, old_pair, n):
    split, logits = new_pair[0][n]
    assert np.isfinite(logits).all() and (split >= 0).all()
    z = n // 2
    assert len({logits[i].tobytes() for i in (z - 1, z, z - 2)}) == 3      # the zero CU, its all-1023 neighbour and a texture CU differ: content reaches the logits
    diff = np.flatnonzero((logits.view(np.uint32) != old_pair[f"logits{n}"].view(np.uint32)).any(axis=1))
    print(f"n = {n}: {len(diff)} CUs with different logit bytes, max |d| = {np.abs(logits - old_pair[f'logits{n}']).max():.3e}")
    assert len(diff) == 0, diff[:16]
    assert split.tobytes() == old_pair[f"split{n}"].tobytes()
