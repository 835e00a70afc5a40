"""CPU: the xs hand-off between the streaming launches (layer0_stream_xs_kernel -> layer1_stream_xs_kernel): the new symbols are held to their siblings' ISA limits
(tests/test_isa_invariants_cpu.py; hipcc cross-compiles gfx950 here), and the dispatcher's launch plans say where the pair runs: behind the five-stage front
followed by layer1's streaming launch, nowhere else."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
TAG = "xs hand-off"


@pytest.fixture(scope="module")
def stats():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    import isa_waits
    return isa_waits.collect([])


def _find(stats, prefix):
    hits = [v for k, v in stats.items() if k.startswith(prefix)]
    assert len(hits) == 1, f"{prefix}: {len(hits)} instantiations"
    return hits[0]


def test_front_form_keeps_the_five_stage_kernels_limits(stats):
    """layer0_stream_xs_kernel against layer0_stream_kernel<true, true>'s limits: at most 6 spilled-dword ops and none inside a loop, no LDS-DMA, S1's raw-row
    waits counted; it has lost the shortcut's four MFMAs per S5 row."""
    import isa_waits
    st = _find(stats, "layer0_stream_xs_kernel(")
    assert st["scratch"] <= 6, f"{st['scratch']} scratch ops"
    assert not isa_waits.scratch_in_loops("layer0_stream_xs_kernel("), "scratch ops inside a loop"
    assert st["glds"] == 0
    drains = [w for w in st["waits"] if w[1] >= 1 and "vmcnt(0)" in w[2]]
    assert len(drains) <= 5, f"compiler drains inside loops: {drains}"
    counted = [w for w in st["waits"] if re.search(r"vmcnt\((\d+)\)", w[2]) and int(re.search(r"vmcnt\((\d+)\)", w[2]).group(1)) >= 4]
    assert len(counted) >= 4, f"S1's raw-row waits are no longer counted: {st['waits']}"


def test_layer1_form_fits_its_waves_without_scratch_and_keeps_its_waits_counted(stats):
    """layer1_stream_xs_kernel against layer1_stream_kernel<false>'s limits: no spills, at most 3 vmcnt(0) drains inside loops (two beside the LDS-clearing loop,
    one at the end of the GAP loaders' step group) -- the waits for the xs rows of the shortcut waves are counted."""
    st = _find(stats, "layer1_stream_xs_kernel(")
    assert st["scratch"] == 0, f"{st['scratch']} scratch ops"
    drains = [w for w in st["waits"] if w[1] >= 1 and "vmcnt(0)" in w[2]]
    assert len(drains) <= 3, f"compiler drains inside loops: {drains}"


def test_the_five_old_instantiations_are_still_there(stats):
    for prefix in ("layer0_stream_kernel<true, true>", "layer0_stream_kernel<true, false>", "layer0_stream_kernel<false, false>", "layer1_stream_kernel<true>",
                   "layer1_stream_kernel<false>"):
        _find(stats, prefix)


@pytest.fixture(scope="module")
def plan(pkg):
    pkg.build.build_lib()
    lib = pkg.capi.load_library()
    lib.mlt_plan_describe.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_char_p, C.c_size_t]
    blob = pkg.weights.synthetic_blob(pkg.synth.arch_for_size(128), 10)

    def go(n, w2_units=0, aligned=1):
        buf = C.create_string_buffer(1 << 15)
        k = lib.mlt_plan_describe(blob, len(blob), 128, n, 0, w2_units, 0, aligned, buf, 1 << 15)
        lines = buf.value.decode().splitlines()
        assert k == len(lines) and k > 0, (k, lines)
        return lines
    return go


def _args(line):
    m = re.search(r"\{(.*)\}$", line)
    return {k: int(v, 0) for k, v in (kv.split("=") for kv in m.group(1).split())}


def test_the_headline_plan_carries_the_tag_on_its_two_streaming_launches(plan):
    p = plan(4096)
    assert [l.split(" [")[0] for l in p] == ["layer0_stream_h64(stem+layer0+layer1.0.conv1+sc)", "layer1_stream_h32(conv2+conv1+conv2)", "stage_128_h16(s2+sc,conv2,conv1,conv2)",
                                            "stage_256_h8(s2+sc,conv2,conv1,conv2)", "heads"]
    assert TAG in p[0].split(" [", 1)[1] and TAG in p[1].split(" [", 1)[1] and not any(TAG in l for l in p[2:])
    assert TAG in plan(128)[0] and TAG in plan(128)[1]                       # from the smallest streaming batch on
    a = [_args(l) for l in plan(4096, aligned=3)]
    assert a[0]["y_sc"] == a[1]["sc"] and a[0]["y_t"] == a[1]["t"] and a[0]["y_sc"] != a[0]["y_t"]   # the hand-off buffer keeps its record keys and its place


@pytest.mark.parametrize("kw", [dict(n=4096, w2_units=0x5), dict(n=4096, w2_units=0xC), dict(n=4096, aligned=0), dict(n=127)],
                         ids=["tiled stride-2 conv in front of layer1's streaming launch", "four-stage front + chain", "unaligned planes", "below the thresholds"])
def test_every_other_plan_keeps_the_sc_hand_off(plan, kw):
    p = plan(**kw)
    assert not any(TAG in l for l in p), p
