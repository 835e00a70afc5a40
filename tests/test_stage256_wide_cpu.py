"""CPU: stage256_wide_kernel, the whole 256-channel stage with both cout passes per wave (hipcc cross-compiles gfx950 here): the new symbol is held to
the budgets of a kernel that runs two waves per SIMD beside a full LDS -- at most 256 VGPRs, no scratch op, no compiler-made vmcnt wait inside a loop,
no static LDS beside the 160 KiB its launcher asks for -- the chain_kernel instantiations it stands beside are all still there, and the dispatcher's
launch plans say where it runs: the single-pass whole-stage launch of the 256 stage, nowhere else."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
TAG = "both cout passes per wave"
WIDE = "stage256_wide_kernel("
STAGE_256 = "stage_256_h8(s2+sc,conv2,conv1,conv2)"
OLD = ("chain_kernel<256, 3, 1, 2, 1, 2, 4, 3, 2, 2, 2, 3, true, true, true, true, false, false>",     # the A/B partner (MLT_TUNING=1 MLT_NO_STAGE256_WIDE=1)
       "chain_kernel<256, 3, 1, 2, 1, 2, 4, 3, 2, 2, 2, 3, true, true, true, false, false, false>",    # devices that fail the LDS probe
       "chain_kernel<128, 4, 0, 2, 2, 2, 4, 3, 2, 2, 2, 3, true, true, true, true, false, false>",
       "chain_kernel<128, 4, 0, 2, 2, 2, 4, 3, 2, 2, 2, 3, true, true, true, false, false, false>",
       "chain_kernel<256, 3, 1, 2, 1, 2, 4, 3, 2, 2, 2, 3, true, false, true, false, false, false>",   # the chain behind a stride-2 launch of its own
       "chain_kernel<256, 3, 1, 2, 1, 2, 4, 1, 2, 1, 2, 3, true, false, true, true, true, true>",      # hi+lo weights
       "chain_kernel<64, 5, 0, 2, 4, 1, 8, 2, 2, 1, 2, 3, true, false, false, true, false, false>")


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


def _descriptor(symbol):
    """{field: value} of the .amdhsa_kernel block of `symbol` in the assembly isa_waits.collect() wrote"""
    import isa_waits
    out, inside = {}, False
    for line in open(isa_waits.ASM):
        t = line.split()
        if len(t) == 2 and t[0] == ".amdhsa_kernel":
            inside = t[1] == symbol
        elif inside and t and t[0] == ".end_amdhsa_kernel":
            break
        elif inside and len(t) == 2 and t[0].startswith(".amdhsa_"):
            out[t[0][len(".amdhsa_"):]] = int(t[1], 0)
    return out


def test_the_new_symbol_meets_the_budgets_of_two_waves_per_simd(stats):
    import isa_waits
    st = _find(stats, WIDE)
    assert st["scratch"] == 0, f"{st['scratch']} scratch ops (register spills)"
    assert not isa_waits.scratch_in_loops(WIDE)
    inner = [w for w in st["waits"] if w[1] >= 1]
    assert not inner, f"compiler-generated vmcnt waits inside loops: {inner[:5]}"
    assert st["glds"] > 50                                   # the LDS-DMA staging is there
    d = _descriptor("_Z20stage256_wide_kernel9ChainArgs")
    print(d)
    assert 0 < d["next_free_vgpr"] <= 256, d                 # VGPRs + AGPRs of the unified file: 512 per SIMD lane, two waves
    assert d["group_segment_fixed_size"] == 0, d             # all of its LDS is the dynamic allocation of the launcher ...
    src = open(os.path.join(ROOT, "fastintercu-vvc_amd", "csrc", "mlt_kernels.hip")).read()
    m = re.search(r"launch_chain_t\(stage256_wide_kernel, once, a, grid_x, 512, (\d+) \* 1024, st\)", src)
    assert m and int(m.group(1)) <= 160, "... which asks for at most 160 KiB"


@pytest.mark.parametrize("kernel", OLD)
def test_the_old_instantiations_are_still_there(stats, kernel):
    _find(stats, kernel)


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


def _tagged(lines):
    return [l.split(" [")[0] for l in lines if TAG in l]


@pytest.mark.parametrize("n", [257, 258, 600, 4096])
def test_the_single_pass_whole_stage_launch_of_the_256_stage_carries_the_tag(plan, n):
    """from 257 CUs on (n * 64 output pixels > 16384) the 256 stage is one launch; it keeps its name and is the only tagged launch of the plan"""
    p = plan(n)
    assert [l.split(" [")[0] for l in p].count(STAGE_256) == 1, p
    assert _tagged(p) == [STAGE_256], p
    assert _tagged(plan(n, aligned=0)) == [STAGE_256]


@pytest.mark.parametrize("kw", [dict(n=256), dict(n=64), dict(n=4096, w2_units=0x40), dict(n=4096, w2_units=0x80), dict(n=4096, w2_units=0xC0)],
                         ids=["256 CUs: per-conv launches", "64 CUs", "stride-2 unit on hi+lo weights", "chain unit on hi+lo weights", "whole stage on hi+lo weights"])
def test_every_other_plan_is_untagged(plan, kw):
    p = plan(**kw)
    assert not _tagged(p), p
    assert STAGE_256 not in [l.split(" [")[0] for l in p], p   # ... because none of them has the whole-stage launch of the 256 stage
