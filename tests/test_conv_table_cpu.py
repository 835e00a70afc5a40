"""CPU: the per-conv kernels' launch table (csrc/mlt_kernels.hip: one row per instantiation of conv_mfma_kernel / conv_ring_dma_kernel; selection, launch
geometry and the host's packing view all derived from it), as text through the host-only hook mlt_debug_conv_table.

tests/golden/conv_launch_table.txt is that text as the launchers produced it BEFORE they were table-driven: captured from the commit before, with a throwaway patch
that printed the template arguments, thread count, grid.y and LDS bytes from inside launch_conv_t / launch_ring_dma_t (ahead of any HIP call) while mlt_launch_conv
and mlt_conv_cfg were driven over the same domain.  So the fixture pins what every key launched and what it refused, independently of the table.

Edited by hand since, in 44 lines, when the ten nsplit-3 rows no context could launch were removed: every nsplit-3 key is "rejected" now, so is (nsplit 4, default) of
64->96 and 96->128 (it was an alias of their nsplit-3 row), and gt_w2 reads 0 for the six layers without an (nsplit 4, default) row."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_rows_common as crc


@pytest.fixture(scope="module")
def table(pkg):
    pkg.build.build_lib()
    lib = pkg.capi.load_library()
    lib.mlt_debug_conv_table.argtypes = [C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 17)
    n = lib.mlt_debug_conv_table(buf, 1 << 17)
    assert n > 0
    assert lib.mlt_debug_conv_table(buf, 100) == -1   # too small a buffer is reported, not overrun
    lib.mlt_debug_conv_table(buf, 1 << 17)
    return buf.raw[:n]


@pytest.fixture(scope="module")
def fixture_text():
    with open(crc.TABLE, "rb") as fh:
        return fh.read()


def test_table_equals_the_launchers_it_replaced(table, fixture_text):
    if table != fixture_text:
        got, want = table.decode().splitlines(), fixture_text.decode().splitlines()
        diff = [f"{w!r} -> {g!r}" for g, w in zip(got, want) if g != w]
        pytest.fail(f"{len(diff)} of {len(want)} lines differ (fixture -> library), {len(got)} lines now:\n" + "\n".join(diff[:20]))


def test_domain_and_rejections(table, fixture_text):
    rows, rejected = crc.load_table(table.decode())
    rows0, rejected0 = crc.load_table(fixture_text.decode())
    assert len(rows0) + len(rejected0) == 10 * 5 * 4   # ten layer shapes x nsplit 1 / 2 / 3 / 4 / 6 x four variants
    assert set(rejected0) <= set(rejected), sorted(set(rejected0) - set(rejected))   # what was refused is still refused
    assert len(set(rows.values())) == 61   # distinct instantiations
    assert sum(l.startswith(b"cfg ") for l in table.splitlines()) == 20   # the packing view per shape, fast and exact


@pytest.fixture(scope="module")
def plans():
    """{case index: table keys of its plan}: one child process per environment (the dispatcher reads its switches once per process)"""
    out = {}
    for env, switches in crc.ENVS.items():
        clean = {k: v for k, v in os.environ.items() if not k.startswith("MLT_")}
        r = subprocess.run([sys.executable, os.path.join(crc.ROOT, "tests", "conv_rows_common.py"), "plan", env], env=dict(clean, **switches),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out.update({int(k): v for k, v in json.loads(r.stdout.splitlines()[-1]).items()})
    return out


def test_gpu_matrix_reaches_every_reachable_row(table, plans):
    """Each case of tests/test_conv_rows_gpu.py, described through mlt_plan_describe, launches per-conv kernels the table accepts; together the cases reach every
    row but the ones listed (with the reason no context can launch them) in conv_rows_common.UNREACHABLE."""
    rows, _ = crc.load_table(table.decode())
    kernels = set(rows.values())
    assert crc.UNREACHABLE <= kernels, crc.UNREACHABLE - kernels
    assert sorted(plans) == list(range(len(crc.CASES)))
    reached = {}
    for i, keys in plans.items():
        assert keys, f"case {crc.CASES[i]} launches no per-conv kernel"
        for k in keys:
            assert k in rows, f"case {crc.CASES[i]}: the plan asks for '{k}', which the table refuses"
            reached.setdefault(rows[k], []).append(i)
    for i in plans:  # no case is idle: each is the first to reach some row, or one of the two multi-workgroup batches
        first = [r for r, cs in reached.items() if min(cs) == i]
        assert first or crc.CASES[i][2] > 1, f"case {crc.CASES[i]} reaches no row of its own"
    assert not (set(reached) & crc.UNREACHABLE), sorted(set(reached) & crc.UNREACHABLE)
    missing = kernels - set(reached) - crc.UNREACHABLE
    assert not missing, f"rows no case reaches: {sorted(missing)}"
    print(f"{len(reached)} of {len(kernels)} rows reached by {len(plans)} cases; {len(crc.UNREACHABLE)} unreachable")
