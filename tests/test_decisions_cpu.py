"""CPU: per-level decision records and the confidence gate -- the C ABI's new exports, the host restatement (decisions.from_logits) against the
committed reference fixtures, the sweep tool, the stats-line parser, the predictor's MLTCNN_MIN_CONF parser, and heads_kernel's register budget.
No compute call reaches a device here; the device side is tests/test_decisions_gpu.py."""
import ctypes as C
import importlib.util
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from helpers import SIZES, head_slices, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("mlt_set_confidence_gate", "mlt_get_confidence_gate", "mlt_predict_decision", "mlt_predict_batch_decisions",
               "mlt_predict_batch_device_decisions", "mlt_wait_decision")
WITHHELD_AT_075 = {128: 67, 64: 44, 32: 44, 16: 45}   # of the 125 CUs of each fixture file, decision head 2 (128) / 0, computed from the fixtures


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build.build_lib()
    return pkg.capi.load_library()


def test_header_declares_and_library_exports_the_decision_calls(pkg, lib):
    header = open(os.path.join(ROOT, "include", "mltcnn.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in mltcnn.h"
        assert name in pkg.capi.EXPORTS and hasattr(lib, name), f"{name} not exported"
    assert "#define MLT_ABI_VERSION 4" in header and lib.mlt_abi_version() == 4   # new exports, no ABI bump


def test_null_ctx_decision_calls_are_argument_errors(lib):
    d = (C.c_char * 48)()
    v = C.c_float(0.0)
    assert lib.mlt_set_confidence_gate(None, 128, C.c_float(0.5)) == 1
    assert lib.mlt_get_confidence_gate(None, 128, C.byref(v)) == 1
    assert lib.mlt_predict_decision(None, None, 128, None, 128, 128, 0, 32, None, None) == 1
    assert lib.mlt_predict_batch_decisions(None, 1, 128, None, None, None, None, d, None) == 1
    assert lib.mlt_predict_batch_device_decisions(None, 1, 128, None, None, None, None, d, None) == 1
    assert lib.mlt_wait_decision(None, 128, C.c_uint64(0), None, None) == 1


def test_decision_struct_layout(pkg):
    D = pkg.capi.MltDecision
    assert C.sizeof(D) == 48
    assert (D.split_mode.offset, D.raw_mode.offset, D.confidence.offset, D.margin.offset, D.level_mode.offset, D.level_conf.offset) == (0, 4, 8, 12, 16, 32)
    dt = pkg.capi.DECISION_DTYPE
    assert dt.itemsize == 48 and [dt.fields[k][1] for k in ("split_mode", "raw_mode", "confidence", "margin", "level_mode", "level_conf")] == [0, 4, 8, 12, 16, 32]
    assert dt.names == pkg.decisions.DTYPE.names   # the float64 restatement carries the same fields


@pytest.mark.parametrize("size", SIZES)
def test_from_logits_against_the_reference_fixtures(pkg, size):
    """level_mode = the fixture's recorded argmax for every head of every CU; level_conf = torch.softmax of the recorded logits in float64;
    the gate at 0.75 withholds the number of CUs computed from the fixtures."""
    import torch
    golden = load_golden(size)
    classes = pkg.decisions.HEAD_CLASSES[size]
    dh = 2 if size == 128 else 0
    withheld = cus = 0
    for case in golden["cases"]:
        lg = np.array(case["logits"], np.float64)
        d = pkg.decisions.from_logits(size, lg)
        g = pkg.decisions.from_logits(size, lg, min_confidence=0.75)
        arg = np.array(case["argmax"])
        for h, sl in enumerate(head_slices(classes)):
            assert np.array_equal(d["level_mode"][:, h], arg[:, h]), (case["name"], h)
            p = torch.softmax(torch.from_numpy(lg[:, sl]), dim=1).numpy()
            want = p[np.arange(len(lg)), arg[:, h]]
            assert np.abs(d["level_conf"][:, h] - want).max() <= 1e-12, (case["name"], h)
        for h in range(len(classes), 4):
            assert (d["level_mode"][:, h] == -1).all() and (d["level_conf"][:, h] == 0).all()
        assert np.array_equal(d["raw_mode"], arg[:, dh]) and np.array_equal(d["split_mode"], d["raw_mode"])
        assert np.array_equal(d["confidence"], d["level_conf"][:, dh])
        top = np.sort(lg[:, head_slices(classes)[dh]], axis=1)
        assert np.array_equal(d["margin"], top[:, -1] - top[:, -2])
        assert np.array_equal(g["raw_mode"], d["raw_mode"]) and np.array_equal(g["confidence"], d["confidence"])
        assert np.array_equal(g["split_mode"], np.where(d["confidence"] >= 0.75, d["raw_mode"], -1))
        if case["variant"] == "tie":   # rows 0 and 1 of the decision head are identical, any others 1000 below: first index, probability 1/2
            tied = d["margin"] == 0      # (the 128 fixture ties exactly; the reference's own fp32 arithmetic leaves ~4e-6 between the rows of some small-model CUs)
            assert tied.any() and (tied.all() or size != 128)
            assert (d["raw_mode"][tied] == 0).all() and (d["confidence"][tied] == 0.5).all()
            assert np.abs(d["confidence"] - 0.5).max() < 1e-5 and (d["level_mode"][:, dh] <= 1).all()
        withheld += int((g["split_mode"] == -1).sum())
        cus += len(lg)
    assert cus == 125 and withheld == WITHHELD_AT_075[size], (cus, withheld)


def test_from_logits_head_choice_nan_and_single_row(pkg):
    lg = np.array([0.0, 1.0, 3.0, 1.0, 2.0, 0.5, 0.5, 0.25, 0.0], np.float64)
    d = pkg.decisions.from_logits(128, lg, head_index=1)
    assert d.shape == (1,) and d["raw_mode"][0] == 0 and d["margin"][0] == 1.0
    assert d["level_mode"][0].tolist() == [1, 0, 0, -1]   # first-max rule on the tied pair of the third head
    assert d["confidence"][0] == pytest.approx(1.0 / (1.0 + np.exp(-2.0) + np.exp(-1.0)), abs=1e-15)
    lg[2] = np.nan
    g = pkg.decisions.from_logits(128, lg, head_index=1, min_confidence=0.1)
    assert np.isnan(g["confidence"][0]) and g["split_mode"][0] == -1   # a NaN confidence gates


def _write_dump(path, records):
    """The call-dump record format of host/mlt_split_predictor.hpp (dumpCall)."""
    with open(path, "wb") as f:
        for cuw, poc, qp, split, lg in records:
            f.write(struct.pack("<6i", 0x4D4C5443, cuw, poc, qp, split, len(lg)))
            f.write(np.concatenate([np.asarray(lg, "<f4"), np.zeros(15 - len(lg), "<f4")]).tobytes())
            f.write(np.zeros((2, cuw, cuw), "<i2").tobytes())


def test_confidence_sweep_on_a_dump_of_fixture_logits(pkg, tmp_path, capsys):
    cs = _tool("confidence_sweep")
    records = []
    for size in (128, 16):
        for case in load_golden(size)["cases"]:
            for row, arg in zip(case["logits"], case["argmax"]):
                records.append((size, 8, 32, arg[2 if size == 128 else 0], row))
    dump = str(tmp_path / "calls.bin")
    _write_dump(dump, records)
    assert cs.main([dump, "--grid", "0.5,0.75,0.9", "--json"]) == 0
    import json
    rep = json.loads(capsys.readouterr().out)
    assert set(rep) == {"128", "16"}
    for size in (128, 16):
        r = rep[str(size)]
        assert r["calls"] == 125 and [t["min_confidence"] for t in r["thresholds"]] == [0.5, 0.75, 0.9]
        t50, t75, t90 = r["thresholds"]
        assert t75["withheld"] == WITHHELD_AT_075[size] and t75["withheld_share"] == pytest.approx(WITHHELD_AT_075[size] / 125)
        assert t50["withheld"] <= t75["withheld"] <= t90["withheld"]
        for t in r["thresholds"]:
            assert sum(t["kept_split_histogram"].values()) == 125 - t["withheld"]
    assert cs.main([dump, "--grid", "0.75"]) == 0
    text = capsys.readouterr().out
    assert "size 128: 125 calls" in text and "withheld     67 ( 53.6 %)" in text
    with pytest.raises(SystemExit):
        cs.main([dump, "--grid", "1.0"])


def test_stats_line_parser_reports_gated_only_when_present(pkg):
    eh = _tool("eval_harness")
    base = ("mltcnn-stats predict_calls=10 predict_s=0.002000 submit_calls=0 submit_s=0.000000 wait_calls=0 wait_s=0.000000 flush_calls=0 flush_s=0.000000 "
            "calls_128=10 calls_64=0 calls_32=0 calls_16=0 failed=0 init_s=1.500000")
    plain = eh.parse_predictor_stats("noise\n" + base + "\n")
    assert plain["cnn_calls"] == 10 and plain["cnn_failed"] == 0 and "cnn_gated" not in plain
    gated = eh.parse_predictor_stats("noise\n" + base + " gated=4\nmore\n")
    assert gated["cnn_gated"] == 4 and gated["cnn_failed"] == 0 and gated["cnn_calls"] == 10
    assert {k: v for k, v in gated.items() if k != "cnn_gated"} == plain


def test_predictor_min_conf_parser_and_decision_calls_build(pkg, tmp_path):
    """host/mlt_split_predictor.hpp: MLTCNN_MIN_CONF is one number or size:value pairs, anything malformed leaves every gate off; predictDecision /
    waitDecision compile against the C ABI and fail cleanly (-1 in the record) without a device."""
    lib = pkg.build.build_lib()
    src = tmp_path / "min_conf.cpp"
    src.write_text(r'''
#include "mlt_split_predictor.hpp"
int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) {
    float thr[4];
    const bool ok = mlt::SplitPredictor::parseMinConf(argv[i], thr);
    std::printf("%d %.4f %.4f %.4f %.4f\n", (int)ok, thr[0], thr[1], thr[2], thr[3]);
  }
  mlt::SplitPredictor cnn("/nonexistent");   // no weights (and maybe no device): every call fails the reference's way
  mlt::Pel plane[16 * 16] = {0};
  mlt_decision d;
  const bool a = cnn.predictDecision(plane, 16, plane, 16, 16, 0, 32, &d);
  const bool b = cnn.waitDecision(16, 0, &d);
  std::printf("calls %d %d %d %d\n", (int)a, (int)b, d.split_mode, d.raw_mode);
  return 0;
}
''')
    exe = str(tmp_path / "min_conf")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "host"), str(src), "-o", exe,
           "-L" + os.path.dirname(lib), "-lmltcnn_hip", "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    specs = ["0.75", "128:0.9,64:0.8", "16:0.5", "0", "1.0", "-0.1", "nan", "abc", "128:0.9,", "48:0.5", "128=0.9", "", "128:0.9,64:1.5", "0.5x"]
    out = subprocess.run([exe] + specs, capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib", MLTCNN_MIN_CONF="0.5"))
    assert out.returncode == 0, out.stderr
    rows = [l.split() for l in out.stdout.splitlines()]
    got = [(int(r[0]), [float(v) for v in r[1:]]) for r in rows[:len(specs)]]
    assert got[0] == (1, [0.75] * 4) and got[1] == (1, [0.9, 0.8, 0.0, 0.0]) and got[2] == (1, [0.0, 0.0, 0.0, 0.5]) and got[3] == (1, [0.0] * 4)
    for spec, g in zip(specs[4:], got[4:]):
        assert g == (0, [0.0] * 4), spec
    assert rows[len(specs)] == ["calls", "0", "0", "-1", "-1"]


def test_heads_kernel_still_uses_no_scratch():
    """The softmax, the record and the gate ride on heads_kernel (pure latency, part of every one-CU call): no register spill, no private array
    in scratch memory -- read from the compiler's own statistics like tests/test_isa_invariants_cpu.py does."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_waits
    stats = isa_waits.collect([])
    for kernel in ("heads_kernel<false>(", "heads_kernel<true>(", "guard_select_kernel(", "guard_scatter_kernel("):   # <true>: with records / gate
        hits = [v for k, v in stats.items() if k.startswith(kernel)]
        assert len(hits) == 1, (kernel, len(hits))
        assert hits[0]["scratch"] == 0, f"{kernel}: {hits[0]['scratch']} scratch ops"
    asm = open(isa_waits.ASM).read()
    for sym in ("_Z12heads_kernelILb0EEv8HeadArgs", "_Z12heads_kernelILb1EEv8HeadArgs"):
        meta = asm[asm.index(".amdhsa_kernel " + sym):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta)
        assert m and int(m.group(1)) == 0, (sym, m and m.group(0))
