"""CPU: candidate split sets -- the C ABI's new exports, the host restatement (decisions.candidates_from_logits) against the committed reference
fixtures, the sweep tool, the predictor's MLTCNN_CANDIDATES parser, and the register budget of heads_cand_kernel and the guard kernels it touches.
No compute call reaches a device here; the device side is tests/test_candidates_gpu.py."""
import ctypes as C
import importlib.util
import json
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from helpers import SIZES, head_slices, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("mlt_set_candidate_policy", "mlt_get_candidate_policy", "mlt_predict_candidates", "mlt_predict_batch_candidates",
               "mlt_predict_batch_device_candidates", "mlt_wait_candidates")
# kept-count histograms (one class kept ... K kept) over the 125 CUs of each fixture file, float64 on the committed logits: (size, head, coverage, max_modes)
KEPT = {
    (128, 2, 0.8, 0): [52, 66, 7, 0],
    (128, 2, 0.9, 0): [51, 50, 24, 0],
    (128, 2, 0.9, 2): [51, 50, 0, 24],
    (64, 3, 0.9, 0): [98, 18, 2, 4, 3, 0],
    (64, 3, 0.9, 2): [98, 18, 0, 0, 0, 9],
    (32, 3, 0.9, 0): [90, 23, 3, 7, 2, 0],
    (16, 3, 0.9, 0): [91, 20, 3, 5, 2, 4],
    (64, 0, 0.9, 0): [77, 48],
    (32, 0, 0.9, 0): [77, 48],
    (16, 0, 0.9, 0): [77, 48],
}


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build.build_lib()
    return pkg.capi.load_library()


def _fixture_logits(size):
    return [np.array(case["logits"], np.float64) for case in load_golden(size)["cases"]], load_golden(size)["cases"]


def test_header_declares_and_library_exports_the_candidate_calls(pkg, lib):
    header = open(os.path.join(ROOT, "include", "mltcnn.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in mltcnn.h"
        assert name in pkg.capi.EXPORTS and hasattr(lib, name), f"{name} not exported"
    assert "typedef struct mlt_candidates" in header
    assert "#define MLT_ABI_VERSION 4" in header and lib.mlt_abi_version() == 4   # new exports, no ABI bump


def test_null_ctx_candidate_calls_are_argument_errors(lib):
    c = (C.c_char * 40)()
    cov, mx = C.c_float(0.0), C.c_int(0)
    assert lib.mlt_set_candidate_policy(None, 128, C.c_float(0.9), 0) == 1
    assert lib.mlt_get_candidate_policy(None, 128, C.byref(cov), C.byref(mx)) == 1
    assert lib.mlt_predict_candidates(None, None, 128, None, 128, 128, 0, 32, None, None, None) == 1
    assert lib.mlt_predict_batch_candidates(None, 1, 128, None, None, None, None, c, None, None) == 1
    assert lib.mlt_predict_batch_device_candidates(None, 1, 128, None, None, None, None, c, None, None) == 1
    assert lib.mlt_wait_candidates(None, 128, C.c_uint64(0), None, None, None) == 1


def test_candidates_struct_layout(pkg):
    S = pkg.capi.MltCandidates
    assert C.sizeof(S) == 40
    assert (S.mask.offset, S.count.offset, S.order.offset, S.prob.offset) == (0, 4, 8, 16)
    dt = pkg.capi.CANDIDATES_DTYPE
    assert dt.itemsize == 40 and [dt.fields[k][1] for k in ("mask", "count", "order", "prob")] == [0, 4, 8, 16]
    assert dt["order"].shape == (8,) and dt["prob"].shape == (6,) and dt["prob"].base == np.dtype("<f4")
    assert pkg.decisions.CAND_DTYPE.names[:4] == dt.names   # the float64 restatement carries the same leading fields


@pytest.mark.parametrize("key", sorted(KEPT), ids=lambda k: f"{k[0]}-head{k[1]}-{k[2]}-max{k[3]}")
def test_restatement_pins_the_kept_count_histograms_of_the_fixtures(pkg, key):
    size, head, cov, mx = key
    K = pkg.decisions.HEAD_CLASSES[size][head]
    hist = np.zeros(K, int)
    cus = 0
    for lg in _fixture_logits(size)[0]:
        c = pkg.decisions.candidates_from_logits(size, lg, head_index=head, coverage=cov, max_modes=mx)
        hist += np.bincount(c["count"], minlength=K + 1)[1:]
        cus += len(c)
        assert np.array_equal(c["count"], [bin(int(v)).count("1") for v in c["mask"]])
        assert (c["mask"] < (1 << K)).all() and (c["order"][:, K:] == -1).all() and (c["prob"][:, K:] == 0).all()
        assert np.array_equal(np.sort(c["order"][:, :K], axis=1), np.tile(np.arange(K), (len(c), 1)))
        assert np.abs(c["prob"][:, :K].sum(axis=1) - 1.0).max() < 1e-12
        if mx:
            assert ((c["count"] <= mx) | (c["count"] == K)).all()
    assert cus == 125 and hist.tolist() == KEPT[key], (key, hist.tolist())


@pytest.mark.parametrize("size", SIZES)
def test_restatement_default_policy_and_the_gate_restated_as_a_mask(pkg, size):
    """(0, 0) keeps the argmax alone; (t, 1) keeps one class iff from_logits' gate at t lets the CU through, else all K -- on every head of every fixture."""
    classes = pkg.decisions.HEAD_CLASSES[size]
    logits, cases = _fixture_logits(size)
    for lg, case in zip(logits, cases):
        for head, K in enumerate(classes):
            d = pkg.decisions.from_logits(size, lg, head_index=head)
            c0 = pkg.decisions.candidates_from_logits(size, lg, head_index=head)
            assert np.array_equal(c0["mask"], np.uint32(1) << d["raw_mode"].astype(np.uint32)) and (c0["count"] == 1).all(), (case["name"], head)
            assert np.array_equal(c0["order"][:, 0], d["raw_mode"])
            assert np.array_equal(c0["prob"][np.arange(len(lg)), d["raw_mode"]], d["confidence"])   # the same operations: equal to the last bit
            assert np.abs(c0["prob"][:, :K] - _softmax64(lg[:, head_slices(classes)[head]])).max() < 1e-12
            for t in (0.5, 0.75, 0.9):
                g = pkg.decisions.from_logits(size, lg, head_index=head, min_confidence=t)
                c1 = pkg.decisions.candidates_from_logits(size, lg, head_index=head, coverage=t, max_modes=1)
                want = np.where(g["split_mode"] >= 0, np.uint32(1) << d["raw_mode"].astype(np.uint32), np.uint32((1 << K) - 1))
                assert np.array_equal(c1["mask"], want), (case["name"], head, t)


def _softmax64(l):
    e = np.exp(l - l.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def test_restatement_exact_ties_keep_the_lower_class_first(pkg):
    """38 CUs of the 128 fixtures hold two classes of EXACTLY equal probability in the decision head: the 36 of the near-tie family (both far-away classes
    underflow to 0) and the 2 of the tie case (equal logits).  The rank never looks at the probabilities: equal LOGITS put the lower class first (the
    first-max rule, extended), unequal ones the larger -- and a coverage just above one half keeps exactly the two classes of an exact logit tie."""
    size = 128
    prob_ties = logit_ties = 0
    for lg in _fixture_logits(size)[0]:
        l = lg[:, head_slices(pkg.decisions.HEAD_CLASSES[size])[2]]
        c = pkg.decisions.candidates_from_logits(size, lg, coverage=0.6)
        for i in range(len(l)):
            order = c["order"][i, :4].astype(int)
            p = c["prob"][i, order]
            if not (p[1:] == p[:-1]).any():
                continue
            prob_ties += 1
            for r in range(3):
                a, b = order[r], order[r + 1]
                assert l[i, a] > l[i, b] or (l[i, a] == l[i, b] and a < b), (i, r)
            if l[i, order[0]] == l[i, order[1]]:
                logit_ties += 1
                assert c["prob"][i, order[0]] == c["prob"][i, order[1]] == 0.5 and c["count"][i] == 2 and c["mask"][i] == (1 << order[0]) | (1 << order[1])
    assert (prob_ties, logit_ties) == (38, 2), (prob_ties, logit_ties)
    # hand-made rows: a three-way tie ranks in class order; a lower logit between equal ones does not disturb them
    lg = np.zeros(9)
    lg[5:9] = [1.0, 2.0, 2.0, 2.0]
    c = pkg.decisions.candidates_from_logits(128, lg, coverage=0.5)
    assert c["order"][0].tolist() == [1, 2, 3, 0, -1, -1, -1, -1] and c["count"][0] == 2 and c["mask"][0] == 0b0110


def test_restatement_nan_cap_prefix_rule_and_input_shapes(pkg):
    lg = np.array([0.0, 1.0, 3.0, 1.0, 2.0, 0.5, 0.5, 0.25, 0.0], np.float64)
    one = pkg.decisions.candidates_from_logits(128, lg, head_index=1, coverage=0.9)
    two = pkg.decisions.candidates_from_logits(128, np.stack([lg, lg]), head_index=1, coverage=0.9)
    assert one.shape == (1,) and two.shape == (2,) and one[0].tobytes() == two[0].tobytes() == two[1].tobytes()
    p = np.exp(np.array([3.0, 1.0, 2.0]) - 3.0)
    p /= p.sum()
    assert one["order"][0].tolist() == [0, 2, 1, -1, -1, -1, -1, -1] and np.allclose(one["prob"][0, :3], p, atol=1e-15)
    assert one["count"][0] == 2 and one["mask"][0] == 0b101 and one["n"][0] == 2      # 0.665 + 0.245 = 0.910 >= 0.9
    assert one["cum"][0, :3] == pytest.approx([p[0], p[0] + p[2], 1.0], abs=1e-15) and one["gap"][0] == 1.0
    capped = pkg.decisions.candidates_from_logits(128, lg, head_index=1, coverage=0.9, max_modes=1)
    assert capped["count"][0] == 3 and capped["mask"][0] == 0b111 and capped["n"][0] == 2 and np.isinf(capped["gap"][0])
    assert pkg.decisions.candidates_from_logits(128, lg, head_index=1, coverage=0.9, max_modes=2)["mask"][0] == 0b101   # the cap is not exceeded
    lg[3] = np.nan
    nan = pkg.decisions.candidates_from_logits(128, lg, head_index=1, coverage=0.1)
    assert nan["mask"][0] == 0b111 and nan["count"][0] == 3 and nan["order"][0, :3].tolist() == [0, 1, 2]   # a NaN row keeps everything
    assert pkg.decisions.candidates_from_logits(128, lg, head_index=2, coverage=0.1)["count"][0] == 1        # ... only in the head that holds it
    for bad in (dict(coverage=1.0), dict(coverage=-0.1), dict(max_modes=4), dict(max_modes=-1)):
        with pytest.raises(AssertionError):
            pkg.decisions.candidates_from_logits(128, lg, head_index=1, **bad)


def _write_dump(path, records):
    """The call-dump record format of host/mlt_split_predictor.hpp (dumpCall)."""
    with open(path, "wb") as f:
        for cuw, poc, qp, split, lg in records:
            f.write(struct.pack("<6i", 0x4D4C5443, cuw, poc, qp, split, len(lg)))
            f.write(np.concatenate([np.asarray(lg, "<f4"), np.zeros(15 - len(lg), "<f4")]).tobytes())
            f.write(np.zeros((2, cuw, cuw), "<i2").tobytes())


def test_candidate_sweep_on_a_dump_of_fixture_logits(pkg, tmp_path, capsys):
    """(the dump stores fp32 logits; the fixtures' logits are fp32 values, so the float64 histograms carry over)"""
    cs = _tool("candidate_sweep")
    records = []
    for size in (128, 64, 16):
        for case in load_golden(size)["cases"]:
            for row, arg in zip(case["logits"], case["argmax"]):
                records.append((size, 8, 32, arg[2 if size == 128 else 0], row))
    dump = str(tmp_path / "calls.bin")
    _write_dump(dump, records)
    assert cs.main([dump, "--coverage", "0.8,0.9", "--max-modes", "0,2", "--head", "128:2,64:3,16:3", "--json"]) == 0
    rep = json.loads(capsys.readouterr().out)
    assert set(rep) == {"128", "64", "16"}

    def row(size, cov, mx):
        r = rep[str(size)]
        assert r["calls"] == 125
        return next(t for t in r["policies"] if t["coverage"] == cov and t["max_modes"] == mx)

    for (size, head, cov, mx), hist in KEPT.items():
        if head == 0 or size == 32:
            continue
        t = row(size, cov, mx)
        assert t["kept_count_histogram"] == hist, (size, cov, mx)
        assert t["full_rdo"] == hist[-1] and t["full_rdo_share"] == pytest.approx(hist[-1] / 125)
        assert t["mean_kept"] == pytest.approx(sum((k + 1) * v for k, v in enumerate(hist)) / 125)
    assert cs.main([dump, "--coverage", "0.9", "--max-modes", "0"]) == 0           # default heads: [2] of the 128 model, [0] of the others
    text = capsys.readouterr().out
    assert "size 128: 125 calls, decision head 2 (4 classes)" in text and "by kept count  1:51 2:50 3:24 4:0" in text
    assert "size 64: 125 calls, decision head 0 (2 classes)" in text and "by kept count  1:77 2:48" in text
    for bad in (["--coverage", "1.0"], ["--max-modes", "7"]):
        with pytest.raises(SystemExit):
            cs.main([dump] + bad)


def test_predictor_candidates_parser_and_candidate_calls_build(pkg, tmp_path):
    """host/mlt_split_predictor.hpp: MLTCNN_CANDIDATES is "coverage[/max]" or size:coverage[/max] pairs, anything malformed leaves every policy at its
    default; predictCandidates / waitCandidates compile against the C ABI with -Wall -Werror and fail cleanly without a device (every class kept,
    raw_mode -1); keptClasses lists the kept classes in rank order."""
    lib = pkg.build.build_lib()
    src = tmp_path / "candidates.cpp"
    src.write_text(r'''
#include "mlt_split_predictor.hpp"
int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) {
    float cov[4];
    int mx[4];
    const bool ok = mlt::SplitPredictor::parseCandidates(argv[i], cov, mx);
    std::printf("%d %.4f/%d %.4f/%d %.4f/%d %.4f/%d\n", (int)ok, cov[0], mx[0], cov[1], mx[1], cov[2], mx[2], cov[3], mx[3]);
  }
  mlt::SplitPredictor cnn("/nonexistent");   // no weights (and maybe no device): every call fails the reference's way
  mlt::Pel plane[16 * 16] = {0};
  mlt_candidates c;
  mlt_decision d;
  const bool a = cnn.predictCandidates(plane, 16, plane, 16, 16, 0, 32, &c, &d);
  std::printf("calls %d %u %d %d %d\n", (int)a, c.mask, c.count, d.split_mode, d.raw_mode);
  const bool b = cnn.waitCandidates(128, 0, &c);
  std::printf("calls %d %u %d %d %d\n", (int)b, c.mask, c.count, (int)c.order[3], (int)c.order[4]);
  mlt_candidates k{};
  k.mask = 0x15; k.count = 3;
  const int8_t order[8] = {4, 1, 2, 0, 3, 5, -1, -1};
  for (int r = 0; r < 8; ++r) k.order[r] = order[r];
  int cls[8];
  const int n = mlt::SplitPredictor::keptClasses(k, cls);
  std::printf("kept %d %d %d %d\n", n, cls[0], cls[1], cls[2]);
  return 0;
}
''')
    exe = str(tmp_path / "candidates")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "host"), str(src), "-o", exe,
           "-L" + os.path.dirname(lib), "-lmltcnn_hip", "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    good = ["0.9", "0.9/2", "128:0.9/2,64:0.8", "16:0.5/6", "0", "0/1", "64:0.95/3,32:0.9,16:0.8/1"]
    bad = ["1.0", "-0.1", "nan", "abc", "0.9/", "0.9/7", "0.9/-1", "0.9/2x", "128:0.9/2,", "48:0.5", "128=0.9", "", "128:0.9,64:1.5", "0.5x", "0.9/2/3", "128:0.9/a"]
    out = subprocess.run([exe] + good + bad, capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib", MLTCNN_CANDIDATES="0.9/2"))
    assert out.returncode == 0, out.stderr
    rows = [l.split() for l in out.stdout.splitlines()]

    def parsed(r):
        return int(r[0]), [(float(t.split("/")[0]), int(t.split("/")[1])) for t in r[1:]]

    got = [parsed(r) for r in rows[:len(good) + len(bad)]]
    assert got[0] == (1, [(0.9, 0)] * 4) and got[1] == (1, [(0.9, 2)] * 4)
    assert got[2] == (1, [(0.9, 2), (0.8, 0), (0.0, 0), (0.0, 0)]) and got[3] == (1, [(0.0, 0), (0.0, 0), (0.0, 0), (0.5, 6)])
    assert got[4] == (1, [(0.0, 0)] * 4) and got[5] == (1, [(0.0, 1)] * 4)
    assert got[6] == (1, [(0.0, 0), (0.95, 3), (0.9, 0), (0.8, 1)])
    for spec, g in zip(bad, got[len(good):]):
        assert g == (0, [(0.0, 0)] * 4), spec
    tail = rows[len(good) + len(bad):]
    assert tail[0] == ["calls", "0", "3", "2", "-1", "-1"]        # 16 x 16: decision head [0], two classes -- both kept
    assert tail[1] == ["calls", "0", "15", "4", "3", "-1"]        # 128 x 128: decision head [2], four classes
    assert tail[2] == ["kept", "3", "4", "2", "0"]


def test_candidate_kernels_use_no_scratch():
    """heads_cand_kernel sorts, sums and masks up to six classes in registers: no spill, no private array in scratch memory, and neither in the guard
    kernels that share head_candidates or carry the records -- read from the compiler's own statistics.  The two heads_kernel instantiations
    are still there, once each, beside the new kernel."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_waits
    stats = isa_waits.collect([])
    for kernel in ("heads_cand_kernel(", "heads_kernel<false>(", "heads_kernel<true>(", "guard_select_kernel(", "guard_scatter_kernel("):
        hits = [v for k, v in stats.items() if k.startswith(kernel)]
        assert len(hits) == 1, (kernel, len(hits))
        assert hits[0]["scratch"] == 0, f"{kernel}: {hits[0]['scratch']} scratch ops"
    assert len([k for k in stats if k.startswith("heads_")]) == 3
    asm = open(isa_waits.ASM).read()
    for sym in ("_Z17heads_cand_kernel8HeadArgs", "_Z12heads_kernelILb0EEv8HeadArgs", "_Z12heads_kernelILb1EEv8HeadArgs",
                "_Z19guard_select_kernel15GuardSelectArgs", "_Z20guard_scatter_kernel16GuardScatterArgs"):
        meta = asm[asm.index(".amdhsa_kernel " + sym):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta)
        assert m and int(m.group(1)) == 0, (sym, m and m.group(0))
