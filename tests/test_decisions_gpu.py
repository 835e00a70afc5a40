"""GPU (MI355X): per-level decision records and the confidence gate through the C ABI, against the committed reference fixtures
(tests/golden/golden_{128,64,32,16}.json) and the host restatement decisions.from_logits.

Bounds (none of them taken from what the device returns):
  CONF_EPS = 2e-6            device fp32 softmax against float64 on THE SAME logits: expf at <= 2 ulp (the HIP math API documents 1 ulp for expf), at most
                             six terms, one division, probabilities <= 1
  LOGIT_TOL / 2 + CONF_EPS   confidence against the reference: two logits within LOGIT_TOL of the reference move a softmax probability by at most
                             LOGIT_TOL / 2 (DESIGN.md "Numerics")
  EXACT_NOISE / 2 + CONF_EPS the same for CUs that went through the exact re-run (|dlogit| <= EXACT_NOISE)"""
import os
import subprocess

import numpy as np
import pytest

from helpers import EXACT_NOISE, SIZES, check_splits, head_slices, load_golden, materialise

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3
CONF_EPS = 2e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


def _ctx(pkg, size, blob, **kw):
    return pkg.MltCnn(device=0, sizes=(size,), blobs={size: blob}, **kw)


def _dh(size):
    return 2 if size == 128 else 0


def _classes(size):
    return [2, 3, 4] if size == 128 else [2, 3, 4, 6]


def _device_pair(pkg, m, size, org, pred, poc, qp, decisions):
    """The device-pointer entry: (split or records, logits) of one batch."""
    import torch
    dev = torch.device("cuda", 0)
    n, nl = len(poc), m.num_logits(size)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (org, pred, poc, qp)]
    d_lg = torch.zeros((n, nl), dtype=torch.float32, device=dev)
    if decisions:
        d_out = torch.zeros((n * 48,), dtype=torch.uint8, device=dev)
        m.predict_batch_device(n, size, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), None, d_lg.data_ptr(), d_decisions=d_out.data_ptr())
        m.synchronize()
        return np.frombuffer(d_out.cpu().numpy().tobytes(), pkg.capi.DECISION_DTYPE).copy(), d_lg.cpu().numpy()
    d_out = torch.full((n,), -7, dtype=torch.int32, device=dev)
    m.predict_batch_device(n, size, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d_out.data_ptr(), d_lg.data_ptr())
    m.synchronize()
    return d_out.cpu().numpy(), d_lg.cpu().numpy()


def _same_records(a, b):
    return a.tobytes() == b.tobytes()


def _check_records_describe_logits(pkg, size, dec, logits, what):
    """Every field of the device's records against from_logits of the logits the SAME call returned."""
    ref = pkg.decisions.from_logits(size, logits)
    assert np.array_equal(dec["level_mode"], ref["level_mode"]), what
    assert np.array_equal(dec["raw_mode"], ref["raw_mode"]), what
    sl = head_slices(_classes(size))[_dh(size)]
    ulp = np.spacing(np.abs(logits[:, sl]).max(axis=1).astype(np.float32)).astype(np.float64)   # 1 ulp of the larger logit
    assert (np.abs(dec["margin"].astype(np.float64) - ref["margin"]) <= ulp).all(), what
    worst = max(float(np.abs(dec["confidence"] - ref["confidence"]).max()), float(np.abs(dec["level_conf"] - ref["level_conf"]).max()))
    assert worst <= CONF_EPS, (what, worst)
    return worst


@pytest.mark.parametrize("size", SIZES)
def test_records_bit_identity_and_accuracy_on_every_fixture(gpu, size):
    """Gate off, shipped configuration (flags = 0), every fixture case, every entry point: the decision twin returns logits bit-equal to the existing
    call's and raw_mode == split_mode == its split; the records describe the returned logits (CONF_EPS) and lie within LOGIT_TOL / 2 + CONF_EPS of the
    reference's confidences -- no CU left out."""
    pkg = gpu
    golden = load_golden(size)
    dh = _dh(size)
    worst_self = worst_ref = 0.0
    for case in golden["cases"]:
        blob, org, pred, poc, qp, exp, exp_arg = materialise(pkg, golden, case)
        what = f"{size}/{case['name']}"
        m = _ctx(pkg, size, blob)
        assert m.confidence_gate(size) == 0.0
        split, logits = m.predict_batch(org, pred, poc, qp)
        dec, lg_d = m.predict_batch_decisions(org, pred, poc, qp)
        assert np.array_equal(lg_d.view(np.uint32), logits.view(np.uint32)), what
        assert np.array_equal(dec["raw_mode"], split) and np.array_equal(dec["split_mode"], split), what
        only, none = m.predict_batch_decisions(org, pred, poc, qp, want_logits=False)
        assert none is None and _same_records(only, dec), what
        worst_self = max(worst_self, _check_records_describe_logits(pkg, size, dec, lg_d, what))
        ref = pkg.decisions.from_logits(size, exp)
        err = max(float(np.abs(dec["confidence"] - ref["confidence"]).max()), float(np.abs(dec["level_conf"] - ref["level_conf"]).max()))
        worst_ref = max(worst_ref, err)
        assert err <= LOGIT_TOL / 2 + CONF_EPS, (what, err)
        assert (dec["level_mode"][:, len(_classes(size)):] == -1).all() and (dec["level_conf"][:, len(_classes(size)):] == 0).all()
        # device-pointer pair
        s_dev, l_dev = _device_pair(pkg, m, size, org, pred, poc, qp, False)
        d_dev, l_dev2 = _device_pair(pkg, m, size, org, pred, poc, qp, True)
        assert np.array_equal(s_dev, split) and np.array_equal(l_dev, logits) and np.array_equal(l_dev2, logits) and _same_records(d_dev, dec), what
        # one CU per call, and the deferred pair
        tickets = [m.submit(org[i], pred[i], int(poc[i]), int(qp[i])) for i in range(len(poc))]
        for i in range(len(poc)):
            s1, l1 = m.predict(org[i], pred[i], int(poc[i]), int(qp[i]))
            d1, l1d = m.predict_decision(org[i], pred[i], int(poc[i]), int(qp[i]))
            assert s1 == split[i] and np.array_equal(l1, logits[i]) and np.array_equal(l1d, l1) and _same_records(d1, dec[i]), (what, i)
            s2, l2 = m.wait(size, tickets[i])
            d2, l2d = m.wait_decision(size, tickets[i])
            assert s2 == split[i] and np.array_equal(l2, logits[i]) and np.array_equal(l2d, l2) and _same_records(d2, dec[i]), (what, i)
        m.close()
        # one context serving two device contexts (the same GPU twice): shards of the batch, same bits
        m2 = pkg.MltCnn(sizes=(size,), blobs={size: blob}, devices=[0, 0])
        s_2, l_2 = m2.predict_batch(org, pred, poc, qp)
        d_2, l_2d = m2.predict_batch_decisions(org, pred, poc, qp)
        assert np.array_equal(s_2, split) and np.array_equal(l_2, logits) and np.array_equal(l_2d, logits) and _same_records(d_2, dec), what
        m2.close()
    print(size, f"confidence vs from_logits(own logits): worst {worst_self:.2e} (bound {CONF_EPS:.0e}); vs the reference: worst {worst_ref:.2e} (bound {LOGIT_TOL / 2 + CONF_EPS:.2e})")


@pytest.mark.parametrize("size", SIZES)
def test_gate_away_from_ties_on_every_entry_point(gpu, size):
    """Gate 0.75, flags = 0.  No reference confidence lies within 1.2e-2 of 0.75 in any fixture file, so no CU is excused on account of the gate: every CU
    whose reference decision helpers.check_splits can decide returns the reference's GATED decision -- single, batch, device pointer, deferred, and the
    record twins.  The CUs not compared are the reference's own argmax ties, counted as check_splits counts them."""
    pkg = gpu
    golden = load_golden(size)
    gate = 0.75
    sl = head_slices(_classes(size))[_dh(size)]
    undecided = withheld = 0
    for case in golden["cases"]:
        blob, org, pred, poc, qp, exp, exp_arg = materialise(pkg, golden, case)
        what = f"{size}/{case['name']}"
        ref = pkg.decisions.from_logits(size, exp, min_confidence=gate)
        assert np.abs(ref["confidence"] - gate).min() > 1.2e-2, what
        m = _ctx(pkg, size, blob)
        m.set_confidence_gate(size, gate)
        assert m.confidence_gate(size) == gate
        n = len(poc)
        split, logits = m.predict_batch(org, pred, poc, qp)
        undecided += check_splits(split, exp, ref["split_mode"], sl, True, LOGIT_TOL, what + " batch")
        withheld += int((split == -1).sum())
        dec, lg_d = m.predict_batch_decisions(org, pred, poc, qp)
        assert np.array_equal(dec["split_mode"], split) and np.array_equal(lg_d, logits), what
        assert (dec["split_mode"] == np.where(dec["confidence"] >= np.float32(gate), dec["raw_mode"], -1)).all(), what
        check_splits(dec["raw_mode"], exp, ref["raw_mode"], sl, True, LOGIT_TOL, what + " raw")
        s_dev, _ = _device_pair(pkg, m, size, org, pred, poc, qp, False)
        d_dev, _ = _device_pair(pkg, m, size, org, pred, poc, qp, True)
        check_splits(s_dev, exp, ref["split_mode"], sl, True, LOGIT_TOL, what + " device")
        assert np.array_equal(s_dev, split) and _same_records(d_dev, dec), what
        tickets = [m.submit(org[i], pred[i], int(poc[i]), int(qp[i])) for i in range(n)]
        s_one = np.array([m.predict(org[i], pred[i], int(poc[i]), int(qp[i]))[0] for i in range(n)], np.int32)
        s_def = np.array([m.wait(size, t)[0] for t in tickets], np.int32)
        d_one = [m.predict_decision(org[i], pred[i], int(poc[i]), int(qp[i]))[0] for i in range(n)]
        d_def = [m.wait_decision(size, t)[0] for t in tickets]
        check_splits(s_one, exp, ref["split_mode"], sl, True, LOGIT_TOL, what + " single")
        check_splits(s_def, exp, ref["split_mode"], sl, True, LOGIT_TOL, what + " deferred")
        assert np.array_equal(s_one, split) and np.array_equal(s_def, split), what
        for i in range(n):
            assert _same_records(d_one[i], dec[i]) and _same_records(d_def[i], dec[i]), (what, i)
        m.close()
    print(size, f"gate {gate}: {withheld} of 125 CUs withheld, {undecided} CUs whose reference argmax is a tie of its own arithmetic")
    if size == 128:
        assert undecided <= 10, undecided   # (the bound tests/test_hip_parity.py uses for the 128 model)


def test_gate_through_a_near_tie_family_is_decided_by_the_exact_arithmetic(gpu):
    """128 model, flags = 0, gate 0.50015: 33 reference confidences lie below it, 39 within 0.75e-3 of it.  The gate guard re-evaluates exactly whatever the
    fast arithmetic leaves inside its band, so every CU's gated decision equals the reference's, except CUs whose reference confidence is within
    EXACT_NOISE / 2 + CONF_EPS = 1.2e-5 of the threshold: counted, at most 2 of 125 (the committed fixtures leave 0: the nearest is 1.45e-5 away).
    Same decisions with the selection as a launch of its own (guard_select_kernel carries the same test)."""
    pkg = gpu
    size = 128
    golden = load_golden(size)
    gate = float(np.float32(0.50015))
    excuse = EXACT_NOISE / 2 + CONF_EPS
    below = band = excused = 0
    for case in golden["cases"]:
        blob, org, pred, poc, qp, exp, exp_arg = materialise(pkg, golden, case)
        ref = pkg.decisions.from_logits(size, exp, min_confidence=gate)
        below += int((ref["confidence"] < gate).sum())
        band += int((np.abs(ref["confidence"] - gate) < 0.75e-3).sum())
        m = _ctx(pkg, size, blob)
        m.set_confidence_gate(size, gate)
        split, _ = m.predict_batch(org, pred, poc, qp)
        dec, _ = m.predict_batch_decisions(org, pred, poc, qp)
        m.close()
        assert np.array_equal(dec["split_mode"], split)
        for i in range(len(poc)):
            if abs(ref["confidence"][i] - gate) <= excuse:
                excused += 1
                continue
            assert split[i] == ref["split_mode"][i], (case["name"], i, int(split[i]), int(ref["split_mode"][i]), float(ref["confidence"][i]))
    assert (below, band) == (33, 39), (below, band)
    assert excused <= 2, excused
    print(f"gate {gate}: {below} reference confidences below, {band} inside the band, {excused} too close to the threshold to compare")


def test_gate_guard_matches_in_the_select_kernel_form(gpu, monkeypatch):
    """The gate guard rides on the heads kernel; guard_select_kernel (MLT_TUNING=1 MLT_GUARD_SELECT_KERNEL=1) carries the same test: same CUs re-run,
    same bits, on the near-tie family with the gate cutting through it."""
    pkg = gpu
    size = 128
    golden = load_golden(size)
    case = next(c for c in golden["cases"] if c["name"] == "near_tie")
    blob, org, pred, poc, qp, exp, _ = materialise(pkg, golden, case)
    gate = 0.50015
    fused = _ctx(pkg, size, blob)
    monkeypatch.setenv("MLT_TUNING", "1")
    monkeypatch.setenv("MLT_GUARD_SELECT_KERNEL", "1")
    plain = _ctx(pkg, size, blob)
    monkeypatch.delenv("MLT_GUARD_SELECT_KERNEL")
    for m in (fused, plain):
        m.set_confidence_gate(size, gate)
    r0 = [m.arithmetic(size)["guard_reruns"] for m in (fused, plain)]
    df, lf = fused.predict_batch_decisions(org, pred, poc, qp)
    dp, lp = plain.predict_batch_decisions(org, pred, poc, qp)
    r1 = [m.arithmetic(size)["guard_reruns"] for m in (fused, plain)]
    assert r1[0] - r0[0] == r1[1] - r0[1] > 0
    assert _same_records(df, dp) and np.array_equal(lf, lp)
    fused.close(); plain.close()


def test_gate_guard_reruns_a_cu_whose_confidence_sits_at_the_threshold(gpu):
    """The gate guard itself, not the decision guard: a CU of the plain fixtures with a wide reference margin (> 3 x LOGIT_TOL) and a reference confidence in
    (0.55, 0.95) that the shipped configuration does not re-run on its own (CU 0 of poc_qp_min, seed-10 weights: confidence 0.7683, margin 1.93).  As a batch
    of one and as a one-CU call: gate off -> no re-run; gate 1e-4 above its reference confidence (the fast confidence is then at most
    1e-4 + LOGIT_TOL / 2 = 6e-4 from the gate, inside the band 0.75 x tolerance) -> exactly one re-run, split -1, raw_mode the reference's argmax, logits
    within EXACT_NOISE of the fixture's; gate 2e-3 above (outside the band) -> no re-run, split still -1."""
    pkg = gpu
    size = 128
    golden = load_golden(size)
    case = next(c for c in golden["cases"] if c["name"] == "poc_qp_min")
    blob, org, pred, poc, qp, exp, exp_arg = materialise(pkg, golden, case)
    ref = pkg.decisions.from_logits(size, exp)
    conf = float(ref["confidence"][0])
    assert case["variant"] == "plain" and ref["margin"][0] > 3 * LOGIT_TOL and 0.55 < conf < 0.95
    m = _ctx(pkg, size, blob)
    a = m.arithmetic(size)
    assert a["exact"] != 1 and a["decision_guard"] == 1   # a non-exact tier behind the guards: what the gate guard exists for
    o1, p1, c1, q1 = org[:1], pred[:1], poc[:1], qp[:1]

    def run(batch):
        r0 = m.arithmetic(size)["guard_reruns"]
        if batch:
            dec, lg = m.predict_batch_decisions(o1, p1, c1, q1)
            dec, lg = dec[0], lg[0]
        else:
            dec, lg = m.predict_decision(org[0], pred[0], int(poc[0]), int(qp[0]))
        return dec, lg, m.arithmetic(size)["guard_reruns"] - r0

    for batch in (True, False):
        m.set_confidence_gate(size, 0.0)
        dec, lg_fast, grew = run(batch)
        assert grew == 0 and dec["split_mode"] == dec["raw_mode"] == ref["raw_mode"][0], (batch, grew)
        m.set_confidence_gate(size, conf + 1e-4)
        dec, lg, grew = run(batch)
        assert grew == 1, (batch, grew)
        assert dec["split_mode"] == -1 and dec["raw_mode"] == ref["raw_mode"][0], batch
        assert np.abs(lg - exp[0]).max() <= EXACT_NOISE, (batch, float(np.abs(lg - exp[0]).max()))
        assert abs(float(dec["confidence"]) - conf) <= EXACT_NOISE / 2 + CONF_EPS
        if batch:
            s, lg_s = m.predict_batch(o1, p1, c1, q1)   # the existing entry point is gated (and guarded) the same way
            assert s[0] == -1 and np.array_equal(lg_s[0], lg)
        m.set_confidence_gate(size, conf + 2e-3)
        dec, lg, grew = run(batch)
        assert grew == 0 and dec["split_mode"] == -1 and dec["raw_mode"] == ref["raw_mode"][0], (batch, grew)
        assert np.array_equal(lg, lg_fast)   # (no re-run: the fast arithmetic's logits)
    m.close()


def test_gate_errors_readback_graph_invalidation_calibrate_and_reload(gpu):
    pkg = gpu
    size = 128
    golden = load_golden(size)
    case = next(c for c in golden["cases"] if c["name"] == "out_of_range_pels")   # reference confidences 0.968, 0.953, 0.829, margins >= 1.6
    blob, org, pred, poc, qp, exp, _ = materialise(pkg, golden, case)
    ref = pkg.decisions.from_logits(size, exp)
    m = _ctx(pkg, size, blob)
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(pkg.MltError) as ei:
            m.set_confidence_gate(size, bad)
        assert ei.value.code == 1, bad          # MLT_ERR_ARG
    for call in (lambda: m.set_confidence_gate(64, 0.5), lambda: m.confidence_gate(64)):
        with pytest.raises(pkg.MltError) as ei:
            call()
        assert ei.value.code == 4               # MLT_ERR_SIZE_DISABLED
    with pytest.raises(pkg.MltError) as ei:
        m.set_confidence_gate(48, 0.5)
    assert ei.value.code == 1
    assert m.confidence_gate(size) == 0.0
    # a gate set after the one-CU graph was captured changes the next call's result
    i = int(np.argmin(ref["confidence"]))
    gate = float(np.float32(0.9))
    assert ref["confidence"][i] < 0.85 and (np.delete(ref["confidence"], i) > 0.95).all() and ref["margin"].min() > 1.0
    for _ in range(3):
        s0, l0 = m.predict(org[i], pred[i], int(poc[i]), int(qp[i]))
    assert s0 == ref["raw_mode"][i]
    m.set_confidence_gate(size, gate)
    s1, l1 = m.predict(org[i], pred[i], int(poc[i]), int(qp[i]))
    assert s1 == -1 and np.array_equal(l1, l0)
    # ... survives a re-calibration on the caller's content and a reload of the size
    want = pkg.decisions.from_logits(size, exp, min_confidence=gate)["split_mode"]
    assert (want == -1).any()
    m.calibrate(size, org, pred, poc, qp)
    assert m.confidence_gate(size) == gate
    assert np.array_equal(m.predict_batch(org, pred, poc, qp)[0], want)
    m.load_weights(size, blob)
    assert m.confidence_gate(size) == gate
    assert np.array_equal(m.predict_batch(org, pred, poc, qp)[0], want)
    assert m.predict(org[i], pred[i], int(poc[i]), int(qp[i]))[0] == -1
    m.set_confidence_gate(size, 0.0)
    assert m.predict(org[i], pred[i], int(poc[i]), int(qp[i]))[0] == s0 and np.array_equal(m.predict_batch(org, pred, poc, qp)[0], ref["raw_mode"])
    m.close()
    # every device context of a multi-device context carries the gate
    m2 = pkg.MltCnn(sizes=(size,), blobs={size: blob}, devices=[0, 0])
    m2.set_confidence_gate(size, gate)
    assert [m2.confidence_gate(size, k) for k in range(m2.num_devices())] == [gate, gate]
    assert np.array_equal(m2.predict_batch(org, pred, poc, qp)[0], want)
    tickets = [m2.submit(org[k], pred[k], int(poc[k]), int(qp[k])) for k in range(len(poc))]   # dealt round-robin over the two contexts
    assert [m2.wait_decision(size, t)[0]["split_mode"] for t in tickets] == want.tolist()
    m2.close()


def test_header_only_predictor_honours_min_conf(gpu, tmp_path):
    """host/mlt_split_predictor.hpp with MLTCNN_MIN_CONF=0.75 MLTCNN_STATS=1: predictSplitMode returns -1 exactly where the Python binding's gated split is
    -1 (and the binding's split elsewhere), a gated call prints no `error` line and does not count in failed=, gated= is that count; predictDecision
    returns the record the binding returns."""
    pkg = gpu
    size = 128
    golden = load_golden(size)
    cus = []
    blob = None
    for case in golden["cases"]:
        if case["weight_seed"] == 10 and case["variant"] == "plain":
            blob, org, pred, poc, qp, _, _ = materialise(pkg, golden, case)
            cus += [(org[i], pred[i], int(poc[i]), int(qp[i])) for i in range(len(poc))]
    (tmp_path / "MLTORPQ_splitMode_128.mltw").write_bytes(blob)
    with open(tmp_path / "cus.bin", "wb") as f:
        f.write(np.array([len(cus)], "<i4").tobytes())
        for o, p, c, q in cus:
            f.write(np.array([c, q], "<i4").tobytes() + o.astype("<i2").tobytes() + p.astype("<i2").tobytes())
    src = tmp_path / "gated_demo.cpp"
    src.write_text(r'''
#include <vector>
#include "mlt_split_predictor.hpp"
int main(int argc, char **argv) {
  mlt::SplitPredictor cnn(argv[1]);
  if (!cnn.ok()) return 2;
  FILE *f = std::fopen(argv[2], "rb");
  int32_t n = 0;
  if (!f || std::fread(&n, 4, 1, f) != 1) return 3;
  std::vector<mlt::Pel> org(128 * 128), pred(128 * 128);
  for (int i = 0; i < n; ++i) {
    int32_t pq[2];
    if (std::fread(pq, 4, 2, f) != 2 || std::fread(org.data(), 2, org.size(), f) != org.size() || std::fread(pred.data(), 2, pred.size(), f) != pred.size()) return 4;
    const int s = cnn.predictSplitMode(org.data(), 128, pred.data(), 128, 128, pq[0], pq[1]);
    mlt_decision d;
    const bool ok = cnn.predictDecision(org.data(), 128, pred.data(), 128, 128, pq[0], pq[1], &d);
    std::printf("cu %d split %d ok %d rec %d %d %.9g\n", i, s, (int)ok, d.split_mode, d.raw_mode, (double)d.confidence);
  }
  std::fclose(f);
  return 0;
}
''')
    exe = str(tmp_path / "gated_demo")
    lib_dir = os.path.dirname(pkg.build.LIB)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "host"), str(src), "-o", exe, "-L" + lib_dir, "-lmltcnn_hip", "-Wl,-rpath," + lib_dir])
    env = dict(os.environ, MLTCNN_MIN_CONF="0.75", MLTCNN_STATS="1")
    out = subprocess.run([exe, str(tmp_path), str(tmp_path / "cus.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    m = _ctx(pkg, size, blob)
    m.set_confidence_gate(size, 0.75)
    want = [m.predict_decision(o, p, c, q)[0] for o, p, c, q in cus]
    m.close()
    rows = [l.split() for l in out.stdout.splitlines() if l.startswith("cu ")]
    assert len(rows) == len(cus) > 20
    gated = 0
    for r, w in zip(rows, want):
        assert int(r[3]) == w["split_mode"] and int(r[5]) == 1 and int(r[7]) == w["split_mode"] and int(r[8]) == w["raw_mode"], (r, w)
        assert np.float32(float(r[9])) == w["confidence"], (r, w)
        gated += w["split_mode"] == -1
    assert 0 < gated < len(cus)
    assert not [l for l in out.stderr.splitlines() if l.strip() == "error"], out.stderr
    stats = [l for l in out.stderr.splitlines() if l.startswith("mltcnn-stats ")]
    assert len(stats) == 1
    kv = dict(t.split("=", 1) for t in stats[0].split()[1:])
    assert kv["failed"] == "0" and int(kv["gated"]) == 2 * gated and int(kv["predict_calls"]) == 2 * len(cus)   # (each CU went through predictSplitMode and predictDecision)
    # without the variable: no gate, no gated= token; a malformed value: a message, the gate stays off
    for extra, msg in (({}, False), ({"MLTCNN_MIN_CONF": "128:0.75,"}, True)):
        env2 = dict(os.environ, MLTCNN_STATS="1", **extra)
        out2 = subprocess.run([exe, str(tmp_path), str(tmp_path / "cus.bin")], capture_output=True, text=True, timeout=300, env=env2)
        assert out2.returncode == 0
        assert all(int(l.split()[3]) == w["raw_mode"] for l, w in zip([l for l in out2.stdout.splitlines() if l.startswith("cu ")], want))
        assert "gated=" not in out2.stderr and ("malformed" in out2.stderr) == msg
