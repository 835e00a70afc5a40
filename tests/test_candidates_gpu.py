"""GPU (MI355X): candidate split sets through the C ABI, against the committed reference fixtures (tests/golden/golden_{128,64,32,16}.json) and the
host restatement decisions.candidates_from_logits.  Shipped configuration (flags = 0) throughout.

Bounds (none of them taken from what the device returns):
  CONF_EPS = 2e-6     one device fp32 softmax probability against float64 on THE SAME logits (tests/test_decisions_gpu.py)
  CAND_EPS = K x that a prefix sum of up to K probabilities against float64 on the same logits
  EXACT_NOISE = 2e-5  |dlogit| of the exact arithmetic against the reference (tests/helpers.py)
A CU is UNDECIDABLE against the reference when a proper prefix sum of the reference lies within EXACT_NOISE / 2 + CAND_EPS of the coverage (logits
within EXACT_NOISE move a prefix sum by at most half of it) or classes are dropped over a reference logit gap <= 2 x EXACT_NOISE (the boundary pair may
swap).  Such CUs are counted, never skipped silently, and capped at 2 of 125 per size and head; every other CU's mask must equal the reference's:
the candidate guard re-runs exactly whatever the fast arithmetic (|dlogit| <= 1e-3, prefix sums within 5e-4) leaves within 0.75e-3 of the coverage or
with a boundary gap below the decision guard's margin."""
import os

import numpy as np
import pytest

from helpers import EXACT_NOISE, SIZES, load_golden, materialise

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3
CONF_EPS = 2e-6
UNDECIDABLE_CAP = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


def _classes(size):
    return [2, 3, 4] if size == 128 else [2, 3, 4, 6]


def _head(size, head):
    return (2 if size == 128 else 0) if head is None else head


def _ctx(pkg, size, blob, head=None, **kw):
    return pkg.MltCnn(device=0, sizes=(size,), blobs={size: blob}, head_index=None if head is None else {size: head}, **kw)


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _device_call(pkg, m, size, org, pred, poc, qp, kind):
    """The device-pointer entry: kind 'split' -> (split, logits); 'records' -> (records, logits); 'candidates' -> (candidates, records, logits)."""
    import torch
    dev = torch.device("cuda", 0)
    n, nl = len(poc), m.num_logits(size)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (org, pred, poc, qp)]
    d_lg = torch.zeros((n, nl), dtype=torch.float32, device=dev)
    d_split = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_dec = torch.zeros((n * 48,), dtype=torch.uint8, device=dev)
    d_cand = torch.zeros((n * 40,), dtype=torch.uint8, device=dev)
    m.predict_batch_device(n, size, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d_split.data_ptr() if kind == "split" else None,
                           d_lg.data_ptr(), d_decisions=None if kind == "split" else d_dec.data_ptr(), d_candidates=d_cand.data_ptr() if kind == "candidates" else None)
    m.synchronize()
    dec = np.frombuffer(d_dec.cpu().numpy().tobytes(), pkg.capi.DECISION_DTYPE).copy()
    if kind == "split":
        return d_split.cpu().numpy(), d_lg.cpu().numpy()
    if kind == "records":
        return dec, d_lg.cpu().numpy()
    return np.frombuffer(d_cand.cpu().numpy().tobytes(), pkg.capi.CANDIDATES_DTYPE).copy(), dec, d_lg.cpu().numpy()


def _undecidable(ref, coverage, K):
    """Per CU of the reference's restated records: too close to call whatever arithmetic produced the logits (module docstring)."""
    near = (np.abs(ref["cum"][:, :K - 1] - coverage) <= EXACT_NOISE / 2 + K * CONF_EPS).any(axis=1)
    return near | ((ref["count"] < K) & (ref["gap"] <= 2 * EXACT_NOISE))


def _check_describes_own_logits(pkg, size, head, cand, dec, logits, coverage, max_modes, what):
    """The device's record against candidates_from_logits of the logits the SAME call returned: rank and probabilities always; count and mask wherever no
    restated proper prefix sum lies within CAND_EPS of the coverage (fp32 against float64 may then fall on either side).  Returns (close CUs, worst |dprob|)."""
    K = _classes(size)[_head(size, head)]
    own = pkg.decisions.candidates_from_logits(size, logits, head_index=head, coverage=coverage, max_modes=max_modes)
    assert np.array_equal(cand["order"], own["order"]), what
    worst = float(np.abs(cand["prob"].astype(np.float64) - own["prob"]).max())
    assert worst <= CONF_EPS, (what, worst)
    assert (cand["prob"][:, K:] == 0).all() and (cand["order"][:, K:] == -1).all(), what
    assert np.array_equal(cand["count"], [bin(int(v)).count("1") for v in cand["mask"]]), what
    raw = dec["raw_mode"]
    assert np.array_equal(cand["order"][:, 0], raw), what
    assert np.array_equal(cand["prob"][np.arange(len(raw)), raw].view(np.uint32), dec["confidence"].view(np.uint32)), what   # bit-equal to the record's confidence
    close = (np.abs(own["cum"][:, :K - 1] - coverage) <= K * CONF_EPS).any(axis=1)
    assert np.array_equal(cand["mask"][~close], own["mask"][~close]) and np.array_equal(cand["count"][~close], own["count"][~close]), what
    return int(close.sum()), worst


CASES = [(s, None) for s in SIZES] + [(s, 3) for s in (64, 32, 16)]


@pytest.mark.parametrize("size,head", CASES, ids=[f"{s}-head{'default' if h is None else h}" for s, h in CASES])
def test_candidates_on_every_fixture_and_entry_point(gpu, size, head):
    """Policy (0.9, 0), every fixture case, every entry point (batch, device pointer, one CU per call, deferred, two device contexts on GPU 0): candidate
    records byte-equal across entry points; logits and decision records bit-equal to the existing twins called under the same policy; prob[raw_mode]
    bit-equal to the confidence; the record describes the returned logits; the mask equals the reference's for every CU that is not undecidable."""
    pkg = gpu
    golden = load_golden(size)
    coverage, max_modes = float(np.float32(0.9)), 0
    K = _classes(size)[_head(size, head)]
    undecidable = close = cus = 0
    worst = 0.0
    hist = np.zeros(K, int)
    for case in golden["cases"]:
        blob, org, pred, poc, qp, exp, _ = materialise(pkg, golden, case)
        what = f"{size}/{head}/{case['name']}"
        n = len(poc)
        m = _ctx(pkg, size, blob, head)
        assert m.candidate_policy(size) == (0.0, 0)
        m.set_candidate_policy(size, coverage, max_modes)
        assert m.candidate_policy(size) == (coverage, max_modes)
        split, logits = m.predict_batch(org, pred, poc, qp)
        dec, lg_d = m.predict_batch_decisions(org, pred, poc, qp)
        cand, dec_c, lg_c = m.predict_batch_candidates(org, pred, poc, qp)
        assert np.array_equal(lg_c.view(np.uint32), logits.view(np.uint32)) and np.array_equal(lg_d.view(np.uint32), logits.view(np.uint32)), what
        assert _same(dec_c, dec) and np.array_equal(dec["split_mode"], split), what
        only, no_dec, no_lg = m.predict_batch_candidates(org, pred, poc, qp, want_logits=False, want_decisions=False)
        assert no_dec is None and no_lg is None and _same(only, cand), what
        c, w = _check_describes_own_logits(pkg, size, head, cand, dec, logits, coverage, max_modes, what)
        close += c
        worst = max(worst, w)
        ref = pkg.decisions.candidates_from_logits(size, exp, head_index=head, coverage=coverage, max_modes=max_modes)
        und = _undecidable(ref, coverage, K)
        for i in range(n):
            if not und[i]:
                assert cand["mask"][i] == ref["mask"][i], (what, i, int(cand["mask"][i]), int(ref["mask"][i]), ref["cum"][i].tolist(), float(ref["gap"][i]))
        undecidable += int(und.sum())
        hist += np.bincount(cand["count"], minlength=K + 1)[1:]
        cus += n
        # device-pointer entries
        s_dev, l_dev = _device_call(pkg, m, size, org, pred, poc, qp, "split")
        c_dev, d_dev, l_dev2 = _device_call(pkg, m, size, org, pred, poc, qp, "candidates")
        assert np.array_equal(s_dev, split) and np.array_equal(l_dev, logits) and np.array_equal(l_dev2, logits) and _same(d_dev, dec) and _same(c_dev, cand), what
        # one CU per call, and the deferred pair
        tickets = [m.submit(org[i], pred[i], int(poc[i]), int(qp[i])) for i in range(n)]
        for i in range(n):
            s1, l1 = m.predict(org[i], pred[i], int(poc[i]), int(qp[i]))
            c1, d1, l1c = m.predict_candidates(org[i], pred[i], int(poc[i]), int(qp[i]))
            assert s1 == split[i] and np.array_equal(l1, logits[i]) and np.array_equal(l1c, l1) and _same(d1, dec[i]) and _same(c1, cand[i]), (what, i)
            s2, l2 = m.wait(size, tickets[i])
            c2, d2, l2c = m.wait_candidates(size, tickets[i])
            assert s2 == split[i] and np.array_equal(l2, logits[i]) and np.array_equal(l2c, l2) and _same(d2, dec[i]) and _same(c2, cand[i]), (what, i)
        m.close()
        # one context serving two device contexts (the same GPU twice): shards of the batch, same bits
        m2 = pkg.MltCnn(sizes=(size,), blobs={size: blob}, devices=[0, 0], head_index=None if head is None else {size: head})
        m2.set_candidate_policy(size, coverage, max_modes)
        s_2, l_2 = m2.predict_batch(org, pred, poc, qp)
        c_2, d_2, l_2c = m2.predict_batch_candidates(org, pred, poc, qp)
        assert np.array_equal(s_2, split) and np.array_equal(l_2, logits) and np.array_equal(l_2c, logits) and _same(d_2, dec) and _same(c_2, cand), what
        m2.close()
    print(size, head, f"policy ({coverage}, {max_modes}): kept-count histogram {hist.tolist()}, {undecidable} of {cus} CUs undecidable against the reference, "
          f"{close} within CAND_EPS of the coverage on their own logits, worst |dprob| {worst:.2e} (bound {CONF_EPS:.0e})")
    assert cus == 125 and undecidable <= UNDECIDABLE_CAP, (cus, undecidable)


@pytest.mark.parametrize("size", SIZES)
def test_default_policy_returns_the_argmax_and_changes_nothing(gpu, size):
    """No policy set: the candidate twins return mask = 1 << split, count 1; logits bit-equal to the plain call's; the guards re-run exactly as many CUs
    as for the plain call."""
    pkg = gpu
    golden = load_golden(size)
    for case in golden["cases"]:
        blob, org, pred, poc, qp, exp, _ = materialise(pkg, golden, case)
        what = f"{size}/{case['name']}"
        m = _ctx(pkg, size, blob)
        r0 = m.arithmetic(size)["guard_reruns"]
        split, logits = m.predict_batch(org, pred, poc, qp)
        r1 = m.arithmetic(size)["guard_reruns"]
        cand, dec, lg = m.predict_batch_candidates(org, pred, poc, qp)
        r2 = m.arithmetic(size)["guard_reruns"]
        assert r2 - r1 == r1 - r0, (what, r0, r1, r2)
        assert np.array_equal(lg.view(np.uint32), logits.view(np.uint32)) and np.array_equal(dec["split_mode"], split), what
        assert np.array_equal(cand["mask"], np.uint32(1) << split.astype(np.uint32)) and (cand["count"] == 1).all(), what
        assert np.array_equal(cand["order"][:, 0], split), what
        c1, d1, l1 = m.predict_candidates(org[0], pred[0], int(poc[0]), int(qp[0]))
        s1, l1p = m.predict(org[0], pred[0], int(poc[0]), int(qp[0]))
        assert _same(c1, cand[0]) and s1 == split[0] and np.array_equal(l1, l1p) and np.array_equal(l1, logits[0]), what
        t = m.submit(org[0], pred[0], int(poc[0]), int(qp[0]))
        c2, d2, l2 = m.wait_candidates(size, t)
        assert _same(c2, cand[0]) and _same(d2, dec[0]) and np.array_equal(l2, logits[0]), what
        m.close()


@pytest.mark.parametrize("size", SIZES)
def test_policy_with_cap_one_is_the_gate_as_a_mask(gpu, size):
    """Policy (0.75, 1): one class iff the SAME call's confidence >= float32(0.75), else all K -- exact, no tolerance (prob[raw_mode] is the confidence)."""
    pkg = gpu
    golden = load_golden(size)
    K = _classes(size)[_head(size, None)]
    one = full = 0
    for case in golden["cases"]:
        blob, org, pred, poc, qp, exp, _ = materialise(pkg, golden, case)
        m = _ctx(pkg, size, blob)
        m.set_candidate_policy(size, 0.75, 1)
        cand, dec, _ = m.predict_batch_candidates(org, pred, poc, qp)
        m.close()
        sure = dec["confidence"] >= np.float32(0.75)
        want = np.where(sure, np.uint32(1) << dec["raw_mode"].astype(np.uint32), np.uint32((1 << K) - 1))
        assert np.array_equal(cand["mask"], want) and np.array_equal(cand["count"], np.where(sure, 1, K)), (size, case["name"])
        assert np.array_equal(dec["split_mode"], dec["raw_mode"])   # the policy leaves the split alone
        one += int(sure.sum())
        full += int((~sure).sum())
    assert one > 0 and full > 0 and one + full == 125
    print(size, f"policy (0.75, 1): {one} CUs keep one class, {full} keep all {K}")


def test_coverage_through_the_near_tie_family(gpu, monkeypatch):
    """128 model, coverage float32(0.50015): in the reference 33 CUs keep two classes and 39 have a proper prefix sum within 0.75e-3 of the coverage.  The
    candidate guard re-evaluates exactly whatever the fast arithmetic leaves inside its band: every decidable mask equals the reference's, at most 2
    undecidable, guard_reruns grows; and the selection as a launch of its own (guard_select_kernel carries the same test) re-runs the same number of
    CUs and returns the same bits."""
    pkg = gpu
    size, K = 128, 4
    golden = load_golden(size)
    coverage = float(np.float32(0.50015))
    two = band = undecidable = grew = 0
    for case in golden["cases"]:
        blob, org, pred, poc, qp, exp, _ = materialise(pkg, golden, case)
        ref = pkg.decisions.candidates_from_logits(size, exp, coverage=coverage)
        two += int((ref["count"] == 2).sum())
        band += int((np.abs(ref["cum"][:, :K - 1] - coverage) < 0.75 * LOGIT_TOL).any(axis=1).sum())
        und = _undecidable(ref, coverage, K)
        fused = _ctx(pkg, size, blob)
        contexts = [fused]
        if case["variant"] == "near_tie":
            monkeypatch.setenv("MLT_TUNING", "1")
            monkeypatch.setenv("MLT_GUARD_SELECT_KERNEL", "1")
            contexts.append(_ctx(pkg, size, blob))
            monkeypatch.delenv("MLT_GUARD_SELECT_KERNEL")
            monkeypatch.delenv("MLT_TUNING")
        got = []
        for m in contexts:
            m.set_candidate_policy(size, coverage, 0)
            r0 = m.arithmetic(size)["guard_reruns"]
            cand, dec, lg = m.predict_batch_candidates(org, pred, poc, qp)
            got.append((cand, dec, lg, m.arithmetic(size)["guard_reruns"] - r0))
            m.close()
        cand = got[0][0]
        grew += got[0][3]
        if len(got) == 2:
            assert got[0][3] == got[1][3] > 0, (case["name"], got[0][3], got[1][3])
            assert _same(got[0][0], got[1][0]) and _same(got[0][1], got[1][1]) and np.array_equal(got[0][2].view(np.uint32), got[1][2].view(np.uint32)), case["name"]
        for i in range(len(poc)):
            if not und[i]:
                assert cand["mask"][i] == ref["mask"][i], (case["name"], i, int(cand["mask"][i]), int(ref["mask"][i]), ref["cum"][i].tolist())
        undecidable += int(und.sum())
    assert (two, band) == (33, 39), (two, band)
    assert undecidable <= UNDECIDABLE_CAP, undecidable
    assert grew > 0
    print(f"coverage {coverage}: {two} reference CUs keep two classes, {band} inside the band, {undecidable} undecidable, {grew} CUs re-run by the guards")


def test_candidate_guard_reruns_a_cu_whose_prefix_sits_at_the_coverage(gpu):
    """The candidate guard itself, not the decision guard: CU 0 of poc_qp_min (seed-10 weights: reference confidence 0.7683, margin 1.93, the next logit gap
    0.039 -- nothing the shipped configuration re-runs on its own).  As a batch of one and as a one-CU call: default policy -> no re-run; coverage 1e-4
    above the reference confidence (the fast prefix sum is then at most 1e-4 + LOGIT_TOL / 2 = 6e-4 away, inside the band) -> exactly one re-run, two
    classes kept as the reference says, logits within EXACT_NOISE of the fixture's, and the plain mlt_predict_batch under that policy returns those same
    logits; coverage 2e-3 above (outside the band) -> no re-run, the fast pass's logits come back."""
    pkg = gpu
    size = 128
    golden = load_golden(size)
    case = next(c for c in golden["cases"] if c["name"] == "poc_qp_min")
    blob, org, pred, poc, qp, exp, _ = materialise(pkg, golden, case)
    dref = pkg.decisions.from_logits(size, exp)
    conf = float(dref["confidence"][0])
    assert case["variant"] == "plain" and dref["margin"][0] > 3 * LOGIT_TOL and 0.55 < conf < 0.95
    m = _ctx(pkg, size, blob)
    a = m.arithmetic(size)
    assert a["exact"] != 1 and a["decision_guard"] == 1   # a non-exact tier behind the guards: what the candidate guard exists for
    o1, p1, c1, q1 = org[:1], pred[:1], poc[:1], qp[:1]

    def run(batch):
        r0 = m.arithmetic(size)["guard_reruns"]
        if batch:
            cand, dec, lg = m.predict_batch_candidates(o1, p1, c1, q1)
            cand, dec, lg = cand[0], dec[0], lg[0]
        else:
            cand, dec, lg = m.predict_candidates(org[0], pred[0], int(poc[0]), int(qp[0]))
        return cand, dec, lg, m.arithmetic(size)["guard_reruns"] - r0

    for batch in (True, False):
        m.set_candidate_policy(size, 0.0, 0)
        cand, dec, lg_fast, grew = run(batch)
        assert grew == 0 and cand["mask"] == 1 << int(dref["raw_mode"][0]) and cand["count"] == 1, (batch, grew)
        near = conf + 1e-4
        ref = pkg.decisions.candidates_from_logits(size, exp[:1], coverage=near)
        assert ref["count"][0] == 2 and ref["gap"][0] > 3 * LOGIT_TOL
        m.set_candidate_policy(size, near, 0)
        cand, dec, lg, grew = run(batch)
        assert grew == 1, (batch, grew)
        assert cand["count"] == 2 and cand["mask"] == ref["mask"][0] and cand["order"].tolist() == ref["order"][0].tolist(), batch
        assert np.abs(lg - exp[0]).max() <= EXACT_NOISE, (batch, float(np.abs(lg - exp[0]).max()))
        assert dec["split_mode"] == dec["raw_mode"] == dref["raw_mode"][0]
        if batch:
            r0 = m.arithmetic(size)["guard_reruns"]
            s, lg_s = m.predict_batch(o1, p1, c1, q1)   # the existing entry point is guarded the same way
            assert s[0] == dref["raw_mode"][0] and np.array_equal(lg_s[0].view(np.uint32), lg.view(np.uint32)) and m.arithmetic(size)["guard_reruns"] - r0 == 1
        far = conf + 2e-3
        ref = pkg.decisions.candidates_from_logits(size, exp[:1], coverage=far)
        m.set_candidate_policy(size, far, 0)
        cand, dec, lg, grew = run(batch)
        assert grew == 0 and cand["count"] == 2 and cand["mask"] == ref["mask"][0], (batch, grew)
        assert np.array_equal(lg.view(np.uint32), lg_fast.view(np.uint32))   # (no re-run: the fast arithmetic's logits)
    m.close()


def test_policy_errors_readback_graph_invalidation_calibrate_and_reload(gpu):
    pkg = gpu
    size = 128
    golden = load_golden(size)
    case = next(c for c in golden["cases"] if c["name"] == "out_of_range_pels")   # reference confidences 0.968, 0.953, 0.829, margins >= 1.6
    blob, org, pred, poc, qp, exp, _ = materialise(pkg, golden, case)
    dref = pkg.decisions.from_logits(size, exp)
    m = _ctx(pkg, size, blob)
    for bad in ((1.0, 0), (1.5, 0), (-0.1, 0), (float("nan"), 0), (0.9, -1), (0.9, 5)):   # the decision head of the 128 model has four classes
        with pytest.raises(pkg.MltError) as ei:
            m.set_candidate_policy(size, *bad)
        assert ei.value.code == 1, bad          # MLT_ERR_ARG
    m.set_candidate_policy(size, 0.9, 4)
    m.set_candidate_policy(size, 0.0, 0)
    for call in (lambda: m.set_candidate_policy(64, 0.5, 0), lambda: m.candidate_policy(64)):
        with pytest.raises(pkg.MltError) as ei:
            call()
        assert ei.value.code == 4               # MLT_ERR_SIZE_DISABLED
    with pytest.raises(pkg.MltError) as ei:
        m.set_candidate_policy(48, 0.5, 0)
    assert ei.value.code == 1
    assert m.candidate_policy(size) == (0.0, 0)
    # a policy set after the one-CU graph was captured changes the next call's record
    i = int(np.argmin(dref["confidence"]))
    cov = float(np.float32(0.9))
    assert dref["confidence"][i] < 0.85 and (np.delete(dref["confidence"], i) > 0.95).all()
    want = pkg.decisions.candidates_from_logits(size, exp, coverage=cov)
    assert want["count"][i] >= 2 and (np.delete(want["count"], i) == 1).all()
    assert (np.abs(want["cum"][:, :3] - cov) > 10 * LOGIT_TOL).all() and (want["gap"] > 10 * LOGIT_TOL).all()   # nothing near a boundary: the masks are the reference's
    for _ in range(3):
        c0, d0, l0 = m.predict_candidates(org[i], pred[i], int(poc[i]), int(qp[i]))
    assert c0["count"] == 1 and c0["mask"] == 1 << int(dref["raw_mode"][i])
    m.set_candidate_policy(size, cov, 0)
    c1, d1, l1 = m.predict_candidates(org[i], pred[i], int(poc[i]), int(qp[i]))
    assert c1["mask"] == want["mask"][i] and c1["count"] == want["count"][i] and np.array_equal(l1, l0) and _same(d1, d0)
    # ... survives a re-calibration on the caller's content and a reload of the size
    m.calibrate(size, org, pred, poc, qp)
    assert m.candidate_policy(size) == (cov, 0)
    assert np.array_equal(m.predict_batch_candidates(org, pred, poc, qp)[0]["mask"], want["mask"])
    m.load_weights(size, blob)
    assert m.candidate_policy(size) == (cov, 0)
    assert np.array_equal(m.predict_batch_candidates(org, pred, poc, qp)[0]["mask"], want["mask"])
    assert m.predict_candidates(org[i], pred[i], int(poc[i]), int(qp[i]))[0]["mask"] == want["mask"][i]
    m.set_candidate_policy(size, 0.0, 0)
    assert m.predict_candidates(org[i], pred[i], int(poc[i]), int(qp[i]))[0]["mask"] == 1 << int(dref["raw_mode"][i])
    m.close()
    # every device context of a multi-device context carries the policy
    m2 = pkg.MltCnn(sizes=(size,), blobs={size: blob}, devices=[0, 0])
    m2.set_candidate_policy(size, cov, 3)
    assert [m2.candidate_policy(size, k) for k in range(m2.num_devices())] == [(cov, 3), (cov, 3)]
    assert np.array_equal(m2.predict_batch_candidates(org, pred, poc, qp)[0]["mask"], want["mask"])
    tickets = [m2.submit(org[k], pred[k], int(poc[k]), int(qp[k])) for k in range(len(poc))]   # dealt round-robin over the two contexts
    assert [int(m2.wait_candidates(size, t)[0]["mask"]) for t in tickets] == want["mask"].tolist()
    m2.close()
