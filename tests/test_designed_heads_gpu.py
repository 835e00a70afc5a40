"""GPU (MI355X): heads_kernel / heads_cand_kernel / guard_select_kernel on DESIGNED logits (tests/designed_heads.py).

A head with zero feature columns returns logits that depend on (poc, qp, bias) alone and are predictable bit for bit, identical in the fast and the exact
arithmetic.  So every record field and every guard decision has ONE right answer, computed on the host from the predicted logits by the scalar restatement of
include/mltcnn.h in designed_heads.py:

  a  the returned logits of the designed head are designed_logits' bytes -- every size, every head, batch / device-pointer / one-CU / deferred entries,
     negative poc / qp and the |poc| >= 2^24 cases in which int -> float rounds
  b  the records -- heads_cand_kernel's through predict_batch_candidates, heads_kernel<true>'s through predict_batch_decisions -- on the whole case set (every weak order of K = 2, 3, 4 and 1561 of K = 6, 483 of them strict): level_mode, raw_mode, order, mask, count and
     margin EQUAL; confidences and probabilities within CONF_EPS = 2e-6 (the bound of tests/test_decisions_gpu.py: expf at <= 2 ulp, six terms, one division),
     equal in the exact-tie cases; prob[raw_mode] bit-equal to confidence.  count / mask / split_mode are derived from the RECORD's probabilities and confidence
     (fp32 prefix sums in rank order, one comparison), which reproduces the device's own sums to the bit: no CU is excused for lying near a coverage.
  c  the float-valued guards at their thresholds: top-2 margin T, T (1 - 2^-24), T + 2^-20, 0, large, NaN; the gate guard and the candidate guard (a) with the
     threshold exactly a band away from a confidence / prefix sum and one fp32 step inside; the candidate guard (b) with the dropped-class gap at T and one step
     below.  Observable as in tests/test_flat_guard_gpu.py: guard_reruns grows by exactly the restatement's count, and a CU's OTHER heads (seeded weights) carry
     the exact context's bytes iff it is flagged, the unguarded fast context's otherwise.
  d  a partition tree over a decision head with a NaN: tree_expand_kernel's own NaN scan writes cand_mask when no candidate records are asked for.

Two constraints shape part c.  (1) A k-way tie is a near-tie: the decision guard flags it whatever the gate or the coverage (a guard margin > 0 is what turns
the other two guards on), so ties cannot show the gate guard or the candidate guard (a).  Their two-sided cases use a CU with a wide margin and the confidence / probabilities THE DEVICE RETURNED for
it (confidence 1 / (1 + e^-1)); the one exactly known confidence away from a tie, 1.0, gives the lower side with hand-stated numbers.  (2) The one-step-below margin
is T - 2^-32 reached with poc = 1 on a slope of -2^-32 over a bias-free T x qp, not with poc = 2^24 - 1: at poc ~ 2^24 the seeded heads' logits are ~10^6 and
their fast and exact bytes coincide, which would blind the byte check.

Byte coincidence of the two reference contexts on the other heads (CUs that tell nothing), texture content (synth.make_patches_bulk), seed-13 weights, measured on
the MI355X: 0 of 1100 CUs at 128 x 128 for each of the three heads (cap: 2 % of a batch; the test prints and asserts it).

Wall time per test on one MI355X (40 tests, 17.6 s with the imports and the shared contexts): records of four classes 1.6 s, select kernel / chunks 1.4 s, records of
six classes 1.2 s, logit bytes 1.1 / 0.9 / 0.8 / 0.7 s (128 / 64 / 32 / 16), six classes on the guarded 64 model 0.8 s (guards) and 0.4 s (records), records of two and
three classes 0.6 s, ties and NaN rows 0.17 - 0.28 s per case, every other test 0.13 - 0.30 s per case."""
import time

import numpy as np
import pytest

import designed_heads as dh

pytestmark = pytest.mark.gpu
F = np.float32
SEED = 13
CONF_EPS = 2e-6
T, TOL = 2.0 ** -8, 2.0 ** -10
BAND = float(F(0.75) * F(TOL))
TREE_ALL = ("leaf_map", "logits", "decisions", "candidates")


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


def _up(x):
    return float(np.nextafter(F(x), F(2.0)))


def _down(x):
    return float(np.nextafter(F(x), F(-2.0)))


def _classes(size):
    return dh.HEAD_CLASSES[dh.arch_of(size)]


def _cols(size, head):
    lo = dh.head_offset(dh.arch_of(size), head)
    return slice(lo, lo + _classes(size)[head])


def _device_call(pkg, m, size, org, pred, poc, qp, kind):
    """The device-pointer entry: kind 'split' -> (split, logits); 'candidates' -> (candidates, records, logits)."""
    import torch
    dev = torch.device("cuda", 0)
    n, nl = len(poc), m.num_logits(size)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (org, pred, np.asarray(poc, np.int32), np.asarray(qp, np.int32))]
    d_lg = torch.zeros((n, nl), dtype=torch.float32, device=dev)
    d_split = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_dec = torch.zeros((n * 48,), dtype=torch.uint8, device=dev)
    d_cand = torch.zeros((n * 40,), dtype=torch.uint8, device=dev)
    m.predict_batch_device(n, size, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d_split.data_ptr() if kind == "split" else None,
                           d_lg.data_ptr(), d_decisions=None if kind == "split" else d_dec.data_ptr(), d_candidates=d_cand.data_ptr() if kind == "candidates" else None)
    m.synchronize()
    if kind == "split":
        return d_split.cpu().numpy(), d_lg.cpu().numpy()
    return (np.frombuffer(d_cand.cpu().numpy().tobytes(), pkg.capi.CANDIDATES_DTYPE).copy(), np.frombuffer(d_dec.cpu().numpy().tobytes(), pkg.capi.DECISION_DTYPE).copy(),
            d_lg.cpu().numpy())


def _same_logits(got, want):
    """Byte equality, a NaN for a NaN (its payload is the adder's business)."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---- a: logit bytes ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (128, 64, 32, 16))
def test_designed_logits_byte_for_byte_on_every_entry_point(gpu, size):
    pkg = gpu
    arch = dh.arch_of(size)
    n = len(dh.SCALARS)
    org, pred = pkg.synth.make_patches_bulk(size, n, 5)
    all_poc, all_qp = (np.array(v, np.int32) for v in zip(*dh.SCALARS))
    small = np.maximum(np.abs(all_poc.astype(np.int64)), np.abs(all_qp.astype(np.int64))) < dh.BIG
    assert (~small).sum() >= 4 and (all_poc < 0).any() and (all_qp < 0).any()
    m, loads = None, 0
    for head, K in enumerate(_classes(size)):
        for design in (dh.sixteenths, dh.one_sided):
            a, c, b = design(K, head)
            poc, qp = (all_poc, all_qp) if design is dh.one_sided else (np.where(small, all_poc, 7).astype(np.int32), np.where(small, all_qp, -9).astype(np.int32))
            blob = dh.designed_blob(arch, SEED, head, a, c, b)
            if m is None:
                m = pkg.MltCnn(device=0, sizes=(size,), blobs={size: blob}, flags=pkg.capi.FLAG_NO_CALIBRATION)
            else:
                m.load_weights(size, blob)
            loads += 1
            want = dh.designed_logits(a, c, b, poc, qp).tobytes()
            sl = _cols(size, head)
            what = (size, head, design.__name__)
            assert m.predict_batch(org, pred, poc, qp)[1][:, sl].tobytes() == want, what
            assert _device_call(pkg, m, size, org, pred, poc, qp, "split")[1][:, sl].tobytes() == want, what
            tickets = [m.submit(org[i], pred[i], int(poc[i]), int(qp[i])) for i in range(n)]
            one = np.stack([m.predict(org[i], pred[i], int(poc[i]), int(qp[i]))[1] for i in range(n)])
            assert one[:, sl].tobytes() == want, what
            assert np.stack([m.wait(size, t)[1] for t in tickets])[:, sl].tobytes() == want, what
    m.close()
    print(f"{size}: {loads} loads")


# ---- b: records ------------------------------------------------------------------------------------------------------------------------------------------------
def _multi_designs(size, i):
    """Blob i of the case set: every head of the model carries design i (modulo the number of designs of its K)."""
    out = {}
    for head, K in enumerate(_classes(size)):
        cs = dh.case_set(K)
        out[head] = cs[i % len(cs)]
    return {h: d for h, (d, _) in out.items()}, {h: reps for h, (_, reps) in out.items()}


def _scalars_of(reps_by_head, heads):
    seen = {}
    for h in heads:
        for _, p, q in reps_by_head[h]:
            seen[(p, q)] = None
    pq = np.array(list(seen), np.int32).reshape(-1, 2)
    return pq[:, 0].copy(), pq[:, 1].copy()


def _same_f32(x, y):
    return np.asarray(x, F).tobytes() == np.asarray(y, F).tobytes() or (np.isnan(x) and np.isnan(y))


def _check_records(what, size, head, designs, poc, qp, cand, dec, logits, gate, coverage, max_modes, exact=False, levels=True):
    """Every CU's records against the scalar restatement of the PREDICTED logits.  -> worst |dconfidence|, |dprob|."""
    classes = _classes(size)
    n = len(poc)
    L = {}
    for h, (a, c, b) in designs.items():
        L[h] = dh.designed_logits(a, c, b, poc, qp)
        assert _same_logits(logits[:, _cols(size, h)], L[h]), (what, "logits of head", h)
    K = classes[head]
    worst = 0.0
    eps = 0.0 if exact else CONF_EPS
    for i in range(n):
        for h in (designs if levels else ()):
            d = dh.decide(L[h][i])
            if d["raw_mode"] is None:
                assert np.isnan(dec["level_conf"][i, h]), (what, i, h)
                continue
            assert dec["level_mode"][i, h] == d["raw_mode"], (what, i, h, L[h][i], int(dec["level_mode"][i, h]), d["raw_mode"])
            err = abs(float(dec["level_conf"][i, h]) - float(d["confidence"]))
            worst = max(worst, err)
            assert err <= eps, (what, i, h, err)
        l = L[head][i]
        d = dh.decide(l)
        conf = dec["confidence"][i]
        assert d["raw_mode"] is None or _same_f32(dec["margin"][i], d["margin"]), (what, i, l, dec["margin"][i], d["margin"])     # (defined for finite logits)
        assert _same_f32(conf, dec["level_conf"][i, head])
        if d["raw_mode"] is None:
            assert np.isnan(conf) and (gate == 0 or dec["split_mode"][i] == -1), (what, i)
        else:
            assert dec["raw_mode"][i] == d["raw_mode"] == dec["level_mode"][i, head], (what, i, l)
            assert dec["split_mode"][i] == (d["raw_mode"] if gate == 0 or conf >= F(gate) else -1), (what, i, l, conf, gate)   # the record's confidence, one comparison
            if exact:
                assert dh.decide(l, gate)["split_mode"] == dec["split_mode"][i]
        if cand is None:
            continue
        c = dh.candidates(l, coverage, max_modes)
        assert list(cand["order"][i]) == c["order"] + [-1] * (8 - K), (what, i, l, cand["order"][i], c["order"])
        assert (cand["prob"][i, K:] == 0).all()
        if c["nan"]:
            assert cand["count"][i] == K and cand["mask"][i] == (1 << K) - 1 and np.isnan(cand["prob"][i, :K]).any(), (what, i)
            continue
        perr = float(np.abs(cand["prob"][i, :K].astype(np.float64) - np.array(c["prob"], np.float64)).max())
        worst = max(worst, perr)
        assert perr <= eps, (what, i, perr)
        assert cand["prob"][i, d["raw_mode"]].tobytes() == conf.tobytes(), (what, i)
        own = dh.candidates(l, coverage, max_modes, prob=cand["prob"][i])     # the device's own prefix sums, to the bit
        assert cand["count"][i] == own["count"] and cand["mask"][i] == own["mask"] and bin(int(cand["mask"][i])).count("1") == own["count"], (what, i, l, cand[i], own)
        if exact or all(abs(float(v) - coverage) > K * CONF_EPS for v in c["cum"][:K - 1]):
            assert (c["count"], c["mask"]) == (own["count"], own["mask"]), (what, i)
        if (coverage, max_modes) == (0.0, 0):
            assert cand["mask"][i] == 1 << d["raw_mode"] and cand["count"][i] == 1
    return worst


DEC_GATES = (0.0, 0.6)     # predict_batch_decisions: ungated and gated
POLICIES = [(0.0, 0.0, 0), (0.0, 0.9, 0), (0.0, 0.9, 2), (0.6, 0.6, 1)]     # (gate, coverage, max_modes); the last: (t, 1) against the gate at t


def _run_case_set(pkg, m, size, head, blobs, org, pred, what, first_loaded=None):
    t0 = time.time()
    worst, cus, loads = 0.0, 0, 0
    for i in blobs:
        designs, reps = _multi_designs(size, i)
        if i != first_loaded:
            m.load_weights(size, dh.designed_blob_multi(dh.arch_of(size), SEED, designs))
            loads += 1
        poc, qp = _scalars_of(reps, [head] if size != 16 else list(designs))
        n = len(poc)
        assert n <= len(org)
        cus += n
        m.set_candidate_policy(size, 0.0, 0)
        for gate in DEC_GATES:     # no candidate buffer, no policy: heads_kernel<true>, not heads_cand_kernel
            m.set_confidence_gate(size, gate)
            dec, lg = m.predict_batch_decisions(org[:n], pred[:n], poc, qp)
            worst = max(worst, _check_records(f"{what} blob {i} decisions alone, gate {gate}", size, head, designs, poc, qp, None, dec, lg, gate, 0.0, 0))
        for gate, cov, mm in POLICIES:
            m.set_confidence_gate(size, gate)
            m.set_candidate_policy(size, cov, mm)
            cand, dec, lg = m.predict_batch_candidates(org[:n], pred[:n], poc, qp)
            worst = max(worst, _check_records(f"{what} blob {i} policy {(gate, cov, mm)}", size, head, designs, poc, qp, cand, dec, lg, gate, cov, mm,
                                              levels=(gate, cov, mm) == POLICIES[0]))
            if (gate, cov, mm) == POLICIES[-1]:   # (t, 1) is the gate restated as a mask
                K = _classes(size)[head]
                assert np.array_equal(cand["mask"], np.where(dec["split_mode"] >= 0, np.uint32(1) << dec["raw_mode"].astype(np.uint32), np.uint32((1 << K) - 1)))
    m.set_confidence_gate(size, 0.0)
    m.set_candidate_policy(size, 0.0, 0)
    print(f"{what}: {cus} CUs x ({len(DEC_GATES)} decision calls + {len(POLICIES)} policies), {loads} loads, worst |dconf|, |dprob| {worst:.2e} (bound {CONF_EPS:.0e}), {time.time() - t0:.1f} s")


def _first_blob(size, i=0):
    return dh.designed_blob_multi(dh.arch_of(size), SEED, _multi_designs(size, i)[0])


@pytest.fixture(scope="module")
def small_content(gpu):
    return gpu.synth.make_patches_bulk(16, 400, 6)


def test_records_of_six_classes_on_every_reached_order(gpu, small_content):
    """16 x 16, exact configuration, head_index 3: eight blobs whose four heads are all designed -- level_mode / level_conf of K = 2, 3, 4 on their full sets, and
    the K = 6 records on 1561 weak orders."""
    pkg = gpu
    m = pkg.MltCnn(device=0, sizes=(16,), blobs={16: _first_blob(16)}, head_index={16: 3}, flags=pkg.capi.FLAG_NO_CALIBRATION)
    assert m.arithmetic(16)["exact"] == 1
    _run_case_set(pkg, m, 16, 3, range(len(dh.DESIGNS[6])), *small_content, "16 / head 3 / exact", first_loaded=0)
    m.close()


def test_records_of_four_classes_small_and_large_model(gpu, small_content):
    """K = 4 through head_index 2 of the 16 x 16 model, and through the 128 model's default head on an exact and on a guarded context."""
    pkg = gpu
    Fl = pkg.capi
    m = pkg.MltCnn(device=0, sizes=(16,), blobs={16: _first_blob(16)}, head_index={16: 2}, flags=Fl.FLAG_NO_CALIBRATION)
    _run_case_set(pkg, m, 16, 2, range(len(dh.DESIGNS[4])), *small_content, "16 / head 2 / exact", first_loaded=0)
    m.close()
    big = pkg.synth.make_patches_bulk(128, 64, 7)
    for name, flags in (("exact", Fl.FLAG_EXACT_128), ("guarded", Fl.FLAG_NO_CALIBRATION)):
        m = pkg.MltCnn(device=0, sizes=(128,), blobs={128: _first_blob(128)}, flags=flags)
        a = m.arithmetic(128)
        assert (a["exact"], a["decision_guard"]) == ((1, 0) if name == "exact" else (0, 1)), a
        _run_case_set(pkg, m, 128, 2, range(len(dh.DESIGNS[4])), *big, f"128 / default head / {name}", first_loaded=0)
        m.close()


def test_records_of_two_and_three_classes_as_decision_heads(gpu, small_content):
    pkg = gpu
    for head in (0, 1):
        m = pkg.MltCnn(device=0, sizes=(16,), blobs={16: _first_blob(16)}, head_index={16: head}, flags=pkg.capi.FLAG_NO_CALIBRATION)
        _run_case_set(pkg, m, 16, head, range(2), *small_content, f"16 / head {head} / exact", first_loaded=0)
        m.close()


def test_records_of_six_classes_on_a_guarded_small_model(gpu):
    """64 x 64 in the shipped configuration: calibrated into a mixed tier with a single-pass prefix (exact == 4), all guards on; two of the K = 6 blobs."""
    pkg = gpu
    org, pred = pkg.synth.make_patches_bulk(64, 280, 8)
    m = pkg.MltCnn(device=0, sizes=(64,), blobs={64: _first_blob(64)}, head_index={64: 3})
    a = m.arithmetic(64)
    assert a["exact"] == 4 and a["decision_guard"] == 1 and a["flat_guard"] == 1, a
    r0 = a["guard_reruns"]
    _run_case_set(pkg, m, 64, 3, (0, 2), org, pred, "64 / head 3 / guarded", first_loaded=0)
    assert m.arithmetic(64)["exact"] == 4 and m.arithmetic(64)["guard_reruns"] > r0     # (the tie orders are near-ties: re-run, same records)
    m.close()


TIES = {2: ([0, 0], 2, 0), 3: ([-200, 0, 0], 2, 1), 4: ([0, 0, 0, 0], 4, 0), 6: ([-200, 0, 0, 0, 0, -200], 4, 1)}    # K: (bias, m tied classes, the first of them)


def _const_designs(size, table):
    return {h: (np.zeros(K, F), np.zeros(K, F), np.array(table[K], F)) for h, K in enumerate(_classes(size))}


@pytest.mark.parametrize("size,head,flags", [(16, 0, "exact"), (16, 1, "exact"), (16, 2, "exact"), (16, 3, "exact"), (128, 0, "guarded"), (128, 2, "guarded"), (128, 2, "exact"),
                                             (64, 3, "shipped")])
def test_exact_ties_and_nan_rows(gpu, size, head, flags):
    """m = 2 or 4 classes tied at the top, the rest 200 below: every probability and prefix sum is exact, so every field must be EQUAL.  coverage j / m keeps j
    classes, the next float32 j + 1; the gate at the confidence keeps the split, one float32 step above withholds it.  Then a NaN bias in class 1 of every head:
    all K classes kept, order in class order, confidence NaN, any gate withholds the split."""
    pkg = gpu
    Fl = pkg.capi
    designs = _const_designs(size, {K: v[0] for K, v in TIES.items()})
    blob = dh.designed_blob_multi(dh.arch_of(size), SEED, designs)
    m = pkg.MltCnn(device=0, sizes=(size,), blobs={size: blob}, head_index={size: head},
                   flags={"exact": Fl.FLAG_EXACT_128 | Fl.FLAG_NO_CALIBRATION, "guarded": Fl.FLAG_NO_CALIBRATION, "shipped": 0}[flags])
    a = m.arithmetic(size)
    assert (a["exact"] == 1 and a["decision_guard"] == 0) if flags == "exact" else (a["exact"] in (0, 4) and a["decision_guard"] == 1), a
    K = _classes(size)[head]
    _, mt, first = TIES[K]
    n = 5
    org, pred = pkg.synth.make_patches_bulk(size, n, 9)
    poc, qp = np.arange(n, dtype=np.int32) - 2, np.arange(n, dtype=np.int32) * 7
    conf = 1.0 / mt
    r0 = a["guard_reruns"]

    def decisions_alone(what, designs, gate):
        """The same CUs through predict_batch_decisions with no candidate policy: heads_kernel<true>'s records (heads_cand_kernel writes the ones above)."""
        dec, lg = m.predict_batch_decisions(org, pred, poc, qp)
        _check_records(f"{what}, decisions alone", size, head, designs, poc, qp, None, dec, lg, gate, 0.0, 0, exact=True)
        one = m.predict_decision(org[0], pred[0], int(poc[0]), int(qp[0]))[0]
        for f in ("split_mode", "raw_mode", "confidence", "margin", "level_mode", "level_conf"):
            assert np.asarray(one[f]).tobytes() == np.asarray(dec[f][0]).tobytes() or np.isnan(one[f]).any(), (what, f, one[f], dec[f][0])
        return dec
    for j in range(1, mt):
        for cov, keep in ((j / mt, j), (_up(j / mt), j + 1)):
            for mm in (0, j):
                m.set_candidate_policy(size, cov, mm)
                cand, dec, lg = m.predict_batch_candidates(org, pred, poc, qp)
                _check_records(f"ties {size}/{head} coverage {cov!r} cap {mm}", size, head, designs, poc, qp, cand, dec, lg, 0.0, cov, mm, exact=True)
                kept = K if mm and keep > mm else keep
                want_mask = (1 << K) - 1 if kept == K else sum(1 << (first + t) for t in range(kept))
                assert (cand["count"] == kept).all() and (cand["mask"] == want_mask).all(), (cov, mm, cand[0])     # stated by hand: the lower classes first
                assert (dec["confidence"] == F(conf)).all() and (dec["margin"] == 0).all() and (dec["raw_mode"] == first).all()
    m.set_candidate_policy(size, 0.0, 0)
    for gate, split in ((conf, first), (_up(conf), -1), (_down(conf), first)):
        m.set_confidence_gate(size, gate)
        cand, dec, lg = m.predict_batch_candidates(org, pred, poc, qp)
        _check_records(f"ties {size}/{head} gate {gate!r}", size, head, designs, poc, qp, cand, dec, lg, gate, 0.0, 0, exact=True)
        assert (dec["split_mode"] == split).all() and (m.predict_batch(org, pred, poc, qp)[0] == split).all(), (gate, dec["split_mode"])
        d2 = decisions_alone(f"ties {size}/{head} gate {gate!r}", designs, gate)
        assert (d2["split_mode"] == split).all() and (d2["confidence"] == F(conf)).all() and (d2["margin"] == 0).all() and (d2["raw_mode"] == first).all(), (gate, d2[0])
        assert m.predict(org[0], pred[0], int(poc[0]), int(qp[0]))[0] == split
    if flags != "exact":
        assert m.arithmetic(size)["guard_reruns"] > r0      # a tie is a near-tie: these CUs went through the exact re-run and kept their records
    if flags == "shipped":     # (a calibration has nothing to measure on NaN logits: the NaN rows run on the configurations above)
        m.close()
        return
    # NaN rows
    nan_bias = {K: [float(-k) if k != 1 else np.nan for k in range(K)] for K in (2, 3, 4, 6)}
    designs = _const_designs(size, nan_bias)
    m.load_weights(size, dh.designed_blob_multi(dh.arch_of(size), SEED, designs))
    for gate, cov, mm in ((0.0, 0.0, 0), (0.5, 0.9, 2), (0.0, 0.9, 0)):
        m.set_confidence_gate(size, gate)
        m.set_candidate_policy(size, cov, mm)
        cand, dec, lg = m.predict_batch_candidates(org, pred, poc, qp)
        _check_records(f"NaN {size}/{head} policy {(gate, cov, mm)}", size, head, designs, poc, qp, cand, dec, lg, gate, cov, mm, exact=True)
        assert (cand["count"] == K).all() and (cand["mask"] == (1 << K) - 1).all() and (cand["order"][:, :K] == np.arange(K)).all()
        assert np.isnan(dec["confidence"]).all()
        if gate > 0:
            assert (dec["split_mode"] == -1).all() and (m.predict_batch(org, pred, poc, qp)[0] == -1).all()
        if (cov, mm) != (0.0, 0):
            m.set_candidate_policy(size, 0.0, 0)
        d2 = decisions_alone(f"NaN {size}/{head} gate {gate}", designs, gate)
        assert np.isnan(d2["confidence"]).all() and (gate == 0 or (d2["split_mode"] == -1).all())
    m.close()


# ---- c: guard selection at its thresholds ----------------------------------------------------------------------------------------------------------------------
N_BIG = 1100


class Refs:
    """Texture content and, per (poc, qp) assignment, the logits of the plain seed-13 blob on an exact and on an unguarded fast context: what a CU's OTHER heads
    return when it was / was not re-run (the designed blobs differ from the plain one in the designed head's rows only)."""

    def __init__(self, pkg, size, n, exact_flags, fast_flags, blob=None, **kw):
        self.pkg, self.size, self.n = pkg, size, n
        self.org, self.pred = pkg.synth.make_patches_bulk(size, n, 77)
        plain = blob or pkg.weights.synthetic_blob(dh.arch_of(size), SEED)
        self.ex = pkg.MltCnn(device=0, sizes=(size,), blobs={size: plain}, flags=exact_flags, **kw)
        self.fa = pkg.MltCnn(device=0, sizes=(size,), blobs={size: plain}, flags=fast_flags, **kw)
        self.cache, self.dev, self.shares = {}, None, []

    def close(self):
        self.ex.close(); self.fa.close()

    def reload(self, blob):
        """Another blob with the same other heads (a calibrated size decides its tier per blob: the references follow the context under test)."""
        self.ex.load_weights(self.size, blob); self.fa.load_weights(self.size, blob)
        self.cache = {}

    def of(self, poc, qp):
        key = (poc.tobytes(), qp.tobytes())
        if key not in self.cache:
            n = len(poc)
            self.cache[key] = (self.ex.predict_batch(self.org[:n], self.pred[:n], poc, qp)[1], self.fa.predict_batch(self.org[:n], self.pred[:n], poc, qp)[1])
        return self.cache[key]

    def device_planes(self):
        import torch
        if self.dev is None:
            self.dev = tuple(torch.from_numpy(a).to(torch.device("cuda", 0)) for a in (self.org, self.pred))
        return self.dev


def _reruns(m, size):
    return m.arithmetic(size)["guard_reruns"]


def _run(refs, m, form, poc, qp):
    """n = len(poc) CUs (the first n of the content) through one entry -> (logits [n, nl], growth of guard_reruns)."""
    import torch
    size, n = refs.size, len(poc)
    r0 = _reruns(m, size)
    if form == "host":
        lg = m.predict_batch(refs.org[:n], refs.pred[:n], poc, qp)[1]
    elif form == "records":
        lg = m.predict_batch_candidates(refs.org[:n], refs.pred[:n], poc, qp)[2]
    elif form == "device":
        o, p = refs.device_planes()
        dev = o.device
        d_poc, d_qp = torch.from_numpy(poc).to(dev), torch.from_numpy(qp).to(dev)
        d_split = torch.full((n,), -7, dtype=torch.int32, device=dev)
        d_lg = torch.zeros((n, m.num_logits(size)), dtype=torch.float32, device=dev)
        m.predict_batch_device(n, size, o.data_ptr(), p.data_ptr(), d_poc.data_ptr(), d_qp.data_ptr(), d_split.data_ptr(), d_lg.data_ptr())
        m.synchronize()
        lg = d_lg.cpu().numpy()
    elif form == "deferred":
        rows = []
        for lo in range(0, n, 48):
            tk = [m.submit(refs.org[i], refs.pred[i], int(poc[i]), int(qp[i])) for i in range(lo, min(lo + 48, n))]
            m.flush(size)
            rows += [m.wait(size, t)[1] for t in tk]
        lg = np.stack(rows)
    else:
        assert form == "single"
        rows, each = [], []
        for i in range(n):
            before = _reruns(m, size)
            rows.append(m.predict(refs.org[i], refs.pred[i], int(poc[i]), int(qp[i]))[1])
            each.append(_reruns(m, size) - before)
        return np.stack(rows), np.array(each)
    return lg, _reruns(m, size) - r0


def _flags_of(design, poc, qp, policy, conf_of=None, prob_of=None):
    """The restatement per CU (computed once per distinct (poc, qp))."""
    l = dh.designed_logits(*design, poc, qp)
    memo, out = {}, np.zeros(len(poc), bool)
    for i, key in enumerate(zip(poc.tolist(), qp.tolist())):
        if key not in memo:
            memo[key] = dh.guard_flags(l[i], T, TOL, confidence=None if conf_of is None else conf_of[key], prob=None if prob_of is None else prob_of[key], **policy)["any"]
        out[i] = memo[key]
    return l, out


def _check(refs, m, head, design, form, poc, qp, policy=None, what="", conf_of=None, prob_of=None):
    size = refs.size
    l, want = _flags_of(design, poc, qp, policy or {}, conf_of, prob_of)
    lg, grew = _run(refs, m, form, poc, qp)
    what = f"{what} [{form}, n = {len(poc)}, head {head}, {int(want.sum())} flagged]"
    sl = _cols(size, head)
    assert _same_logits(lg[:, sl], l), what + ": designed logits"
    other = np.ones(lg.shape[1], bool)
    other[sl] = False
    le, lf = refs.of(poc, qp)
    le, lf, got = le[:, other].view(np.uint32), lf[:, other].view(np.uint32), np.ascontiguousarray(lg[:, other]).view(np.uint32)
    blind = (le == lf).all(axis=1)
    refs.shares.append(float(blind.mean()))
    assert blind.sum() <= 0.02 * len(poc), f"{what}: {int(blind.sum())} CUs whose exact and fast bytes coincide"
    is_ex, is_fa = (got == le).all(axis=1), (got == lf).all(axis=1)
    bad = np.flatnonzero(~blind & ((is_ex != want) | (is_fa == want)))
    for i in bad[:12]:
        print(f"{what}: CU {i} (poc {poc[i]}, qp {qp[i]}, logits {l[i]}): expected {'the exact re-run' if want[i] else 'the fast result'}, "
              f"bytes are {'exact' if is_ex[i] else 'fast' if is_fa[i] else 'neither'}")
    assert bad.size == 0, f"{what}: {bad.size} CUs on the wrong side of the guard"
    assert (is_ex | is_fa)[blind].all()
    if form == "single":     # every call on its own count
        assert grew.tolist() == want.astype(int).tolist(), f"{what}: re-runs per call {grew.tolist()}, the restatement flags {want.astype(int).tolist()}"
    else:
        assert grew == int(want.sum()), f"{what}: {grew} re-runs, the restatement flags {int(want.sum())}"
    return want


def _placements(cases, flagged, n):
    """(poc, qp) assignments of n CUs: the flagged cases first, last, in a run across index 511 / 512, everywhere, nowhere, and all cases in turn."""
    fl = [k for k in cases if flagged[k]]
    un = [k for k in cases if not flagged[k]]
    assert fl and un, (fl, un)

    def build(is_flagged):
        names = [(fl[i % len(fl)] if f else un[i % len(un)]) for i, f in enumerate(is_flagged)]
        return np.array([cases[k][0] for k in names], np.int32), np.array([cases[k][1] for k in names], np.int32)
    idx = np.arange(n)
    keys = list(cases)
    return {"first": build(idx < 37), "last": build(idx >= n - 41), "run": build((idx >= 500) & (idx < 524)), "all": build(idx >= 0), "none": build(idx < 0),
            "mixed": (np.array([cases[keys[i % len(keys)]][0] for i in idx], np.int32), np.array([cases[keys[i % len(keys)]][1] for i in idx], np.int32))}


GUARD_HEADS = {0: (1, 0), 1: (2, 0), 2: (3, 1)}        # decision head -> the classes (p, q) that carry the top two logits
GAP_HEADS = {1: (2, 0, 1), 2: (1, 3, 0)}               # ... (p, q, r) of the gap family


@pytest.fixture(scope="module")
def big(gpu):
    pkg = gpu
    Fl = pkg.capi
    refs = Refs(pkg, 128, N_BIG, Fl.FLAG_EXACT_128, Fl.FLAG_NO_CALIBRATION | Fl.FLAG_NO_DECISION_GUARD | Fl.FLAG_NO_FLAT_GUARD)
    assert refs.ex.arithmetic(128)["exact"] == 1 and refs.fa.arithmetic(128)["exact"] == 0 and refs.fa.arithmetic(128)["decision_guard"] == 0
    made = {}

    def guarded(head, design, env=None):
        """The context under test for a decision head (one per head and environment), with the design loaded."""
        blob = dh.designed_blob(0, SEED, head, *design)
        key = (head, env)
        if key not in made:
            made[key] = pkg.MltCnn(device=0, sizes=(128,), blobs={128: blob}, head_index={128: head}, flags=Fl.FLAG_NO_CALIBRATION | Fl.FLAG_NO_FLAT_GUARD,
                                   tolerance=TOL, guard_margin=T)
            a = made[key].arithmetic(128)
            assert a["guard_margin"] == T and a["decision_guard"] == 1 and a["flat_guard"] == 0 and a["exact"] == 0 and a["mag_guard_kind"] == 0 and a["mag_guard_thr"] == 0, a
        else:
            made[key].load_weights(128, blob)
        m = made[key]
        m.set_confidence_gate(128, 0.0)
        m.set_candidate_policy(128, 0.0, 0)
        return m
    yield refs, guarded
    share = max(refs.shares) if refs.shares else 0.0
    print(f"byte coincidence of the exact and the fast reference on the other heads: worst share {share:.4f} over {len(refs.shares)} calls (cap 0.02)")
    for m in made.values():
        m.close()
    refs.close()


@pytest.mark.parametrize("head", (0, 1, 2))
def test_decision_guard_on_its_threshold_in_the_batch_tail(big, head):
    """!(t1 - t2 >= margin) in the heads kernel's tail for batches: margins T (kept), one step below (re-run), T + 2^-20, 0, large, both classes on top; 600 and 1100
    CUs with the flagged ones first, last, across 511 / 512, all, none; batch, device-pointer, record and deferred entries."""
    refs, guarded = big
    K = dh.HEAD_CLASSES[0][head]
    design, cases = dh.margin_family(K, T, *GUARD_HEADS[head])
    m = guarded(head, design)
    flagged = {k: dh.guard_flags(dh.designed_logits(*design, [v[0]], [v[1]])[0], T, TOL)["any"] for k, v in cases.items()}
    assert {k for k, f in flagged.items() if f} == {"T-", "zero", "T- other way"}
    for n in (600, N_BIG):
        pl = _placements(cases, flagged, n)
        for name in ("first", "last", "run", "all", "none", "mixed"):
            for form in (("host", "device") if name in ("run", "mixed") else ("device",) if n == 600 else ("host",)):
                want = _check(refs, m, head, design, form, *pl[name], what=f"margin family, {name}")
                assert want.sum() == {"first": 37, "last": 41, "run": 24, "all": n, "none": 0}.get(name, want.sum())
    pl = _placements(cases, flagged, 130)
    _check(refs, m, head, design, "deferred", *pl["mixed"], what="margin family, deferred batches of 48 + 48 + 34")
    _check(refs, m, head, design, "records", *pl["mixed"], what="margin family, record twins")


def _nan_design(head):
    K = dh.HEAD_CLASSES[0][head]
    (a, c, b), cases = dh.margin_family(K, T, *GUARD_HEADS[head])
    b = b.copy()
    b[GUARD_HEADS[head][0]] = np.nan
    return (a, c, b), cases, {k: k in ("T-", "zero", "T- other way") for k in cases}


@pytest.mark.parametrize("head", (0, 1, 2))
def test_nan_in_the_decision_head_is_rerun_under_a_gate_or_a_policy(big, head):
    """One class of the decision head is NaN in every CU.  With a gate or a candidate policy set the NaN confidence / prefix sums select every CU, in both tails."""
    refs, guarded = big
    design, cases, flagged = _nan_design(head)
    m = guarded(head, design)
    for policy in ({"min_conf": 0.5}, {"coverage": 0.9}):
        m.set_confidence_gate(128, policy.get("min_conf", 0.0))
        m.set_candidate_policy(128, policy.get("coverage", 0.0), 0)
        for form, n in (("device", 600), ("host", N_BIG), ("single", 3)):
            want = _check(refs, m, head, design, form, *_placements(cases, flagged, n)["mixed"], policy, "NaN in the decision head")
            assert want.all()
    m.set_confidence_gate(128, 0.0)
    m.set_candidate_policy(128, 0.0, 0)


@pytest.mark.parametrize("head", (0, 1, 2))
def test_nan_in_the_decision_head_is_rerun_by_the_decision_guard_alone(big, head):
    """The same CUs with no gate and no policy: the decision guard alone has to select a NaN, as the restatement does.  !(top1 - top2 >= margin) does not on its
    own: a NaN logit loses both comparisons of the top-2 scan, which then reports the margin of the OTHER classes (3.4e38 for K = 2, 200 for K = 3, 4 here; only a
    head whose logits are ALL NaN keeps both seeds, margin 0, and is selected) -- before margin_guard (csrc/mlt_tail_kernels.inc) tested for the NaN itself, 0 of
    these 600 CUs were re-run, for each of the heads 0, 1 and 2.  Batch tail, n == 1 tail; guard_select_kernel runs the same family in
    test_select_kernel_and_chunked_batches."""
    refs, guarded = big
    design, cases, flagged = _nan_design(head)
    m = guarded(head, design)
    for form, n in (("device", 600), ("host", N_BIG), ("single", 3)):
        want = _check(refs, m, head, design, form, *_placements(cases, flagged, n)["mixed"], what="NaN in the decision head, decision guard alone")
        assert want.all()


@pytest.mark.parametrize("head", (0, 1, 2))
def test_decision_guard_on_its_threshold_one_cu_per_call(big, head):
    """The n == 1 tail (mlt_predict's captured graph): once per boundary case, twice round (a flagged call must not leave its count to the next)."""
    refs, guarded = big
    K = dh.HEAD_CLASSES[0][head]
    design, cases = dh.margin_family(K, T, *GUARD_HEADS[head])
    m = guarded(head, design)
    keys = list(cases) * 2
    poc, qp = np.array([cases[k][0] for k in keys], np.int32), np.array([cases[k][1] for k in keys], np.int32)
    want = _check(refs, m, head, design, "single", poc, qp, what="margin family, mlt_predict")
    assert want.sum() == 6


def _device_values(refs, m, cases):
    """Confidence and probabilities THE DEVICE returns per case (gate and policy off: the fast pass; the designed head's logits are the same in every arithmetic)."""
    keys = list(cases)
    poc, qp = np.array([cases[k][0] for k in keys], np.int32), np.array([cases[k][1] for k in keys], np.int32)
    cand, dec, _ = m.predict_batch_candidates(refs.org[:len(keys)], refs.pred[:len(keys)], poc, qp)
    by = {(int(p), int(q)): i for i, (p, q) in enumerate(zip(poc, qp))}
    return {k: dec["confidence"][i] for k, i in by.items()}, {k: cand["prob"][i].copy() for k, i in by.items()}


def _around(x):
    return [_down(x), float(F(x)), _up(x)]


# A confidence c in [0.5, 1) is a multiple of 2^-24 and so is the band, 3 x 2^-12: c -/+ band is a float32, |c - (c -/+ band)| IS the band in fp32 and the middle
# threshold of _around(c -/+ band) is not flagged; its neighbour towards c is one float32 step inside the band and is, the outer neighbour is not.
EDGE = {"below": [False, False, True], "above": [True, False, False]}


@pytest.mark.parametrize("head", (0, 1, 2))
def test_gate_guard_a_band_away_from_the_confidence(big, head):
    """!(|confidence - min_conf| >= 0.75 x tolerance): confidence exactly 1 with the gate at 1 - band (kept) and one step above (re-run); confidence
    1 / (1 + e^-1) as the device returns it with the gate a band below and a band above, each with its two neighbours -- at the band exactly and one step
    outside it the CU is kept, one step inside it is re-run (EDGE).  Batch tail (600 CUs of all cases in turn, device and host entries) and the n == 1 tail."""
    refs, guarded = big
    K = dh.HEAD_CLASSES[0][head]
    design, cases = dh.margin_family(K, T, *GUARD_HEADS[head])
    m = guarded(head, design)
    conf_of, _ = _device_values(refs, m, cases)
    sure, one = (cases["sure"][0], cases["sure"][1]), (cases["one"][0], cases["one"][1])
    assert conf_of[sure] == F(1.0) and abs(float(conf_of[one]) - 1 / (1 + np.exp(-1.0))) <= CONF_EPS
    poc, qp = _placements(cases, {k: k in ("T-", "zero", "T- other way") for k in cases}, 600)["mixed"]
    is_one, is_sure = (poc == one[0]) & (qp == one[1]), (poc == sure[0]) & (qp == sure[1])
    c1 = float(conf_of[one])
    seen = {"below": [], "above": []}
    for side, gates in (("sure", [1.0 - BAND, _up(1.0 - BAND)]), ("below", _around(c1 - BAND)), ("above", _around(c1 + BAND))):
        for gate in gates:
            m.set_confidence_gate(128, gate)
            for form in ("device", "host"):
                want = _check(refs, m, head, design, form, poc, qp, {"min_conf": gate}, f"gate {gate!r}", conf_of=conf_of)
            if side == "sure":
                assert want[is_sure].all() == (gate != 1.0 - BAND) and not want[is_one].any(), gate
            else:
                seen[side].append(bool(want[is_one].all()))
                assert want[is_one].all() or not want[is_one].any()
            k = list(cases).index("one" if side != "sure" else "sure")
            _check(refs, m, head, design, "single", poc[:k + 1], qp[:k + 1], {"min_conf": gate}, f"gate {gate!r}, one CU per call", conf_of=conf_of)
    assert seen == EDGE, seen
    m.set_confidence_gate(128, 0.0)


@pytest.mark.parametrize("head", (0, 1, 2))
def test_candidate_guard_a_band_away_from_a_prefix_sum(big, head):
    """(a) a proper prefix sum within the band of the coverage: prefix sum exactly 1 with the coverage at 1 - band / one step above; the first prefix sum
    1 / (1 + e^-1) (the device's own probability) with the coverage a band below and above it, with neighbours."""
    refs, guarded = big
    K = dh.HEAD_CLASSES[0][head]
    design, cases = dh.margin_family(K, T, *GUARD_HEADS[head])
    m = guarded(head, design)
    conf_of, prob_of = _device_values(refs, m, cases)
    one = (cases["one"][0], cases["one"][1])
    p1 = float(prob_of[one][GUARD_HEADS[head][0]])
    assert p1 == float(conf_of[one])
    poc, qp = _placements(cases, {k: k in ("T-", "zero", "T- other way") for k in cases}, 600)["mixed"]
    is_one = (poc == one[0]) & (qp == one[1])
    seen = {"below": [], "above": []}
    for side, covs in (("sure", [1.0 - BAND, _up(1.0 - BAND)]), ("below", _around(p1 - BAND)), ("above", _around(p1 + BAND))):
        for cov in covs:
            m.set_candidate_policy(128, cov, 0)
            for form in ("device", "records"):
                want = _check(refs, m, head, design, form, poc, qp, {"coverage": cov}, f"coverage {cov!r}", prob_of=prob_of)
            if side != "sure":
                seen[side].append(bool(want[is_one].all()))
            k = list(cases).index("one" if side != "sure" else "sure")
            _check(refs, m, head, design, "single", poc[:k + 1], qp[:k + 1], {"coverage": cov}, f"coverage {cov!r}, one CU per call", prob_of=prob_of)
    assert seen == EDGE, seen
    m.set_candidate_policy(128, 0.0, 0)


@pytest.mark.parametrize("head", (1, 2))
def test_candidate_guard_b_dropped_class_gap_on_the_margin(big, head):
    """(b) classes dropped over a logit gap below the guard margin: l = (1, 0, -gap) under coverage 0.7 keeps two classes; gap T (kept), one step below (re-run),
    T + 2^-20, 0, 0.25, both orders of the two lower classes.  The top-2 margin is 1 throughout and no prefix sum is near 0.7."""
    refs, guarded = big
    K = dh.HEAD_CLASSES[0][head]
    design, cases = dh.gap_family(K, T, *GAP_HEADS[head])
    m = guarded(head, design)
    policy = {"coverage": 0.7}
    flagged = {k: dh.guard_flags(dh.designed_logits(*design, [v[0]], [v[1]])[0], T, TOL, **policy)["any"] for k, v in cases.items()}
    assert {k for k, f in flagged.items() if f} == {"T-", "zero", "T- other way"}
    _, prob_of = _device_values(refs, m, cases)
    m.set_candidate_policy(128, 0.7, 0)
    for n in (600, N_BIG):
        pl = _placements(cases, flagged, n)
        for name in ("run", "mixed", "none", "all"):
            _check(refs, m, head, design, "device" if n == 600 else "host", *pl[name], policy, f"gap family, {name}", prob_of=prob_of)
    keys = list(cases)
    _check(refs, m, head, design, "single", np.array([cases[k][0] for k in keys], np.int32), np.array([cases[k][1] for k in keys], np.int32), policy, "gap family, mlt_predict", prob_of=prob_of)
    # policy (0, 0): no candidate guard at all; a cap that keeps every class: nothing is dropped
    m.set_candidate_policy(128, 0.0, 0)
    assert not _check(refs, m, head, design, "device", *_placements(cases, flagged, 600)["mixed"], what="gap family, policy (0, 0)").any()
    m.set_candidate_policy(128, 0.7, 1)
    assert not _check(refs, m, head, design, "device", *_placements(cases, flagged, 600)["mixed"], {"coverage": 0.7, "max_modes": 1}, "gap family, cap 1", prob_of=prob_of).any()
    m.set_candidate_policy(128, 0.0, 0)


def test_select_kernel_and_chunked_batches(big, monkeypatch):
    """guard_select_kernel applies the rules to the logits in memory, a launch of its own in place of the heads kernel's tail (MLT_TUNING=1 MLT_GUARD_SELECT_KERNEL=1; 1100 CUs give each of its 1024 threads up to two CUs), and
    MLT_CHUNK=200 cuts a batch into ragged chunks with a counter pair per chunk."""
    refs, guarded = big
    head = 2
    K = dh.HEAD_CLASSES[0][head]
    design, cases = dh.margin_family(K, T, *GUARD_HEADS[head])
    gdesign, gcases = dh.gap_family(K, T, *GAP_HEADS[head])
    monkeypatch.setenv("MLT_TUNING", "1")
    monkeypatch.setenv("MLT_GUARD_SELECT_KERNEL", "1")
    ms = guarded(head, design, env="select")
    monkeypatch.delenv("MLT_GUARD_SELECT_KERNEL")
    monkeypatch.setenv("MLT_CHUNK", "200")
    mc = guarded(head, design, env="chunk")
    monkeypatch.delenv("MLT_CHUNK")
    monkeypatch.delenv("MLT_TUNING")
    flagged = {k: k in ("T-", "zero", "T- other way") for k in cases}
    # the contexts took the paths they are named for: launches of one batch of 1100 CUs, none of them flagged, as the context's own profile counts them
    none = _placements(cases, flagged, N_BIG)["none"]
    launches = {}
    for name, m in (("tail", guarded(head, design)), ("select", ms), ("chunk", mc)):
        m.profile_enable(True)
        _check(refs, m, head, design, "host", *none, what=f"{name}: launches")
        launches[name] = {e["name"]: e["launches"] for e in m.profile_read()}
        m.profile_enable(False)
    got = {name: (p.get("heads", 0), p.get("guard_select", 0)) for name, p in launches.items()}
    # (heads launches, guard_select launches): host arrays are staged 512 CUs at a time (stage_chunk, csrc/mlt_runtime.h), so 1100 CUs are 3 passes, each with its
    # own selection; in chunks of 200 they are 6
    assert got == {"tail": (3, 0), "select": (3, 3), "chunk": (6, 0)}, got
    for what, m in (("guard_select_kernel", ms), ("MLT_CHUNK=200", mc)):
        m = guarded(head, design, env="select" if m is ms else "chunk")
        conf_of, prob_of = _device_values(refs, m, cases)
        for n in (600, N_BIG):
            pl = _placements(cases, flagged, n)
            for name in ("first", "last", "run", "all", "none", "mixed"):
                _check(refs, m, head, design, "device" if name != "mixed" else "host", *pl[name], what=f"{what}: margin family, {name}")
        poc, qp = _placements(cases, flagged, N_BIG)["mixed"]
        c1 = float(conf_of[(cases["one"][0], cases["one"][1])])
        for gate in _around(c1 - BAND) + _around(c1 + BAND) + [1.0 - BAND, _up(1.0 - BAND)]:
            m.set_confidence_gate(128, gate)
            _check(refs, m, head, design, "device", poc, qp, {"min_conf": gate}, f"{what}: gate {gate!r}", conf_of=conf_of)
        m.set_confidence_gate(128, 0.0)
        for cov in _around(c1 - BAND) + _around(c1 + BAND) + [1.0 - BAND, _up(1.0 - BAND)]:
            m.set_candidate_policy(128, cov, 0)
            _check(refs, m, head, design, "device", poc, qp, {"coverage": cov}, f"{what}: coverage {cov!r}", prob_of=prob_of)
        m = guarded(head, gdesign, env="select" if m is ms else "chunk")
        _, prob_of = _device_values(refs, m, gcases)
        m.set_candidate_policy(128, 0.7, 0)
        gfl = {k: k in ("T-", "zero", "T- other way") for k in gcases}
        for name in ("run", "mixed"):
            _check(refs, m, head, gdesign, "device", *_placements(gcases, gfl, N_BIG)[name], {"coverage": 0.7}, f"{what}: gap family, {name}", prob_of=prob_of)
        m.set_candidate_policy(128, 0.0, 0)
        ndesign, ncases, nfl = _nan_design(head)     # a NaN class, the decision guard alone (margin_guard's NaN test in this copy)
        m = guarded(head, ndesign, env="select" if m is ms else "chunk")
        assert _check(refs, m, head, ndesign, "device", *_placements(ncases, nfl, N_BIG)["mixed"], what=f"{what}: NaN in the decision head").all()


def test_growing_and_shrinking_batches_leave_no_count_behind(big):
    """The batch tail appends to one of two counters and re-arms the other for the next launch: calls of n = 1, 7, 600, 3, 1100, 2 with every CU flagged, each
    followed by a call in which none is -- a count that survived would show as re-runs there (and the bad-count check would fail the call)."""
    refs, guarded = big
    head = 1
    design, cases = dh.margin_family(3, T, *GUARD_HEADS[head])
    m = guarded(head, design)
    flagged = {k: k in ("T-", "zero", "T- other way") for k in cases}
    for n in (1, 7, 600, 3, N_BIG, 2, 600):
        pl = _placements(cases, flagged, max(n, 1))
        for name in ("all", "none", "mixed") if n > 1 else ("all", "none"):
            want = _check(refs, m, head, design, "device", *pl[name], what=f"sequence, {name}")
            assert want.sum() == {"all": n, "none": 0}.get(name, want.sum())


def test_six_classes_on_a_guarded_small_model(gpu):
    """The K = 6 boundary set -- decision guard and candidate guard (b) -- on the 64 x 64 model with head_index 3: the calibration of a designed blob keeps a
    single-pass prefix (exact == 4, asserted) and with it the guards."""
    pkg = gpu
    Fl = pkg.capi
    kw = dict(tolerance=TOL, guard_margin=T)
    design, cases = dh.margin_family(6, T, 4, 2)
    blob = dh.designed_blob(1, SEED, 3, *design)
    refs = Refs(pkg, 64, 150, Fl.FLAG_NO_CALIBRATION, Fl.FLAG_NO_DECISION_GUARD, blob=blob, **kw)
    assert not pkg.synth.flat_guard_flags(refs.org, refs.pred, flat_div=16)[2].any(), "the flat guard (left on: the shipped configuration) must flag none of the texture CUs"
    m = pkg.MltCnn(device=0, sizes=(64,), blobs={64: blob}, head_index={64: 3}, **kw)
    a, af, ae = m.arithmetic(64), refs.fa.arithmetic(64), refs.ex.arithmetic(64)
    print("64 x 64:", a)
    assert a["exact"] == 4 and a["decision_guard"] == 1 and a["guard_margin"] == T and a["mag_guard_kind"] == 0, a
    assert ae["exact"] == 1 and af["exact"] == 4 and af["decision_guard"] == 0 and (af["x_units"], af["w2_units"], af["rounding"]) == (a["x_units"], a["w2_units"], a["rounding"]), (a, af)
    flagged = {k: k in ("T-", "zero", "T- other way") for k in cases}
    pl = _placements(cases, flagged, 150)
    for name, form in (("mixed", "host"), ("mixed", "device"), ("all", "device"), ("none", "device"), ("first", "host")):
        _check(refs, m, 3, design, form, *pl[name], what=f"64: margin family, {name}")
    keys = list(cases)
    _check(refs, m, 3, design, "single", np.array([cases[k][0] for k in keys], np.int32), np.array([cases[k][1] for k in keys], np.int32), what="64: margin family, mlt_predict")
    gdesign, gcases = dh.gap_family(6, T, 5, 0, 3)
    gblob = dh.designed_blob(1, SEED, 3, *gdesign)
    m.load_weights(64, gblob)
    refs.reload(gblob)
    a2, af2 = m.arithmetic(64), refs.fa.arithmetic(64)
    assert (a2["exact"], a2["decision_guard"]) == (4, 1) and (af2["exact"], af2["x_units"], af2["w2_units"], af2["rounding"]) == (4, a2["x_units"], a2["w2_units"], a2["rounding"]), (a2, af2)
    _, prob_of = _device_values(refs, m, gcases)
    m.set_candidate_policy(64, 0.7, 0)
    gfl = {k: k in ("T-", "zero", "T- other way") for k in gcases}
    gpl = _placements(gcases, gfl, 150)
    for name, form in (("mixed", "host"), ("mixed", "device"), ("last", "device")):
        _check(refs, m, 3, gdesign, form, *gpl[name], {"coverage": 0.7}, f"64: gap family, {name}", prob_of=prob_of)
    keys = list(gcases)
    _check(refs, m, 3, gdesign, "single", np.array([gcases[k][0] for k in keys], np.int32), np.array([gcases[k][1] for k in keys], np.int32), {"coverage": 0.7}, "64: gap family, mlt_predict",
           prob_of=prob_of)
    print(f"64: worst coincidence share {max(refs.shares):.4f}")
    m.close()
    refs.close()


# ---- d: a tree over a decision head with a NaN ---------------------------------------------------------------------------------------------------------------
def test_tree_over_a_nan_decision_head(gpu):
    """Size-32 head 0 has a NaN bias in class 1.  Without candidate records cand_mask is written by tree_expand_kernel's own scan (every class of the head when a
    logit is NaN): the tree must be the one with records, and the host descent's, byte for byte.  By split mode no node descends (the comparison scan leaves class
    0); with MLT_TREE_BY_CANDIDATES every node does."""
    from test_tree_gpu import _same, device_tree, host_tree
    pkg = gpu
    W, H = 96, 64
    blobs = {32: dh.designed_blob(1, SEED, 0, [0, 0], [0, 0], [0.0, np.nan]), 16: pkg.weights.synthetic_blob(1, SEED)}
    m = pkg.MltCnn(device=0, sizes=(32, 16), blobs=blobs, head_index={32: 0, 16: 0}, flags=pkg.capi.FLAG_NO_CALIBRATION)
    o, p = pkg.synth.make_patches_bulk(32, 6, 11)
    tile = lambda v: np.ascontiguousarray(v.reshape(2, 3, 32, 32).transpose(0, 2, 1, 3).reshape(H, W))
    po, pp = m.picture(W, H).upload(tile(o)), m.picture(W, H).upload(tile(p))
    for by_cand, count in ((False, 6), (True, 30)):
        kw = dict(top=32, min_size=16, by_candidates=by_cand)
        nodes, leaf_map, rec, _ = host_tree(pkg, m, po, pp, W, H, **kw)
        full, _ = device_tree(m, po, pp, want=TREE_ALL, sizes=(32, 16), **kw)
        bare, _ = device_tree(m, po, pp, want=("leaf_map",), sizes=(32, 16), **kw)
        assert len(nodes) == count, (by_cand, len(nodes))
        assert _same(full["nodes"], nodes) and _same(bare["nodes"], nodes), by_cand
        assert _same(full["leaf_map"], leaf_map) and _same(bare["leaf_map"], leaf_map)
        top = bare["nodes"][bare["nodes"]["size"] == 32]
        assert len(top) == 6 and (top["cand_mask"] == 3).all() and np.isnan(top["confidence"]).all() and (top["split_mode"] == 0).all()
        assert ((top["first_child"] >= 0) == by_cand).all()
        assert (full["candidates"]["mask"][:6] == 3).all() and (full["candidates"]["order"][:6, :2] == [0, 1]).all()
        low = bare["nodes"][bare["nodes"]["size"] == 16]
        assert len(low) == count - 6 and (np.isin(low["cand_mask"], (1, 2))).all()
    po.close(); pp.close()
    m.close()
