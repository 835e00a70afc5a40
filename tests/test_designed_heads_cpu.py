"""CPU: the designed-head helper (tests/designed_heads.py) against the C oracle, the coverage of its case set, the host restatements
(decisions.from_logits / candidates_from_logits) ON their thresholds, and the scalar restatement of the guard rules against expectations stated by hand.
The device side is tests/test_designed_heads_gpu.py."""
import numpy as np
import pytest

import designed_heads as dh

F = np.float32
BIG, SCALARS, _sixteenths, _one_sided = dh.BIG, dh.SCALARS, dh.sixteenths, dh.one_sided


@pytest.mark.parametrize("size", (128, 16))
def test_oracle_returns_the_designed_logits_exactly(pkg, size):
    """Both architectures, every head: the C oracle's bytes for the designed head are designed_logits' -- including the |poc|, |qp| >= 2^24 cases, where the
    expected operand is np.float32(poc)."""
    import oracle
    arch = dh.arch_of(size)
    poc, qp = (np.array(v, np.int32) for v in zip(*SCALARS))
    assert np.float32(BIG + 1) == BIG and np.float32(-(BIG + 3)) == -(BIG + 4)
    org, pred = pkg.synth.make_patches_bulk(size, len(poc), 5)
    plain_big = oracle.Oracle(pkg.weights.synthetic_blob(arch, 13)).forward(org, pred, poc, qp)[0]
    small = np.maximum(np.abs(poc), np.abs(qp)) < BIG
    for head, K, design in [(h, K, d) for h, K in enumerate(dh.HEAD_CLASSES[arch]) for d in (_sixteenths, _one_sided)]:
        a, c, b = design(K, head)
        if design is _sixteenths:     # (general coefficients are exact on small scalars only: the large ones get the small ones' values)
            poc, qp = np.where(small, poc, 7).astype(np.int32), np.where(small, qp, -9).astype(np.int32)
            plain = oracle.Oracle(pkg.weights.synthetic_blob(arch, 13)).forward(org, pred, poc, qp)[0]
        else:
            poc, qp = (np.array(v, np.int32) for v in zip(*SCALARS))
            plain = plain_big
        blob = dh.designed_blob(arch, 13, head, a, c, b)
        got = oracle.Oracle(blob).forward(org, pred, poc, qp)[0]
        want = dh.designed_logits(a, c, b, poc, qp)
        lo = dh.head_offset(arch, head)
        assert got[:, lo:lo + K].tobytes() == want.tobytes(), (size, head)
        other = np.ones(got.shape[1], bool)
        other[lo:lo + K] = False
        assert got[:, other].tobytes() == plain[:, other].tobytes(), "the other heads keep their seeded weights"
        assert not np.array_equal(got[:, lo:lo + K], plain[:, lo:lo + K])
    # keep_other_heads=False: the other heads answer +0.0
    z = oracle.Oracle(dh.designed_blob(arch, 13, 0, *_sixteenths(2, 0), keep_other_heads=False)).forward(org, pred, poc, qp)[0]
    assert (z[:, 2:].view(np.uint32) == 0).all()


def test_designed_logits_refuses_an_inexact_design():
    with pytest.raises(AssertionError):
        dh.designed_logits([F(0.1), F(0.0)], [F(0.0), F(0.0)], [F(0.0), F(0.0)], [3], [0])      # 0.1f * 3 rounds
    with pytest.raises(AssertionError):
        dh.designed_logits([F(1.0), F(0.0)], [F(0.0), F(0.0)], [F(2.0 ** -30), F(0.0)], [1], [0])  # 1 + 2^-30 rounds
    l = dh.designed_logits([F(-1.0), F(0.0)], [F(0.0), F(0.0)], [F(0.0), F(0.0)], [0], [0])
    assert (l.view(np.uint32) == 0).all(), "-1 * 0 enters the kernel's fmaf as -0 + +0 = +0"


def _reached(K):
    sigs = set()
    for _, reps in dh.case_set(K):
        sigs |= {s for s, _, _ in reps}
    return sigs, {s for s in sigs if dh.is_strict(s)}


def test_case_set_reaches_the_required_orders():
    """At most 8 designs per K; K = 2: all 3 weak orders; 3: all 13; 4: all 24 strict and >= 56 weak; 6: >= 400 strict with the identity and the full reversal,
    all 36 (class, rank) pairs, all 30 ordered (top, second) pairs, >= 700 weak."""
    counts = {}
    for K in (2, 3, 4, 6):
        assert len(dh.DESIGNS[K]) <= 8
        for (a, c, b), reps in dh.case_set(K):
            l = dh.designed_logits(a, c, b, [p for _, p, _ in reps], [q for _, _, q in reps])
            assert (np.abs(l) <= 64).all() and all(max(abs(p), abs(q)) <= 48 for _, p, q in reps)
            assert all(dh.signature(row) == s for row, (s, _, _) in zip(l, reps))
        weak, strict = _reached(K)
        counts[K] = (len(weak), len(strict))
        if K == 6:
            assert tuple(range(6)) in strict and tuple(range(5, -1, -1)) in strict
            assert len({(k, s[k]) for s in strict for k in range(6)}) == 36
            assert len({(s.index(0), s.index(1)) for s in strict}) == 30
    print("weak / strict orders reached per K:", counts)
    assert counts[2][0] == 3 and counts[3][0] == 13
    assert counts[4][1] == 24 and counts[4][0] >= 56
    assert counts[6][1] >= 400 and counts[6][0] >= 700


def test_signature_counts_weak_orders():
    assert dh.signature([1.0, 1.0, 0.0]) == (0, 0, 2) and dh.signature([0.0, 2.0, 1.0]) == (2, 0, 1) and dh.signature([5.0, 5.0]) == (0, 0)
    import itertools
    assert len({dh.signature(v) for v in itertools.product(range(3), repeat=3)}) == 13
    assert len({dh.signature(v) for v in itertools.product(range(4), repeat=4)}) == 75


# ---- the package's float64 restatements ON their thresholds ------------------------------------------------------------------------------------------------
def _tie_row(size, head, m, first=0):
    """All logits of `size`: head `head` has m classes tied at 0 from class `first`, the rest 200 below; the other heads are decisive."""
    classes = dh.HEAD_CLASSES[dh.arch_of(size)]
    row = []
    for h, K in enumerate(classes):
        if h == head:
            v = [-200.0] * K
            for k in range(first, first + m):
                v[k] = 0.0
        else:
            v = [float(-10 * k) for k in range(K)]
        row += v
    return np.array([row], F)


@pytest.mark.parametrize("size,head,m,first", [(128, 0, 1, 1), (128, 0, 2, 0), (128, 2, 2, 1), (128, 2, 4, 0), (16, 3, 1, 5), (16, 3, 2, 3), (16, 3, 4, 1), (16, 2, 4, 0)])
def test_candidates_from_logits_on_the_coverage(pkg, size, head, m, first):
    """m = 1, 2, 4 classes tied at the top: every probability is 1 / m and every prefix sum j / m, exact in fp32 and in float64.  coverage = j / m keeps j classes
    (cum >= coverage holds with equality), the next float32 keeps j + 1; the lower classes come first."""
    assert np.exp(F(-200.0), dtype=F) == 0 and 1.0 + np.exp(-200.0) == 1.0
    lg = _tie_row(size, head, m, first)
    K = dh.HEAD_CLASSES[dh.arch_of(size)][head]
    for j in range(1, m + 1):
        cov = j / m
        if cov >= 1.0:
            continue
        r = pkg.decisions.candidates_from_logits(size, lg, head_index=head, coverage=cov)[0]
        assert list(r["prob"][first:first + m]) == [1.0 / m] * m and list(r["cum"][:m]) == [(i + 1) / m for i in range(m)]
        assert r["n"] == r["count"] == j and r["mask"] == sum(1 << (first + i) for i in range(j)), (cov, r)
        assert list(r["order"][:m]) == list(range(first, first + m))
        up = float(np.nextafter(F(cov), F(1.0)))
        r = pkg.decisions.candidates_from_logits(size, lg, head_index=head, coverage=up)[0]
        assert r["n"] == r["count"] == j + 1 and r["mask"] == sum(1 << (first + i) for i in range(j + 1)), (up, r)
        # ... and under a cap of j classes the step above the coverage falls back to all K
        r = pkg.decisions.candidates_from_logits(size, lg, head_index=head, coverage=up, max_modes=j)[0]
        assert r["n"] == j + 1 and r["count"] == K and r["mask"] == (1 << K) - 1
        # the scalar restatement says the same
        mine = dh.candidates(lg[0, dh.head_offset(dh.arch_of(size), head):][:K], cov)
        assert (mine["n"], mine["mask"], mine["order"][:m]) == (j, sum(1 << (first + i) for i in range(j)), list(range(first, first + m)))
        assert dh.candidates(lg[0, dh.head_offset(dh.arch_of(size), head):][:K], up)["n"] == j + 1
    if m == 1:
        r = pkg.decisions.candidates_from_logits(size, lg, head_index=head, coverage=float(np.nextafter(F(1.0), F(0.0))))[0]
        assert r["n"] == 1 and r["mask"] == 1 << first


@pytest.mark.parametrize("size,head,m,first", [(128, 0, 2, 0), (128, 2, 4, 0), (128, 2, 2, 2), (16, 3, 4, 2), (16, 3, 1, 4)])
def test_from_logits_on_the_gate(pkg, size, head, m, first):
    """min_confidence EQUAL to the confidence keeps the split; one float32 step above withholds it."""
    lg = _tie_row(size, head, m, first)
    conf = 1.0 / m
    r = pkg.decisions.from_logits(size, lg, head_index=head)[0]
    assert r["confidence"] == conf and r["raw_mode"] == first and r["margin"] == (0.0 if m > 1 else 200.0) and r["level_conf"][head] == conf
    if conf < 1.0:
        assert pkg.decisions.from_logits(size, lg, head_index=head, min_confidence=conf)[0]["split_mode"] == first
        up = float(np.nextafter(F(conf), F(1.0)))
        assert pkg.decisions.from_logits(size, lg, head_index=head, min_confidence=up)[0]["split_mode"] == -1
        K = dh.HEAD_CLASSES[dh.arch_of(size)][head]
        row = lg[0, dh.head_offset(dh.arch_of(size), head):][:K]
        assert dh.decide(row, conf)["split_mode"] == first and dh.decide(row, up)["split_mode"] == -1 and dh.decide(row)["confidence"] == F(conf)
    else:
        top = float(np.nextafter(F(1.0), F(0.0)))
        assert pkg.decisions.from_logits(size, lg, head_index=head, min_confidence=top)[0]["split_mode"] == first


# ---- the scalar restatement of the guards against expectations stated by hand --------------------------------------------------------------------------------
T, TOL = F(2.0 ** -8), F(2.0 ** -10)
BAND = F(0.75) * TOL                     # 3 x 2^-12, exact
EPS = F(2.0 ** -32)                      # one fp32 step of a number in [2^-9, 2^-8)
STEP_HALF = F(2.0 ** -25)                # one fp32 step below 0.5
NAN = F(np.nan)


def _up(x):
    return float(np.nextafter(F(x), F(2.0)))


def _down(x):
    return float(np.nextafter(F(x), F(-2.0)))


BOUNDARY = [
    # logits, policy (min_conf, coverage, max_modes), expected (decision, gate, cand_a, cand_b)
    ("margin = T", [T, 0], {}, (False, False, False, False)),
    ("margin one step below T", [F(T - EPS), 0], {}, (True, False, False, False)),
    ("margin T, second class on top, K = 3", [-200, 0, T], {}, (False, False, False, False)),
    ("margin below T, second class on top", [-200, F(-T + EPS), 0], {}, (True, False, False, False)),
    ("a tie", [3, 3, -200, -200], {}, (True, False, False, False)),
    ("NaN, no gate, no policy", [0, NAN, -200], {}, (True, False, False, False)),
    ("NaN under a gate and a policy", [0, NAN, -200], {"min_conf": 0.5, "coverage": 0.9}, (True, True, True, False)),
    ("gate at conf - band: on the band's edge", [200, 0], {"min_conf": 1.0 - float(BAND)}, (False, False, False, False)),
    ("gate one step inside", [200, 0], {"min_conf": _up(1.0 - float(BAND))}, (False, True, False, False)),
    ("tie: conf 0.5, gate at conf + band (the tie itself is a near-tie)", [0, 0], {"min_conf": 0.5 + float(BAND)}, (True, False, False, False)),
    ("tie: gate one step inside, above", [0, 0], {"min_conf": _down(0.5 + float(BAND))}, (True, True, False, False)),
    ("tie: gate at conf - band", [0, 0], {"min_conf": 0.5 - float(BAND)}, (True, False, False, False)),
    ("tie: gate one step inside, below", [0, 0], {"min_conf": _up(0.5 - float(BAND))}, (True, True, False, False)),
    ("four-way tie: conf 0.25, gate at conf + band", [0, 0, 0, 0], {"min_conf": 0.25 + float(BAND)}, (True, False, False, False)),
    ("four-way tie: one step inside", [0, 0, 0, 0], {"min_conf": _down(0.25 + float(BAND))}, (True, True, False, False)),
    ("coverage at cum - band (cum = 1)", [200, 0, -1], {"coverage": 1.0 - float(BAND)}, (False, False, False, False)),
    ("coverage one step inside", [200, 0, -1], {"coverage": _up(1.0 - float(BAND))}, (False, False, True, False)),
    ("tie pair: prefix 0.5, coverage at cum + band", [0, 0, -200], {"coverage": 0.5 + float(BAND)}, (True, False, False, False)),
    ("tie pair: coverage one step inside", [0, 0, -200], {"coverage": _down(0.5 + float(BAND))}, (True, False, True, False)),
    ("the LAST prefix sum is no proper prefix", [0, 0], {"coverage": _down(1.0)}, (True, False, False, False)),
    ("dropped gap = T", [1, 0, -T, -200], {"coverage": 0.7}, (False, False, False, False)),
    ("dropped gap one step below T", [1, 0, F(-T + EPS), -200], {"coverage": 0.7}, (False, False, False, True)),
    ("dropped gap below T but the cap keeps every class", [1, 0, F(-T + EPS), -200], {"coverage": 0.7, "max_modes": 1}, (False, False, False, False)),
    ("policy (0, 0): no candidate guard", [1, 0, F(-T + EPS)], {}, (False, False, False, False)),
    ("(t, 1): one class kept over a gap below T", [0, F(-T + EPS), -200], {"coverage": 0.25, "max_modes": 1}, (True, False, False, True)),
]


@pytest.mark.parametrize("what,l,policy,want", BOUNDARY, ids=[b[0] for b in BOUNDARY])
def test_guard_restatement_on_boundaries(what, l, policy, want):
    assert F(T - EPS) < T and F(T - EPS) == np.nextafter(T, F(0)) and F(0.5) - STEP_HALF == np.nextafter(F(0.5), F(0))
    got = dh.guard_flags(l, T, TOL, **policy)
    assert (got["decision"], got["gate"], got["cand_a"], got["cand_b"]) == want, (what, got)
    assert got["any"] == any(want)


def test_threshold_families_state_their_margins():
    for K, p, q in ((2, 0, 1), (2, 1, 0), (3, 2, 0), (4, 3, 1), (6, 4, 2)):
        (a, c, b), cases = dh.margin_family(K, T, p, q)
        for name, (poc, qp, margin) in cases.items():
            l = dh.designed_logits(a, c, b, [poc], [qp])[0]
            d = dh.decide(l)
            assert d["margin"] == margin and d["raw_mode"] == (min(p, q) if margin == 0 else p if qp > 0 else q), (K, name, l)
            assert dh.guard_flags(l, T, TOL)["decision"] == (name in ("T-", "zero", "T- other way")), (K, name)
        assert dh.decide(dh.designed_logits(a, c, b, [0], [51200])[0])["confidence"] == 1.0
    for K, p, q, r in ((3, 0, 1, 2), (3, 2, 0, 1), (4, 1, 3, 0), (6, 5, 0, 3)):
        (a, c, b), cases = dh.gap_family(K, T, p, q, r)
        for name, (poc, qp, gap) in cases.items():
            l = dh.designed_logits(a, c, b, [poc], [qp])[0]
            cd = dh.candidates(l, 0.7)
            assert cd["count"] == 2 and cd["gap"] == gap and cd["order"][0] == p and set(cd["order"][1:3]) == {q, r}, (K, name, cd)
            g = dh.guard_flags(l, T, TOL, coverage=0.7)
            assert (g["decision"], g["cand_a"]) == (False, False) and g["cand_b"] == (name in ("T-", "zero", "T- other way")), (K, name, g)
