"""CPU: the shift weights (tests/shift_weights.py) -- the conditions under which "no arithmetic tier rounds" is true of the family, its reference against the C
oracle, the tolerance RHO_SHIFT, its power, and the coverage of run_network's lo-plane hand-offs by the configurations tests/test_shift_gpu.py runs.  Nothing in
this file or in the tolerance comes from a device run.

Conditions, per size (128, 64) and tap set (0, 1, 2):
  (a) rounding-free   the largest relative deviation of Net64("fp16") and Net64("hilo") from float64 over impulses of 512 / 37 / 1 at tw.sample_positions(size, 24, 40)
                      of both planes is <= 2e-7 (measured 8.7e-8 at 128, 1.01e-7 at 64: 1023 x float32(1 / 1023) and the BN fold's 6.8e-9); a logit that is 0 in
                      float64 is 0 under either rounding.  Amplitude 37 also on the rest of the 512-position subset in tap set 0, where the GPU test runs it
  (b) range           the all-ones CU stays below 2^14 (128: 9990, 64: 9393 .. 12488)
  (c) underflow       tw.underflow_terms on the family is <= 1e-7 of the smallest non-zero expected logit (measured: 0 -- no activation of the family is an fp16
                      subnormal; amplitude 1 on the sets with the stem 2^10 larger)
  (d) not vacuous     at least 30 % of the sweep's CUs have every expected logit > 0 (128: 76 / 75 / 100 %, 64: 65 / 73 / 100 %)
  (e) linearity (ws.adjoint(check=True)), agreement with the C oracle on 36 impulse CUs per tap set (ws.SHIFT_ORACLE_MEASURED; 8 dense CUs against the oracle's own fp32 bound), power: each of tw.mutations(size) moves some
      impulse response of some tap set by more than 100 x RHO_SHIFT; each tap mutation (one tap zeroed or moved to its neighbour) turns some expected logit of
      the sweep from non-zero to zero or the reverse."""
import time

import numpy as np
import pytest

import shift_weights as ws
import tracer_weights as tw

CASES = [(size, ts) for size in ws.SIZES for ts in ws.TAPSETS]
ORACLE_BOUND_DENSE = 6e-5
_CACHE, _DEV = {}, {}


def shift(size, tapset=0, low=False):
    """(state dict, G) of a set, computed once."""
    key = (size, tapset, low)
    if key not in _CACHE:
        sd = ws.shift_state_dict(size, tapset, ws.stem_gain(size, 1 if low else 512))
        _CACHE[key] = (sd, ws.adjoint(sd, size))            # (e): adjoint(check=True) -- linear on non-negative content, the zero CU exactly 0
    return _CACHE[key]


def deviation(size, tapset):
    if (size, tapset) not in _DEV:
        _DEV[(size, tapset)] = ws.emulated_deviation(size, tapset)
    return _DEV[(size, tapset)]


@pytest.mark.parametrize("size", ws.SIZES)
def test_weights_are_what_the_construction_says(pkg, size):
    for ts in ws.TAPSETS:
        sd = ws.shift_state_dict(size, ts)
        a, back = pkg.weights.unpack_blob(ws.shift_blob(size, ts))
        assert a == tw.arch_of(size)
        tp = ws.taps(size, ts)
        for k, v in back.items():
            assert np.array_equal(v, sd[k]), k
            if v.ndim == 4 and v.shape[2] == 3:
                nz = np.argwhere((v != 0).any(axis=(0, 1)))
                assert sorted(map(tuple, nz)) == sorted(set(tp[k[:-7]])), (k, nz.tolist(), tp[k[:-7]])
                w = v[v != 0]
                m, e = np.frexp(w.astype(np.float64) / (1023.0 if k == "conv1.weight" else 1.0))
                assert (m == 0.5).all() and w.min() > 2.0 ** -14 and w.max() < 2.0 ** 14, k          # powers of two (the stem: 1023 x one), normal in fp16
                if v.shape[1] == 96:
                    assert (v[:, 64:] == 0).all() and (v[:, :64] != 0).any()
        assert np.array_equal(ws.shift_state_dict(size, ts, ws.stem_gain(size, 1))["conv1.weight"], np.float32(ws.STEM_LOW) * sd["conv1.weight"])
    # the seeded tap sets differ in every conv that is not pinned to the centre tap (or mirrors one that is), the third is the centre set; channels are told apart
    t0, t1, t2 = (ws.taps(size, ts) for ts in ws.TAPSETS)
    for k in t0:
        pinned = k.startswith("layer") and ws.map_of(size, int(k[5])) <= 2 and len(t0[k]) == 1
        assert (t0[k] == t1[k] == [(1, 1)]) if pinned else t0[k] != t1[k], k
        assert t2[k] in ([(1, 1)], [(1, 1), (1, 1)], [(1, 1), (1, 2), (2, 1), (2, 2)]), k
        if k.endswith(".1.conv2"):
            assert [(2 - y, 2 - x) for y, x in t0[k[:-1] + "1"]] == t0[k]
    w = ws.shift_state_dict(size, 0)["layer1.1.conv1.weight"]
    assert len(np.unique(w[w != 0])) >= 3


@pytest.mark.parametrize("size,tapset", CASES)
def test_rounding_free(size, tapset):
    """(a)"""
    t0 = time.time()
    d = deviation(size, tapset)
    print(f"size {size} tap set {tapset}: largest relative deviation from float64: fp16 {d['fp16']:.2e}, hilo {d['hilo']:.2e} ({time.time() - t0:.1f} s)")
    assert d["fp16"] <= 2e-7 and d["hilo"] <= 2e-7, d


@pytest.mark.parametrize("size,tapset", CASES)
def test_conditions(pkg, size, tapset):
    """(b), (c), (d)"""
    sd, G = shift(size, tapset)
    sdl, Gl = shift(size, tapset, True)
    assert np.array_equal(Gl, ws.STEM_LOW * G) and (G >= 0).all() and np.isfinite(G).all()
    top = tw.activation_report(sd, np.ones((1, 2, size, size)))
    assert top < 2.0 ** 14, top
    top_low = max(tw.activation_report(sdl, tw.preprocess(o, p)) for a, _, o, p in ws.family(size) if a == 1)
    assert top_low < 2.0 ** 14, top_low
    worst = 0.0
    for a, plane, o, p in ws.family(size):
        s_, g_ = (sdl, Gl) if a == 1 else (sd, G)
        want = tw.expected(g_, o, p)
        if not (want > 0).any():
            continue
        frac = tw.underflow_terms(s_, size, tw.preprocess(o, p)).max() / want[want > 0].min()
        worst = max(worst, frac)
        assert frac <= 1e-7, (a, plane, frac)
    plane, pos = tw.sweep(size)
    e = tw.expected_impulse(G, plane, pos, 512)
    hk = tw.head_of_logit(tw.arch_of(size))
    full = float((e > 0).all(axis=1).mean())
    heads = [float((e[:, hk == h] > 0).all(axis=1).mean()) for h in range(hk.max() + 1)]
    print(f"size {size} tap set {tapset}: all-ones top {top:.4g}, amplitude 1 top {top_low:.4g}, underflow term / smallest logit {worst:.1e}; "
          f"CUs with every logit > 0: {full:.0%}, per head {[f'{h:.0%}' for h in heads]}")
    assert full >= 0.30
    # within a head the classes are 2^-k of one another: a head is zero or non-zero as a whole
    for h in range(hk.max() + 1):
        z = e[:, hk == h] > 0
        assert (z.all(axis=1) | ~z.any(axis=1)).all()


@pytest.mark.parametrize("size", ws.SIZES)
def test_expected_agrees_with_the_c_oracle(pkg, size):
    from oracle import Oracle
    pos = tw.sample_positions(size, 6, 8)
    worst = 0.0
    for ts, amp in ((0, 512), (1, 37), (2, 1)):           # 36 impulse CUs per tap set, and 8 dense CUs on the first
        sd, G = shift(size, ts, amp == 1)
        orc = Oracle(ws.shift_blob(size, ts, ws.stem_gain(size, amp)))
        cases = [tw.impulses(size, plane, pos, amp) for plane in (0, 1)]
        if amp == 512:
            cases.append(pkg.synth.make_patches_bulk(size, 8, 31))
        org, pred = (np.concatenate([c[i] for c in cases]) for i in (0, 1))
        n = len(org)
        want = tw.expected(G, org, pred)
        got, _ = orc.forward(org, pred, np.zeros(n, np.int32), np.zeros(n, np.int32), threads=8)
        got = got.astype(np.float64)
        assert (got[want == 0.0] == 0.0).all()
        k = 2 * len(pos)
        rel = np.abs(got - want)[:k][want[:k] > 0] / want[:k][want[:k] > 0]
        print(f"size {size} tap set {ts} amplitude {amp}: expected vs C oracle, {k} impulse CUs: max relative {rel.max():.2e}")
        worst = max(worst, float(rel.max()))
        if n > k:
            # dense content: the ORACLE's fp32 sums round (2304 products per output, 21 layers: the bound of tests/test_tracer_cpu.py) -- `expected` does not
            dense = float((np.abs(got - want)[k:] / want[k:]).max())
            print(f"size {size} tap set {ts}: {n - k} dense CUs: max relative {dense:.2e}")
            assert (want[k:] > 0).all() and dense <= ORACLE_BOUND_DENSE
    assert worst <= ws.SHIFT_ORACLE_MEASURED[size], (worst, "ws.SHIFT_ORACLE_MEASURED is no longer what is measured")
    assert worst >= 0.25 * ws.SHIFT_ORACLE_MEASURED[size] or ws.SHIFT_ORACLE_MEASURED[size] <= 2.0 ** -24


@pytest.mark.parametrize("size", ws.SIZES)
def test_tolerance(size):
    emu = max(max(deviation(size, ts).values()) for ts in ws.TAPSETS)
    rho = 8 * max(emu, ws.SHIFT_ORACLE_MEASURED[size], 2.0 ** -24)
    print(f"size {size}: emulation {emu:.3e}, oracle {ws.SHIFT_ORACLE_MEASURED[size]:.2e}, 2^-24 {2.0 ** -24:.2e} -> rho_shift {rho:.3e} (table {ws.RHO_SHIFT[size]:.3e})")
    assert emu <= ws.SHIFT_EMULATED[size]
    assert abs(ws.RHO_SHIFT[size] - rho) <= 0.05 * rho
    assert ws.RHO_SHIFT[size] < 2e-6 < 1e-3 * min(tw.RHO_FAST[size]) * 8


@pytest.mark.parametrize("size", ws.SIZES)
def test_power(size):
    rho = ws.RHO_SHIFT[size]
    missed = []
    for name, mut in tw.mutations(size):
        best = 0.0
        for ts in ws.TAPSETS:
            sd, G = shift(size, ts)
            Gm = ws.adjoint(sd, size, mutation=mut, check=False)
            nz = G > 0
            assert ((Gm > 0) == nz).all()
            move = np.abs(Gm - G)[nz] / G[nz]
            best = max(best, float(move.max()) if move.size else 0.0)
        print(f"size {size}: {name}: largest move {best:.2%} = {best / rho:.0f} x rho_shift")
        if not best > 100 * rho:
            missed.append(name)
    assert not missed, f"mutations the tolerance cannot see: {missed}"


@pytest.mark.parametrize("size", ws.SIZES)
def test_tap_mutations_change_which_logits_are_zero(size):
    plane, pos = tw.sweep(size)
    for ts in ws.TAPSETS[:1 if size == 128 else 2]:
        sd, G = shift(size, ts)
        e = tw.expected_impulse(G, plane, pos, 512) > 0
        for name, over in ws.tap_mutations(size, ts):
            Gm = ws.adjoint(ws.shift_state_dict(size, ts, tap_override=over), size, check=False)
            em = tw.expected_impulse(Gm, plane, pos, 512) > 0
            flips = int((e != em).sum())
            print(f"size {size} tap set {ts}: {name}: {flips} logits of the sweep change between zero and non-zero")
            assert flips > 0, name


# ---- the configurations of the GPU test ------------------------------------------------------------------------------------------------------------------------
def test_mixed_configurations_cover_every_lo_offset_state(pkg):
    """run_network hands an exact unit `lo offset 0 = read zeros` wherever its producer wrote one plane.  Over the mixed configurations of the GPU test, at both batch
    classes of its stale-plane runs, every such assignment is met in BOTH states: the stride-2 conv's x_lo (in_has_lo), block 0's conv2 x_lo / res_lo (the
    `ex1 && !ex0` branch), and layer0.1's conv1 x_lo / conv2 res_lo (b0_has_lo)."""
    pkg.build.build_lib()
    blob = ws.shift_blob(128, 0)
    assert len(ws.MIXED_128) == 13 and len({(w, x) for _, _, w, x, _ in ws.MIXED_128}) == 13
    seen = set()
    plans = {}
    for name, env, w2, x, _ in ws.MIXED_128:
        assert w2 & x == 0 and (w2 | x) != 0
        for n in ws.STALE_N:
            lines = ws.plan_lines(pkg, blob, 128, n, 0, w2, x, detail=True)
            ws.check_plan_arithmetic(lines, w2, x)
            plans[(name, n)] = [l.split(" {")[0] for l in lines]
            for role, conv, xl, rl in ws.lo_states(lines):
                stage0 = conv.endswith("32to32")
                seen.add((role, stage0, xl, rl))
                if role == "S2":
                    assert not rl
                if role == "B0C2":
                    assert xl == rl
                if role == "B1C1":
                    assert not rl and (xl or stage0)
                if role == "B1C2":
                    assert xl and (rl or stage0)
    want = {("S2", False, False, False), ("S2", False, True, False), ("B0C2", False, False, False), ("B0C2", False, True, True), ("B0C2", True, True, True),
            ("B1C1", True, False, False), ("B1C1", True, True, False), ("B1C1", False, True, False),
            ("B1C2", True, True, False), ("B1C2", True, True, True), ("B1C2", False, True, True)}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    # the two batch sizes of the stale-plane runs are two batch classes: some configuration launches other kernels for them
    assert any(plans[(name, ws.STALE_N[0])] != plans[(name, ws.STALE_N[1])] for name, *_ in ws.MIXED_128)
    # every w2 / x stage mask and unit mask of the list, and both illegal pairs avoided
    assert {w for _, e, w, x, _ in ws.MIXED_128 if x == 0} == {0x03, 0x0C, 0x30, 0xC0, 0x55, 0xFA}
    assert {x for _, e, w, x, _ in ws.MIXED_128 if x} == {0x30, 0x3C, 0x03, 0xC0, 0xF8, 0x54, 0x0A}
    assert sum(full for *_, full in ws.MIXED_128) == 2
