"""Input families at the thresholds of the flat-content guard, and the reference they are built against.

The guard's statistic is defined by the text of csrc/mlt_kernels.h (MLT_FLAT_RANGE, MLT_FLAT_EXACT_SHIFT): per CU, the number of aligned
4-pixel quads that are NEAR-FLAT and the number that are EXACTLY FLAT.  `scalar_quad_bits` restates one quad's two bits from that text in
plain Python integers; it calls nothing of the package and is the reference of everything below (tests/test_flat_guard_cpu.py holds the
package's numpy form, synth.flat_guard_flags, to it; tests/test_flat_guard_gpu.py holds the four device implementations to the flags).

Per CU size S: Q = S * S / 4 quads, T = Q // div exactly flat quads flag a CU (div = 8, or 16 for the tiers behind the magnitude guard and
the exact-lite tier), H = Q // 2 near-flat quads flag it too.  Every CU built here carries EXACTLY T or T - 1 (family E, family C) or H or
H - 1 (family N) counted quads on a background that counts nothing, so one quad dropped or counted twice anywhere changes a flag:

  E  exactly flat quads of four kinds (constant; org exactly linear with slope 3 / 6 / 12 over a constant residual; constant org over an
     exactly linear residual; org constant only after the clip to 10 bits), laid out by three orders of the Q positions -- a seeded
     permutation, row-major (whole rows flat, the first and the last row of the CU included), column-major (every row partly flat).  Per
     order `div` CUs of T quads on consecutive slices (together: every position exactly once) and the CUs of T - 1 quads it takes to cover
     every position again (div + 1 of them wherever (div + 1)(T - 1) >= Q, i.e. T > div: more at 16 x 16 and at 32 x 32 with div = 16).
  N  near-flat quads ON the rule's edges (range exactly 6 in both planes; second differences of exactly +-1 on a steep slope; one plane
     by range, the other by linearity), (T - 1) // 2 exactly flat ones among them, H (2 CUs per order) or H - 1 (3 CUs per order, covering
     every position); a quarter of the remaining background quads replaced by quads just OUTSIDE the rule (range 7 with second differences
     of 2 in one plane; one plane coherent, the other not).
  C  quads that are exactly flat only through the casts (negative int16 Pels are >= 32768 after the uint16 cast and clip to 1023; the
     residual is taken on the cast values before ITS clip), T and T - 1 of them in the permuted order; a quarter of the remaining
     background replaced by quads that only a signed restatement would call flat.
"""
from typing import NamedTuple

import numpy as np

FLAT_RANGE = 6            # mlt_kernels.h: MLT_FLAT_RANGE
LAYOUTS = ("perm", "rows", "cols")


# ---- the reference: one quad, plain integers, from the header's text ----------------------------------------------------------------
def _plane_bits(v0, v1, v2, v3, flat_range):
    """(near-flat, exactly flat) of one plane's four values."""
    lo01, hi01 = (v0, v1) if v0 < v1 else (v1, v0)
    lo23, hi23 = (v2, v3) if v2 < v3 else (v3, v2)
    rng = (hi01 if hi01 > hi23 else hi23) - (lo01 if lo01 < lo23 else lo23)      # max - min
    d1, d2 = v0 + v2 - 2 * v1, v1 + v3 - 2 * v2                                   # the two second differences
    return (rng <= flat_range or (-1 <= d1 <= 1 and -1 <= d2 <= 1),   # range <= 6, or linear to within one step
            rng == 0 or (d1 == 0 and d2 == 0))                          # constant, or exactly linear


def scalar_quad_bits(o4, p4, flat_range=FLAT_RANGE):
    """(near-flat, exactly flat) of the aligned quad with org Pels o4 and pred Pels p4 (four int16 values each, as Python ints).
    (Written out value by value: the GPU module runs it over 2.5 million quads.)"""
    o0, o1, o2, o3 = o4
    o0 &= 0xFFFF; o1 &= 0xFFFF; o2 &= 0xFFFF; o3 &= 0xFFFF             # "as the network sees them: uint16 cast,
    near_o, exact_o = _plane_bits(o0 if o0 < 1023 else 1023, o1 if o1 < 1023 else 1023, o2 if o2 < 1023 else 1023, o3 if o3 < 1023 else 1023,
                                  flat_range)                          # ... clip to 10 bits"
    if not near_o:
        return False, False           # the quad counts when BOTH planes do, and a plane that is not near-flat is not exactly flat either
    p0, p1, p2, p3 = p4
    r0, r1, r2, r3 = abs(o0 - (p0 & 0xFFFF)), abs(o1 - (p1 & 0xFFFF)), abs(o2 - (p2 & 0xFFFF)), abs(o3 - (p3 & 0xFFFF))   # absdiff of the CAST values,
    near_r, exact_r = _plane_bits(r0 if r0 < 1023 else 1023, r1 if r1 < 1023 else 1023, r2 if r2 < 1023 else 1023, r3 if r3 < 1023 else 1023,
                                  flat_range)                          # THEN its clip
    return near_r, near_r and exact_o and exact_r


def scalar_counts(org, pred, flat_range=FLAT_RANGE):
    """(near-flat count, exactly flat count) of ONE CU (two [S, S] int16 arrays), quad by quad with scalar_quad_bits."""
    o, p = org.tolist(), pred.tolist()
    near = exact = 0
    for ro, rp in zip(o, p):
        for x in range(0, len(ro), 4):
            nb, eb = scalar_quad_bits(ro[x:x + 4], rp[x:x + 4], flat_range)
            near += nb
            exact += eb
    return near, exact


def scalar_flag(near, exact, size, div):
    """guard_thresholds (csrc/mlt_guards.cpp): flagged when >= Q // div quads are exactly flat or >= Q // 2 near-flat."""
    q = size * size // 4
    return exact >= q // div or near >= q // 2


def thresholds(size, div):
    q = size * size // 4
    return q, q // div, q // 2


# ---- quads ---------------------------------------------------------------------------------------------------------------------------
class _Draws:
    """A seeded numpy Generator behind a pool of 32-bit words drawn in bulk (one Generator call per value costs more than the quad it fills)."""

    def __init__(self, seed):
        self.g = np.random.default_rng(seed)
        self.pool, self.at = [], 0

    def word(self):
        if self.at == len(self.pool):
            self.pool, self.at = self.g.integers(0, 1 << 32, 1 << 16).tolist(), 0
        self.at += 1
        return self.pool[self.at - 1]


def _ri(rng, lo, hi):
    """an integer in [lo, hi] (the modulo's bias, < 2^-20, does not matter here)"""
    return lo + rng.word() % (hi - lo + 1)


def _pred_for(org, res):
    """pred with |org - pred| = res, kept non-negative where it can be (no cast effects where none are meant)."""
    return [o - r if o - r >= 0 else o + r for o, r in zip(org, res)]


def _q_const(rng, k):
    return [_ri(rng, 0, 1023)] * 4, [_ri(rng, 0, 1023)] * 4


def _q_org_linear(rng, k):
    s = (3, 6, 12)[k % 3] * (1 if (k // 3) % 2 else -1)
    a = _ri(rng, 140, 860)
    org = [a + s * j for j in range(4)]
    return org, _pred_for(org, [_ri(rng, 0, 90)] * 4)


def _q_res_linear(rng, k):
    s = (3, 6, 12)[k % 3]
    r0 = _ri(rng, 0, 100)
    res = [r0 + s * j for j in range(4)]
    if (k // 3) % 2:
        res.reverse()
    c = _ri(rng, 300, 700)
    return [c] * 4, ([c - r for r in res] if (k // 6) % 2 else [c + r for r in res])


def _q_clip_const(rng, k):
    org = [1023, _ri(rng, 1024, 1999), _ri(rng, 1024, 1999), 2000]      # 1023 ... 2000: constant only after the clip
    j = _ri(rng, 0, 3)
    org = org[j:] + org[:j]
    if k % 2:
        return org, [0] * 4                                             # residual = org >= 1023: constant after ITS clip
    r = _ri(rng, 0, 1023)
    return org, [o - r for o in org]                                    # residual r on the unclipped values


_R6 = ([0, 6, 0, 6], [6, 0, 5, 1], [0, 6, 6, 0], [3, 0, 6, 2], [6, 2, 0, 4])   # range exactly 6, second differences >= 4 in magnitude


def _range6(rng, k, lo, hi):
    c = _ri(rng, lo, hi)
    return [c + v for v in _R6[k % len(_R6)]]


def _steep(rng, k, lo, hi):
    """second differences exactly +1 / -1 (or -1 / +1) on a slope of 20 ... 60 per pixel: range >= 61."""
    s, e = _ri(rng, 20, 60), (1 if k % 2 else -1)
    v = [0, s, 2 * s + e, 3 * s + e]
    if (k // 2) % 2:
        v.reverse()
    a = _ri(rng, lo, hi - max(v))
    return [a + x for x in v]


def _q_range6(rng, k):
    org = _range6(rng, k, 200, 800)
    return org, _pred_for(org, _range6(rng, k + 2, 0, 150))


def _q_steep(rng, k):
    org = _steep(rng, k, 200, 800)
    return org, _pred_for(org, _steep(rng, k + 1, 0, 200))


def _q_mixed(rng, k):
    if k % 2:
        org = _steep(rng, k // 2, 200, 800)
        return org, _pred_for(org, _range6(rng, k // 2, 0, 150))
    org = _range6(rng, k // 2, 200, 800)
    return org, _pred_for(org, _steep(rng, k // 2, 0, 200))


def _q_out_range7(rng, k):
    pat = [0, 3, 4, 7] if (k // 2) % 2 else [7, 4, 3, 0]                # range exactly 7, second differences exactly -2 / +2
    if k % 2:
        c, r = _ri(rng, 200, 800), _ri(rng, 0, 150)
        return [c] * 4, _pred_for([c] * 4, [r + v for v in pat])
    c = _ri(rng, 200, 800)
    org = [c + v for v in pat]
    return org, _pred_for(org, [_ri(rng, 0, 150)] * 4)


def _wild(rng):
    while True:
        v = [_ri(rng, 0, 1023) for _ in range(4)]
        d1, d2 = v[0] + v[2] - 2 * v[1], v[1] + v[3] - 2 * v[2]
        if max(v) - min(v) > 40 and max(abs(d1), abs(d2)) > 8:
            return v


def _q_out_one_plane(rng, k):
    if k % 2:
        c = _ri(rng, 0, 1023)
        res = _wild(rng)
        return [c] * 4, [c - r if c - r >= 0 else c + r for r in res]   # org constant, residual incoherent
    org = _wild(rng)
    return org, _pred_for(org, [_ri(rng, 0, 150)] * 4)                  # org incoherent, residual constant


_NEG = (-1, -5, -300, -32768, -2, -1000, -77, -20000)


def _q_cast(rng, k):
    v = k % 3
    if v == 0:                                                           # negative org over pred = 0: both planes 1023 after the clips
        return [_NEG[(k + j * 3) % len(_NEG)] for j in range(4)], [0] * 4
    if v == 1:                                                           # negative org (1023 after cast and clip), residual constant on the cast values
        org = [-_ri(rng, 1, 2000) for _ in range(3)] + [-1]
        r = _ri(rng, 0, 500)
        return org, [o - r for o in org]
    c = _ri(rng, 0, 1023)                                                # constant org, negative pred: residual >= 62000 -> 1023
    return [c] * 4, [-_ri(rng, 1, 2000) for _ in range(3)] + [-2000]


def _q_out_signed(rng, k):
    """flat for a restatement that treats the Pels as signed, not flat through the uint16 cast."""
    org = [-1, 0, -1, 0] if k % 2 else [0, -1, -1, 0]
    r = _ri(rng, 1, 50)
    return org, [o - r for o in org]


EXACT_KINDS = (_q_const, _q_org_linear, _q_res_linear, _q_clip_const)
NEAR_KINDS = (_q_range6, _q_steep, _q_mixed)
OUTSIDE_KINDS = (_q_out_range7, _q_out_one_plane)


def _make(kinds, rng, k, want):
    o4, p4 = kinds[k % len(kinds)](rng, k // len(kinds))
    assert -32768 <= min(o4 + p4) and max(o4 + p4) <= 32767, (kinds[k % len(kinds)].__name__, o4, p4)
    assert scalar_quad_bits(o4, p4) == want, (kinds[k % len(kinds)].__name__, k, o4, p4, scalar_quad_bits(o4, p4), want)
    return o4, p4


# ---- CUs -----------------------------------------------------------------------------------------------------------------------------
def layout_order(size, layout, rng):
    """The Q quad positions (index = row * S / 4 + quad column) in the layout's order."""
    q, qr = size * size // 4, size // 4
    if layout == "perm":
        return rng.g.permutation(q)
    if layout == "rows":
        return np.arange(q)
    assert layout == "cols"
    return np.arange(q).reshape(size, qr).T.reshape(-1)


def _window(order, start, count):
    return order[(start + np.arange(count)) % len(order)]


def _background(size, rng):
    return rng.g.integers(0, 1024, (size, size)).astype(np.int16), rng.g.integers(0, 1024, (size, size)).astype(np.int16)


def _put(org, pred, pos, o4, p4):
    y, x = divmod(int(pos), org.shape[0] // 4)
    org[y, 4 * x:4 * x + 4] = o4
    pred[y, 4 * x:4 * x + 4] = p4


def _cu(bg, rng, order, start, n_exact, n_near_only, exact_kinds, outside_kinds):
    """One CU: the background bg (which counts nothing); n_exact exactly flat quads and n_near_only near-flat, not exactly flat ones on the
    positions order[start ...] (wrapping); with outside_kinds, every fourth of the other positions holds a quad just outside the rule."""
    org, pred = bg[0].copy(), bg[1].copy()
    count = n_exact + n_near_only
    win = _window(order, start, count)
    assert len(set(win.tolist())) == count
    step = max(count // max(n_exact, 1), 1)
    is_exact = np.zeros(count, bool)
    is_exact[np.arange(n_exact) * step % count if n_near_only else np.arange(n_exact)] = True
    assert is_exact.sum() == n_exact
    ke = kn = 0
    for j, pos in enumerate(win):
        if is_exact[j]:
            _put(org, pred, pos, *_make(exact_kinds, rng, ke, (True, True)))
            ke += 1
        else:
            _put(org, pred, pos, *_make(NEAR_KINDS, rng, kn, (True, False)))
            kn += 1
    if outside_kinds:
        rest = _window(order, start + count, len(order) - count)[::4]
        for k, pos in enumerate(rest):
            _put(org, pred, pos, *_make(outside_kinds, rng, k, (False, False)))
    return org, pred, win


class Family(NamedTuple):
    size: int
    div: int
    org: np.ndarray      # [n, S, S] int16
    pred: np.ndarray
    near: np.ndarray     # [n] intended near-flat count (asserted with the scalar reference at construction)
    exact: np.ndarray    # [n] intended exactly flat count
    flagged: np.ndarray  # [n] scalar_flag of the two
    label: tuple         # [n] "family/layout/count#index seed s"

    def __len__(self):
        return len(self.label)


def _family(size, div, seed, numpy_counts, families=("E", "N", "C")):
    q, t, h = thresholds(size, div)
    assert t * div == q and t >= 2 and h > t
    cus = []   # (org, pred, near, exact, label)

    def add(fam, layout, what, i, rng, order, bg, start, n_exact, n_near_only, exact_kinds, outside_kinds):
        org, pred, win = _cu(bg, rng, order, start, n_exact, n_near_only, exact_kinds, outside_kinds)
        want = (n_exact + n_near_only, n_exact)
        label = f"{fam}/{layout}/{what}#{i} size {size} div {div} seed {seed}"
        got = scalar_counts(org, pred)
        assert got == want, (label, got, want)
        cus.append((org, pred, want[0], want[1], label))
        return set(win.tolist())

    for li, layout in enumerate(LAYOUTS):
        rng = _Draws([seed, size, div, li])
        order = layout_order(size, layout, rng)
        bg = _background(size, rng)        # one background per layout and seed: 10-bit uniform Pels in both planes
        assert scalar_counts(*bg) == (0, 0), "the background must count nothing"
        everything = set(range(q))
        if "E" in families:
            seen = []
            for i in range(div):
                seen.append(add("E", layout, "T", i, rng, order, bg, i * t, t, 0, EXACT_KINDS, None))
            assert sum(len(s) for s in seen) == q and set().union(*seen) == everything, "the T CUs cover every quad position exactly once"
            m = max(div + 1, -(-q // (t - 1)))
            seen = [add("E", layout, "T-1", i, rng, order, bg, i * (t - 1), t - 1, 0, EXACT_KINDS, None) for i in range(m)]
            assert set().union(*seen) == everything, "the T - 1 CUs cover every quad position"
        if "N" in families:
            nex = (t - 1) // 2
            seen = [add("N", layout, "H", i, rng, order, bg, i * h, nex, h - nex, EXACT_KINDS, OUTSIDE_KINDS) for i in range(2)]
            assert set().union(*seen) == everything
            seen = [add("N", layout, "H-1", i, rng, order, bg, i * (h - 1), nex, h - 1 - nex, EXACT_KINDS, OUTSIDE_KINDS) for i in range(3)]
            assert set().union(*seen) == everything
        if "C" in families and layout == "perm":
            for i in range(2):
                add("C", layout, "T", i, rng, order, bg, i * t + t // 2, t, 0, (_q_cast,), (_q_out_signed,))
            for i in range(2):
                add("C", layout, "T-1", i, rng, order, bg, i * t + t // 3, t - 1, 0, (_q_cast,), (_q_out_signed,))
    org = np.stack([c[0] for c in cus])
    pred = np.stack([c[1] for c in cus])
    near = np.array([c[2] for c in cus], np.int64)
    exact = np.array([c[3] for c in cus], np.int64)
    flagged = np.array([scalar_flag(c[2], c[3], size, div) for c in cus], bool)
    # the intended flags: T and H CUs are flagged, T - 1 and H - 1 CUs are not (near <= T < H in E and C; exact < T in N)
    for c, f in zip(cus, flagged):
        assert f == ("/T#" in c[4] or "/H#" in c[4]), c[4]
    # the package's numpy restatement returns the same integers
    n_near, n_exact, n_flag = numpy_counts(org, pred, div)
    bad = np.flatnonzero((n_near != near) | (n_exact != exact) | (n_flag != flagged))
    assert bad.size == 0, [(cus[i][4], int(n_near[i]), int(n_exact[i]), bool(n_flag[i])) for i in bad[:8]]
    return Family(size, div, org, pred, near, exact, flagged, tuple(c[4] for c in cus))


_CACHE = {}


def family(pkg, size, div, seed=0, families=("E", "N", "C")):
    """All CUs of the named families at (size, div) under `seed` (built once per process; treat the arrays as read-only)."""
    key = (size, div, seed, tuple(families))
    if key not in _CACHE:
        _CACHE[key] = _family(size, div, seed, lambda o, p, d: pkg.synth.flat_guard_flags(o, p, flat_div=d, flat_range=FLAT_RANGE), families)
        for a in _CACHE[key][2:7]:
            a.setflags(write=False)
    return _CACHE[key]


def batch(pkg, size, div, n, seed=0, shuffle_seed=1):
    """n CUs: the families under seed, seed + 1, ... until there are n, in a seeded shuffled order (flagged and unflagged CUs alternate)."""
    parts, total, s = [], 0, seed
    while total < n:
        parts.append(family(pkg, size, div, s))
        total += len(parts[-1])
        s += 1
    perm = np.random.default_rng([shuffle_seed, size, div, n]).permutation(total)[:n]
    cat = lambda k: np.concatenate([getattr(p, k) for p in parts])[perm]
    labels = [l for p in parts for l in p.label]
    out = Family(size, div, cat("org"), cat("pred"), cat("near"), cat("exact"), cat("flagged"), tuple(labels[i] for i in perm))
    for a in out[2:7]:
        a.setflags(write=False)
    return out
