"""CPU: quarter-sample refinement and per-block reference choice -- the host side of mlt_picture_predict_refs / mlt_picture_compensate_refs (exports, the 24-byte
config, the NULL-context paths) and the numpy restatement motion.refine / compensate_refs / predict_refs against an INDEPENDENT brute force built only from the
already tested motion.compensate and motion.search: every candidate compensates the whole picture with the field mv0 + q, per-block sums of |cur - P| follow, and
the key is formed in Python integers.  Integer arithmetic only: every comparison is equality."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MLT_ERR_ARG = 1
NEW = ("mlt_picture_predict_refs", "mlt_picture_compensate_refs")
WD = {0: (0,), 1: (-2, 0, 2), 2: (-3, -2, -1, 0, 1, 2, 3)}
GEOMETRIES = [(72, 40, 16, 4), (45, 29, 8, 3), (136, 80, 64, 2), (80, 48, 32, 4)]   # width, height, block, range
TAPS = ((0, 0, 0, 64, 0, 0, 0, 0), (-1, 4, -10, 58, 17, -5, 1, 0), (-1, 4, -11, 40, 40, -11, 4, -1), (0, 1, -5, 17, 58, -10, 4, -1))


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build.build_lib()
    return pkg.capi.load_library()


@pytest.fixture(scope="module")
def motion(pkg):
    return pkg.motion


def test_new_names_are_declared_and_exported(pkg, lib):
    header = open(os.path.join(ROOT, "include", "mltcnn.h")).read()
    declared = set(re.findall(r"\b(mlt_[a-z_0-9]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in pkg.capi.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert lib.mlt_abi_version() == 4
    assert C.sizeof(pkg.capi.MltMotionRefsConfig) == 24 and C.sizeof(pkg.capi.MltMotionConfig) == 20
    assert "typedef struct mlt_motion_refs_config {   /* 24 bytes */" in header
    assert "#define MLT_MOTION_MAX_REFS 4" in header and pkg.capi.MOTION_MAX_REFS == pkg.motion.MAX_REFS == 4
    assert pkg.motion.WINDOWS == (WD[0], WD[1], WD[2])
    for doc in ("include/mltcnn.h", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read().replace("**", "")
        assert "Not there: sub-sample search" not in text, doc


def test_null_context_calls_touch_nothing(pkg, lib):
    cfg = pkg.capi.motion_refs_config(16, 4, 0, 2)
    mv = np.full((1, 1, 2), 5, np.int16)
    ref = np.full((1, 1), 3, np.uint8)
    cost = np.full((1, 1), 9, np.uint32)
    refs = (C.c_void_p * 1)(None)
    assert lib.mlt_picture_predict_refs(None, None, refs, 1, C.byref(cfg), None, mv.ctypes.data, ref.ctypes.data, cost.ctypes.data) == MLT_ERR_ARG
    assert lib.mlt_picture_compensate_refs(None, refs, 1, C.byref(cfg), mv.ctypes.data, ref.ctypes.data, None) == MLT_ERR_ARG
    assert (mv == 5).all() and (ref == 3).all() and (cost == 9).all()


# ---- content ----
def _noise(shape, seed, lo=-300, hi=1500):
    return np.random.default_rng(seed).integers(lo, hi, size=shape).astype(np.int16)


def _smooth(shape, rng):
    """Standard normal noise filtered by [1, 4, 6, 4, 1] / 16 along both axes, scaled to about -40 .. 1060: a few samples lie outside 0 .. 1023."""
    h, w = shape
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    a = rng.standard_normal((h + 4, w + 4))
    a = sum(k[i] * a[i:i + h, :] for i in range(5))
    a = sum(k[i] * a[:, i:i + w] for i in range(5))
    a = (a - a.min()) / (a.max() - a.min())
    return np.round(-40 + 1100 * a).astype(np.int16)


def _block_sums(a, block):
    h, w = a.shape
    return np.add.reduceat(np.add.reduceat(a, np.arange(0, h, block), axis=0), np.arange(0, w, block), axis=1)


# ---- the brute force: existing compensate and search only, Python-integer keys ----
def _sadp_volumes(motion, cur, refs, block, R, lam):
    """-> (mv0 [n_refs, by, bx, 2], {(r, qx, qy): int64 [by, bx] SADP}) over the 49 candidates of subpel 2 (the windows of subpel 0 and 1 are subsets)."""
    c = cur.astype(np.int64)
    mv0 = np.stack([motion.search(cur, ref, block, R, lam)[0] for ref in refs])
    vol = {}
    for r, ref in enumerate(refs):
        for qy in WD[2]:
            for qx in WD[2]:
                p = motion.compensate(ref, (mv0[r] + np.array([qx, qy], np.int16)).astype(np.int16), block)
                vol[(r, qx, qy)] = _block_sums(np.abs(c - p.astype(np.int64)), block)
    return mv0, vol


def _brute_pick(mv0, vol, n_refs, subpel, lam):
    _, by, bx, _ = mv0.shape
    mv, ref, cost = np.zeros((by, bx, 2), np.int16), np.zeros((by, bx), np.uint8), np.zeros((by, bx), np.uint32)
    for j in range(by):
        for i in range(bx):
            best = None
            for r in range(n_refs):
                for qy in WD[subpel]:
                    for qx in WD[subpel]:
                        mvx, mvy = int(mv0[r, j, i, 0]) + qx, int(mv0[r, j, i, 1]) + qy
                        l1 = abs(mvx) + abs(mvy)
                        cq = 4 * int(vol[(r, qx, qy)][j, i]) + lam * l1
                        assert cq < 2 ** 32 and l1 <= 518 and abs(mvx) <= 259 and abs(mvy) <= 259
                        key = (cq << 32) | (l1 << 22) | (r << 20) | ((mvy + 512) << 10) | (mvx + 512)
                        assert (best is None or key != best[0])
                        if best is None or key < best[0]:
                            best = (key, (cq, l1, r, mvy, mvx))
            # the packed key orders like the tuple of the rule
            cq, l1, r, mvy, mvx = best[1]
            mv[j, i], ref[j, i], cost[j, i] = (mvx, mvy), r, cq
    return mv, ref, cost


def _refs_for(motion, w, h, block, seed):
    """cur and three references: smooth content moved by a whole-sample part (the crops) and a fraction (5, -6 quarter samples), the references disturbed
    differently so that the choice among them varies."""
    rng = np.random.default_rng(seed)
    base = _smooth((h + 8, w + 8), rng)
    bx, by = motion.blocks(w, h, block)
    cur = motion.compensate(base[4:4 + h, 4:4 + w].copy(), np.tile(np.array([5, -6], np.int16), (by, bx, 1)), block)
    refs = [base[3:3 + h, 5:5 + w].copy(), base[4:4 + h, 2:2 + w].copy(), base[6:6 + h, 4:4 + w].copy()]
    refs[0][: h // 2] += rng.integers(-30, 31, size=(h // 2, w)).astype(np.int16)    # reference 0 worse in the upper half
    refs[1][:, w // 2:] += rng.integers(-30, 31, size=(h, w - w // 2)).astype(np.int16)
    return cur, refs


@pytest.fixture(scope="module")
def volumes(motion):
    """The brute-force SADP volumes, once per (geometry, lambda), shared by the tests below and left unchanged."""
    out = {}
    for g, (w, h, block, R) in enumerate(GEOMETRIES):
        cur, refs = _refs_for(motion, w, h, block, 300 + g)
        for lam in (0, 4):
            out[(g, lam)] = (cur, refs) + _sadp_volumes(motion, cur, refs, block, R, lam)
    return out


@pytest.mark.parametrize("n_refs", [1, 3])
@pytest.mark.parametrize("lam", [0, 4])
@pytest.mark.parametrize("subpel", [0, 1, 2])
@pytest.mark.parametrize("g", range(4), ids=["%dx%d_b%d_r%d" % c for c in GEOMETRIES])
def test_refine_against_the_brute_force(motion, volumes, g, subpel, lam, n_refs):
    w, h, block, R = GEOMETRIES[g]
    cur, refs, mv0, vol = volumes[(g, lam)]
    want = _brute_pick(mv0, vol, n_refs, subpel, lam)
    got = motion.refine(cur, refs[:n_refs], mv0[:n_refs], block, lam, subpel)
    assert got[0].dtype == np.int16 and got[1].dtype == np.uint8 and got[2].dtype == np.uint32
    for a, b, what in zip(got, want, ("mv", "ref", "cost")):
        assert np.array_equal(a, b), (what, np.argwhere(a != b)[:4])
    plane, mv, ref, cost = motion.predict_refs(cur, refs[:n_refs], block, R, lam, subpel)
    assert np.array_equal(mv, want[0]) and np.array_equal(ref, want[1]) and np.array_equal(cost, want[2])
    # step 4: block by block the winner's compensation
    full = [motion.compensate(r, mv, block) for r in refs[:n_refs]]
    sel = np.repeat(np.repeat(ref, block, 0), block, 1)[:h, :w]
    assert np.array_equal(plane, np.choose(sel, full)) and np.array_equal(plane, motion.compensate_refs(refs[:n_refs], mv, ref, block))
    if n_refs == 3 and subpel == 2 and lam == 0 and block < 64:   # (136 x 80 has six blocks of 64: one reference takes them all)
        assert len(np.unique(ref)) >= 2 and ((mv & 3) != 0).any(), "the case exercises neither the reference choice nor a fraction"


def _scalar_refs(cur, refs, block, R, lam, subpel):
    """The rule word for word on a tiny picture: scalar loops, tuples compared lexicographically, no packed key, no call into motion.py."""
    H, W = cur.shape

    def Rf(ref, x, y):
        return int(ref[min(max(y, 0), H - 1), min(max(x, 0), W - 1)])

    def P(ref, x, y, mvx, mvy):
        ix, fx, iy, fy = mvx >> 2, mvx & 3, mvy >> 2, mvy & 3
        v = sum(TAPS[fy][j] * sum(TAPS[fx][k] * Rf(ref, x + ix + k - 3, y + iy + j - 3) for k in range(8)) for j in range(8))
        return min(max((v + 2048) >> 12, 0), 1023)

    by, bx = -(-H // block), -(-W // block)
    mv, idx, cost = np.zeros((by, bx, 2), np.int16), np.zeros((by, bx), np.uint8), np.zeros((by, bx), np.uint32)
    plane = np.zeros((H, W), np.int16)
    for j in range(by):
        for i in range(bx):
            pix = [(x, y) for y in range(j * block, min((j + 1) * block, H)) for x in range(i * block, min((i + 1) * block, W))]
            best = None
            for r, ref in enumerate(refs):
                integer = min((sum(abs(int(cur[y, x]) - Rf(ref, x + dx, y + dy)) for x, y in pix) + lam * (abs(dx) + abs(dy)), abs(dx) + abs(dy), dy, dx)
                              for dy in range(-R, R + 1) for dx in range(-R, R + 1))
                for qy in WD[subpel]:
                    for qx in WD[subpel]:
                        mvx, mvy = 4 * integer[3] + qx, 4 * integer[2] + qy
                        sadp = sum(abs(int(cur[y, x]) - P(ref, x, y, mvx, mvy)) for x, y in pix)
                        key = (4 * sadp + lam * (abs(mvx) + abs(mvy)), abs(mvx) + abs(mvy), r, mvy, mvx)
                        best = key if best is None or key < best else best
            mv[j, i], idx[j, i], cost[j, i] = (best[4], best[3]), best[2], best[0]
            for x, y in pix:
                plane[y, x] = P(refs[best[2]], x, y, best[4], best[3])
    return plane, mv, idx, cost


def test_predict_refs_against_a_scalar_loop(motion):
    rng = np.random.default_rng(77)
    base = _smooth((9 + 4, 13 + 4), rng)
    cur = base[2:11, 2:15].copy()
    refs = [base[1:10, 3:16] + rng.integers(-3, 4, size=(9, 13)).astype(np.int16), base[2:11, 1:14].copy()]
    for lam in (0, 2):
        want = _scalar_refs(cur, refs, 8, 1, lam, 2)
        got = motion.predict_refs(cur, refs, 8, 1, lam, 2)
        for a, b, what in zip(got, want, ("plane", "mv", "ref", "cost")):
            assert np.array_equal(a, b), (lam, what)


# ---- designed cases ----
def test_constant_pictures_give_the_zero_vector_of_reference_zero(motion):
    cur = np.full((40, 72), 517, np.int16)
    for lam in (0, 4):
        plane, mv, ref, cost = motion.predict_refs(cur, [cur.copy(), cur.copy(), cur.copy()], 16, 4, lam, 2)
        assert not mv.any() and not ref.any() and not cost.any() and np.array_equal(plane, cur)


def test_identical_references_give_reference_zero(motion):
    ref = _smooth((40, 72), np.random.default_rng(3))
    cur = _smooth((40, 72), np.random.default_rng(4))
    plane, mv, idx, cost = motion.predict_refs(cur, [ref, ref.copy()], 16, 4, 4, 2)
    one = motion.predict_refs(cur, [ref], 16, 4, 4, 2)
    assert not idx.any() and np.array_equal(mv, one[1]) and np.array_equal(cost, one[3]) and np.array_equal(plane, one[0])


def test_cost_q_is_on_clipped_samples(motion):
    ref = _noise((40, 72), 5)          # -300 .. 1500: samples below 0 and above 1023 in every block
    cur = _noise((40, 72), 6)
    assert ref.min() < 0 and ref.max() > 1023 and cur.min() < 0 and cur.max() > 1023
    mv_i, cost_i = motion.search(cur, ref, 16, 4, 4)
    _, mv, _, cost_q = motion.predict_refs(cur, [ref], 16, 4, 4, 0)
    assert np.array_equal(mv, mv_i) and (cost_q != 4 * cost_i.astype(np.int64)).all()
    inside = np.clip(ref, 0, 1023)     # ... and 4 x the integer cost when no reference sample is clipped
    mv_i, cost_i = motion.search(cur, inside, 16, 4, 4)
    _, mv, _, cost_q = motion.predict_refs(cur, [inside], 16, 4, 4, 0)
    assert np.array_equal(mv, mv_i) and np.array_equal(cost_q.astype(np.int64), 4 * cost_i.astype(np.int64))   # lam |mv| = 4 lam (|dx| + |dy|)


@pytest.mark.parametrize("g", range(4), ids=["%dx%d_b%d_r%d" % c for c in GEOMETRIES])
def test_integer_window_and_one_reference_is_predict(motion, g):
    w, h, block, R = GEOMETRIES[g]
    cur, refs = _refs_for(motion, w, h, block, 400 + g)
    for lam in (0, 4):
        plane, mv, _ = motion.predict(cur, refs[0], block, R, lam)
        got = motion.predict_refs(cur, refs[:1], block, R, lam, 0)
        assert np.array_equal(got[0], plane) and np.array_equal(got[1], mv) and not got[2].any()


def test_planted_fields_are_recovered(motion):
    rng = np.random.default_rng(5)
    for w, h, block, R in GEOMETRIES:
        ref = _smooth((h, w), rng)
        assert ref.min() < 0 and ref.max() > 1023
        bx, by = motion.blocks(w, h, block)
        planted = rng.integers(-4 * R + 3, 4 * R - 3 + 1, size=(by, bx, 2)).astype(np.int16)
        cur = motion.compensate(ref, planted, block)
        plane, mv, idx, cost = motion.predict_refs(cur, [ref], block, R, 0, 2)
        hit = (mv == planted).all(axis=2) & (cost == 0)
        print(f"{w}x{h} block {block} range {R}: {int(hit.sum())}/{hit.size} planted vectors recovered, {int(((planted & 3) != 0).any(axis=2).sum())} fractional")
        assert hit.sum() >= 0.9 * hit.size, (w, h, block, int(hit.sum()), hit.size)
        assert np.array_equal(plane[np.repeat(np.repeat(hit, block, 0), block, 1)[:h, :w]], cur[np.repeat(np.repeat(hit, block, 0), block, 1)[:h, :w]])


def test_compensate_refs_table(motion):
    refs = [_noise((45, 77), 50 + r) for r in range(4)]
    bx, by = motion.blocks(77, 45, 16)
    rng = np.random.default_rng(8)
    mv = rng.integers(-40, 41, size=(by, bx, 2)).astype(np.int16)
    idx = (np.arange(by * bx) % 4).astype(np.uint8).reshape(by, bx)
    got = motion.compensate_refs(refs, mv, idx, 16)
    for j in range(by):
        for i in range(bx):
            ys, xs = slice(16 * j, min(16 * j + 16, 45)), slice(16 * i, min(16 * i + 16, 77))
            assert np.array_equal(got[ys, xs], motion.compensate(refs[idx[j, i]], mv, 16)[ys, xs])
    assert np.array_equal(motion.compensate_refs(refs, mv, None, 16), motion.compensate(refs[0], mv, 16))
    with pytest.raises(AssertionError):
        motion.compensate_refs(refs[:2], mv, idx, 16)


# ---- tools/picture_map.py --motion-refine ----
def test_picture_map_motion_refine_option():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import picture_map as pm
    assert pm.parse_motion_refine("2") == (2, 1) and pm.parse_motion_refine("1,4") == (1, 4) and pm.parse_motion_refine("0,2") == (0, 2)
    for bad in ("3", "-1", "2,0", "2,5", "a", "2,2,2", ""):
        with pytest.raises(ValueError):
            pm.parse_motion_refine(bad)
    base = ["o.npy", "r.npy", "--synthetic", "10", "--out", "x"]
    assert pm.parse_args(base + ["--motion", "8,4,2"]).motion_cfg == (8, 4, 2)            # unchanged: three entries, the integer call
    assert pm.parse_args(base + ["--motion", "8,4,2", "--motion-refine", "2,3"]).motion_cfg == (8, 4, 2, 2, 3)
    assert pm.parse_args(base + ["--motion", "16,4", "--motion-refine", "1"]).motion_cfg == (16, 4, 0, 1, 1)
    frames = np.arange(4 * 2 * 2, dtype=np.int16).reshape(4, 2, 2)
    lists = pm.motion_reference_lists(frames, 3)
    assert [[int(r[0, 0]) for r in refs] for refs in lists] == [[0, 0, 0], [0, 0, 0], [4, 0, 0], [8, 4, 0]]   # f - 1, f - 2, f - 3, clipped at frame 0
    assert [len(refs) for refs in pm.motion_reference_lists(frames[1], 2)] == [2]


def test_picture_map_refuses_motion_refine_without_motion():
    tool = os.path.join(ROOT, "tools", "picture_map.py")
    args = [sys.executable, tool, "o.npy", "r.npy", "--synthetic", "10", "--out", "x"]
    r = subprocess.run(args + ["--motion-refine", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--motion-refine" in r.stderr and "--motion" in r.stderr
    r = subprocess.run(args + ["--motion", "16,4", "--motion-refine", "3"], capture_output=True, text=True)
    assert r.returncode == 2 and "--motion-refine" in r.stderr
