"""GPU (MI355X): quarter-sample refinement and per-block reference choice -- mlt_picture_predict_refs and mlt_picture_compensate_refs against the numpy restatement
motion.predict_refs / compensate_refs (itself held to an independent brute force and to scalar loops by tests/test_motion_refs_cpu.py), and against the library's
own earlier calls.  The rule is integer arithmetic, so EVERY assertion is byte equality or an integer inequality; no tolerance appears anywhere in this file.

Shapes: 77 x 45 for blocks 8 and 16 (odd width, a clipped block width of 13 resp. 5, cut store items, clipped bottom blocks) and 80 x 72 for block 64, where only
one block is complete.  Range 3 or 4."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MLT_ERR_ARG = 1
W, H = 77, 45
CASES = [(77, 45, 8, 3), (77, 45, 16, 4), (80, 72, 64, 3)]   # width, height, block, range
IDS = ["%dx%d_b%d_r%d" % c for c in CASES]


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


def _blobs(pkg):
    return {s: pkg.weights.synthetic_blob(pkg.synth.ARCH_CU, 13) for s in (32, 16)}


@pytest.fixture(scope="module")
def ctx(gpu):
    m = gpu.MltCnn(device=0, sizes=(32, 16), blobs=_blobs(gpu), head_index={32: 0, 16: 0})
    yield m
    m.close()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _noise(shape, seed, lo=-300, hi=1500):
    """Seeded noise with pels outside 0 .. 1023 on both sides."""
    return np.random.default_rng(seed).integers(lo, hi, size=shape).astype(np.int16)


def _smooth(shape, seed):
    """Standard normal noise filtered by [1, 4, 6, 4, 1] / 16 along both axes, scaled to about -40 .. 1060."""
    h, w = shape
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    a = np.random.default_rng(seed).standard_normal((h + 4, w + 4))
    a = sum(k[i] * a[i:i + h, :] for i in range(5))
    a = sum(k[i] * a[:, i:i + w] for i in range(5))
    a = (a - a.min()) / (a.max() - a.min())
    return np.round(-40 + 1100 * a).astype(np.int16)


def _shifted(ref, sx, sy):
    h, w = ref.shape
    ys, xs = np.mgrid[0:h, 0:w]
    return ref[np.clip(ys + sy, 0, h - 1), np.clip(xs + sx, 0, w - 1)]


def _wrap(m, arr2d, offset_elems, pitch):
    """arr2d as a wrapped picture: a torch int16 tensor of offset_elems + H * pitch elements of seeded noise, the plane starting at element offset_elems."""
    import torch
    h, w = arr2d.shape
    host = np.random.default_rng(99).integers(0, 1024, size=offset_elems + h * pitch).astype(np.int16)
    host[offset_elems:offset_elems + h * pitch].reshape(h, pitch)[:, :w] = arr2d
    t = torch.from_numpy(host).to(torch.device("cuda", 0))
    return m.wrap_picture(t.data_ptr() + 2 * offset_elems, pitch, w, h, keep=t)


def _pictures(m, *planes):
    return [m.picture(p.shape[1], p.shape[0]).upload(p) for p in planes]


def _close(*pics):
    for p in pics:
        p.close()


def _contents(pkg, w, h, block, R, kind, seed):
    """-> (cur, [four references])."""
    rng = np.random.default_rng(seed)
    if kind == "planted":     # cur is the compensation of reference 0 with a planted quarter-sample field; the other references are disturbed copies and shifts
        ref = _smooth((h, w), seed)
        bx, by = pkg.motion.blocks(w, h, block)
        planted = rng.integers(-4 * R + 3, 4 * R - 3 + 1, size=(by, bx, 2)).astype(np.int16)
        cur = pkg.motion.compensate(ref, planted, block)
        r1 = ref.copy()
        r1[: h // 2] += rng.integers(-20, 21, size=(h // 2, w)).astype(np.int16)
        r0 = ref.copy()
        r0[h // 2:] += rng.integers(-20, 21, size=(h - h // 2, w)).astype(np.int16)
        return cur, [r0, r1, _shifted(ref, 1, -1).copy(), ref.copy()]
    if kind == "noise":
        return _noise((h, w), seed), [_noise((h, w), seed + 1 + r) for r in range(4)]
    if kind == "constant":
        c = np.full((h, w), 517, np.int16)
        return c, [c.copy() for _ in range(4)]
    assert kind == "borders"  # cur is reference r moved by (-R, 0), (R, 0), (0, -R), (0, R): the winners point across the left / right / top / bottom border and the
    ref = _smooth((h, w), seed)   # windows are clamped there.  Reference r is left clean only near ITS border, so each of them is chosen where it matters
    cur = _shifted(ref, -R, 0)
    refs = [ref.copy(), _shifted(ref, -2 * R, 0).copy(), _shifted(ref, -R, R).copy(), _shifted(ref, -R, -R).copy()]
    ys, xs = np.mgrid[0:h, 0:w]
    middle = (xs >= w // 4) & (xs < 3 * w // 4)
    clean = [xs < w // 4, xs >= 3 * w // 4, middle & (ys < h // 2), middle & (ys >= h // 2)]
    for r in range(4):
        refs[r] = np.where(clean[r], refs[r], refs[r] + rng.integers(-25, 26, size=(h, w)).astype(np.int16)).astype(np.int16)
    return cur, refs


_WANT = {}


def _want(pkg, key, cur, refs, block, R, lam, subpel):
    """The restatement, computed once per case and shared."""
    if key not in _WANT:
        _WANT[key] = pkg.motion.predict_refs(cur, refs, block, R, lam, subpel)
    return _WANT[key]


@pytest.mark.parametrize("kind", ["planted", "noise", "constant", "borders"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_predict_refs_equals_the_restatement(gpu, ctx, case, kind):
    pkg, m = gpu, ctx
    w, h, block, R = case
    cur, refs = _contents(pkg, w, h, block, R, kind, 500 + block)
    p_cur, *p_refs = _pictures(m, cur, *refs)
    dst, dst2 = _pictures(m, np.full((h, w), -1, np.int16), np.full((h, w), -2, np.int16))
    fractional, chosen = False, set()
    try:
        for n_refs in (1, 2, 4):
            for subpel in (0, 1, 2):
                for lam in (0, 4):
                    what = (case, kind, n_refs, subpel, lam)
                    plane, mv, ref, cost = _want(pkg, what, cur, refs[:n_refs], block, R, lam, subpel)
                    out = m.predict_picture_refs(p_cur, p_refs[:n_refs], dst, block=block, search_range=R, lam=lam, subpel=subpel)
                    assert _same(out["mv"], mv), (what, np.argwhere(out["mv"] != mv)[:4])
                    assert _same(out["ref"], ref), (what, np.argwhere(out["ref"] != ref)[:4])
                    assert _same(out["cost"], cost), (what, np.argwhere(out["cost"] != cost)[:4])
                    got = dst.download()
                    assert _same(got, plane), (what, np.argwhere(got != plane)[:4])
                    # the internal contracts
                    m.compensate_refs(p_refs[:n_refs], out["mv"], out["ref"], dst2, block=block)
                    assert _same(dst2.download(), got), what
                    if n_refs == 1:
                        m.compensate(p_refs[0], out["mv"], dst2, block=block)
                        assert _same(dst2.download(), got), what
                        if subpel == 0:
                            field = m.predict_picture(p_cur, p_refs[0], dst2, block=block, search_range=R, lam=lam)
                            assert _same(field["mv"], out["mv"]) and _same(dst2.download(), got), what
                    fractional |= bool((out["mv"] & 3).any())
                    chosen |= set(np.unique(out["ref"]).tolist())
        if kind == "constant":
            assert not fractional and chosen == {0}
        if kind == "planted":
            assert fractional and len(chosen) >= 2, (fractional, chosen)
        if kind == "borders" and block < 64:   # (80 x 72 has four blocks of 64)
            assert len(chosen) >= 2, chosen
    finally:
        _close(p_cur, *p_refs, dst, dst2)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_block_residual_never_grows_with_the_window_or_the_references(gpu, ctx, case):
    """No restatement: at lam = 0 the winner minimises the block's sum |cur - dst|, and the candidate sets are nested (subpel 0 < 1 < 2, reference lists that are
    prefixes of one another), so the per-block residual of the downloaded planes is non-increasing along both."""
    pkg, m = gpu, ctx
    w, h, block, R = case
    cur, refs = _contents(pkg, w, h, block, R, "planted", 600 + block)
    p_cur, *p_refs = _pictures(m, cur, *refs)
    dst = m.picture(w, h).upload(np.zeros((h, w), np.int16))

    def residual(n_refs, subpel):
        m.predict_picture_refs(p_cur, p_refs[:n_refs], dst, block=block, search_range=R, lam=0, subpel=subpel, want_field=False)
        d = np.abs(cur.astype(np.int64) - dst.download().astype(np.int64))
        return np.add.reduceat(np.add.reduceat(d, np.arange(0, h, block), axis=0), np.arange(0, w, block), axis=1)

    try:
        res = {(n, s): residual(n, s) for n in (1, 2, 4) for s in (0, 1, 2)}
        for n in (1, 2, 4):
            assert (res[(n, 1)] <= res[(n, 0)]).all() and (res[(n, 2)] <= res[(n, 1)]).all(), n
        for s in (0, 1, 2):
            assert (res[(2, s)] <= res[(1, s)]).all() and (res[(4, s)] <= res[(2, s)]).all(), s
        assert res[(4, 2)].sum() < res[(1, 0)].sum()
    finally:
        _close(p_cur, *p_refs, dst)


def test_wrapped_references_of_different_pitches(gpu, ctx):
    pkg, m = gpu, ctx
    block, R = 16, 4
    cur, refs = _contents(pkg, W, H, block, R, "planted", 700)
    # odd pitches, bases one element behind a 16-byte boundary (2-byte aligned only), every reference its own pitch
    p_cur = _wrap(m, cur, 1, W + 2)
    p_refs = [_wrap(m, refs[0], 1, W + 2), _wrap(m, refs[1], 1, W + 4), m.picture(W, H).upload(refs[2]), _wrap(m, refs[3], 9, W + 7)]
    dst = m.picture(W, H).upload(np.full((H, W), -1, np.int16))
    try:
        for subpel, lam in ((2, 0), (1, 4)):
            plane, mv, ref, cost = pkg.motion.predict_refs(cur, refs, block, R, lam, subpel)
            out = m.predict_picture_refs(p_cur, p_refs, dst, block=block, search_range=R, lam=lam, subpel=subpel)
            assert _same(out["mv"], mv) and _same(out["ref"], ref) and _same(out["cost"], cost) and _same(dst.download(), plane), (subpel, lam)
            m.compensate_refs(p_refs, mv, ref, dst, block=block)
            assert _same(dst.download(), plane)
    finally:
        _close(p_cur, *p_refs, dst)


# ---- compensation with a table ----
def _special_vectors():
    """All 16 fractions on small whole-sample parts, vectors far outside each of the four borders (with fractions), the int16 extremes (the list of
    tests/test_motion_gpu.py)."""
    v = [(4 * ((f * 5) % 7 - 3) + (f & 3), 4 * ((f * 3) % 5 - 2) + (f >> 2)) for f in range(16)]
    v += [(-4 * 200 + 1, 6), (4 * 200 + 3, -5), (7, -4 * 150 + 2), (-2, 4 * 150 + 1), (-4 * 300, -4 * 300), (4 * 300 + 2, 4 * 300 + 2)]
    v += [(-32768, 32767), (32767, -32768), (-32768, -32768), (32767, 32767)]
    return v


@pytest.mark.parametrize("block", [8, 16, 64])
def test_compensate_refs_equals_the_restatement(gpu, ctx, block):
    pkg, m = gpu, ctx
    w, h = (80, 72) if block == 64 else (W, H)
    refs = [_noise((h, w), 800 + block + r) for r in range(4)]
    bx, by = pkg.capi.motion_blocks(w, h, block)
    n = bx * by
    special = _special_vectors()
    rng = np.random.default_rng(block)
    p_refs = [_wrap(m, refs[0], 1, w + 2)] + _pictures(m, *refs[1:])
    dst = m.picture(w, h).upload(np.full((h, w), -1, np.int16))
    try:
        seen, used = set(), set()
        for k in range(0, len(special), n):
            mv = rng.integers(-40, 41, size=(n, 2)).astype(np.int16)
            part = special[k:k + n]
            mv[rng.permutation(n)[:len(part)]] = np.array(part, np.int16)
            mv = mv.reshape(by, bx, 2)
            idx = ((np.arange(n) + k) % 4).astype(np.uint8).reshape(by, bx)   # every index used, neighbours differ
            m.compensate_refs(p_refs, mv, idx, dst, block=block)
            got, want = dst.download(), pkg.motion.compensate_refs(refs, mv, idx, block)
            assert _same(got, want), (block, np.argwhere(got != want)[:4])
            seen |= {tuple(v) for v in mv.reshape(-1, 2).tolist()}
            used |= set(idx.reshape(-1).tolist())
        assert seen >= set(special) and used == {0, 1, 2, 3}
        m.compensate_refs(p_refs, mv, None, dst, block=block)                 # NULL table: reference 0 everywhere
        assert _same(dst.download(), pkg.motion.compensate(refs[0], mv, block))
    finally:
        _close(*p_refs, dst)


def test_stream_order_predict_refs_then_predict_at(gpu, ctx):
    pkg, m = gpu, ctx
    org = np.ascontiguousarray(pkg.synth.natural_patches(128, 1, 5)[0][0][:H, :W]).astype(np.int16)
    refs = [_shifted(org, 2, -1).copy(), _shifted(org, -1, 1).copy()]
    refs[0][::4, ::4] += 3
    xy = np.array([(0, 0), (16, 0), (61, 0), (5, 7), (33, 29), (61, 29), (0, 29)], np.int32)
    poc, qp = np.arange(7, dtype=np.int32), np.full(7, 32, np.int32)
    p_org, *p_refs = _pictures(m, org, *refs)
    dst = m.picture(W, H).upload(np.zeros((H, W), np.int16))
    try:
        assert m.predict_picture_refs(p_org, p_refs, dst, block=16, search_range=4, lam=2, subpel=2, want_field=False) == {}
        got = m.predict_at(16, p_org, dst, xy, poc, qp)    # no synchronisation in between: the stream orders the two calls
        m.predict_picture_refs(p_org, p_refs, dst, block=16, search_range=4, lam=2, subpel=2)   # synchronous
        plane = dst.download()
        exp = m.predict_at(16, p_org, dst, xy, poc, qp)
        for k in exp:
            assert _same(got[k], exp[k]), k
        assert _same(plane, pkg.motion.predict_refs(org, refs, 16, 4, 2, 2)[0])
    finally:
        _close(p_org, *p_refs, dst)


def test_two_device_context_gives_equal_planes(gpu, ctx):
    pkg, m1 = gpu, ctx
    cur, refs = _contents(pkg, W, H, 16, 4, "planted", 900)
    refs = refs[:3]
    xy = np.array([(0, 0), (16, 0), (61, 0), (5, 7), (33, 29), (61, 29), (0, 29)], np.int32)   # 7 CUs of 16: both shards get some
    poc, qp = np.arange(7, dtype=np.int32), np.full(7, 32, np.int32)

    def run(m):
        p_cur, *p_refs = _pictures(m, cur, *refs)
        dst, dst2 = _pictures(m, np.zeros((H, W), np.int16), np.zeros((H, W), np.int16))
        try:
            field = m.predict_picture_refs(p_cur, p_refs, dst, block=16, search_range=4, lam=1, subpel=2)
            at = m.predict_at(16, p_cur, dst, xy, poc, qp)     # shards over the devices: every device's plane of dst is read
            m.compensate_refs(p_refs, field["mv"], field["ref"], dst2, block=16)
            return field, at, dst.download(), m.predict_at(16, p_cur, dst2, xy, poc, qp)
        finally:
            _close(p_cur, *p_refs, dst, dst2)

    one = run(m1)
    m2 = pkg.MltCnn(sizes=(16,), blobs={16: _blobs(pkg)[16]}, head_index={16: 0}, devices=[0, 0])
    try:
        assert m2.num_devices() == 2
        two = run(m2)
    finally:
        m2.close()
    plane, mv, ref, cost = pkg.motion.predict_refs(cur, refs, 16, 4, 1, 2)
    for f, at, d, at2 in (one, two):
        assert _same(f["mv"], mv) and _same(f["ref"], ref) and _same(f["cost"], cost) and _same(d, plane)
        for k in at:
            assert _same(at[k], one[1][k]) and _same(at2[k], one[1][k]), k


def test_errors_leave_everything_untouched(gpu, ctx):
    pkg, m = gpu, ctx
    lib = m._lib
    ref = _noise((H, W), 61)
    cur = _shifted(ref, 1, 1)
    marker = np.full((H, W), 7, np.int16)
    p_cur, p_ref, p_ref2, dst = _pictures(m, cur, ref, ref, marker)
    small = m.picture(W - 1, H).upload(np.zeros((H, W - 1), np.int16))
    wrapped = _wrap(m, marker, 0, W + 3)
    other = pkg.MltCnn(device=0, sizes=(16,))
    foreign = other.picture(W, H).upload(ref)
    mv = np.full((3, 5, 2), 5, np.int16)
    idx = np.full((3, 5), 1, np.uint8)
    cost = np.full((3, 5), 9, np.uint32)

    def cfg(block=16, rng=4, lam=0, subpel=2, flags=0, size=None):
        c = pkg.capi.motion_refs_config(block, rng, lam, subpel, flags)
        if size is not None:
            c.struct_size = size
        return c

    def handles(pics):
        return (C.c_void_p * 8)(*[p._h if p is not None else None for p in pics])

    two = (p_ref, p_ref2)

    def predict(c, a=p_cur, refs=two, n=None, d=dst):
        return lib.mlt_picture_predict_refs(m._h, a._h if a else None, handles(refs), len(refs) if n is None else n, C.byref(c), d._h if d else None,
                                            mv.ctypes.data, idx.ctypes.data, cost.ctypes.data)

    def compensate(c, refs=two, n=None, d=dst, field=mv, table=idx):
        return lib.mlt_picture_compensate_refs(m._h, handles(refs), len(refs) if n is None else n, C.byref(c), field.ctypes.data if field is not None else None,
                                               table.ctypes.data if table is not None else None, d._h if d else None)

    bad_table = idx.copy()
    bad_table[2, 3] = 2
    try:
        m.profile_enable(True)
        bad = {
            "wrapped dst": lambda: (predict(cfg(), d=wrapped), compensate(cfg(), d=wrapped)),
            "dst is a reference": lambda: (predict(cfg(), d=p_ref), predict(cfg(), d=p_ref2), compensate(cfg(), d=p_ref), compensate(cfg(), d=p_ref2)),
            "dst is cur": lambda: (predict(cfg(), d=p_cur),),
            "unequal geometry": lambda: (predict(cfg(), refs=(p_ref, small)), predict(cfg(), a=small), compensate(cfg(), refs=(p_ref, small)), compensate(cfg(), d=small)),
            "block 24": lambda: (predict(cfg(block=24)), compensate(cfg(block=24))),
            "range 65": lambda: (predict(cfg(rng=65)), predict(cfg(rng=-1))),
            "lambda 65536": lambda: (predict(cfg(lam=65536)), predict(cfg(lam=-1))),
            "subpel 3": lambda: (predict(cfg(subpel=3)), predict(cfg(subpel=-1))),
            "flags 1": lambda: (predict(cfg(flags=1)), compensate(cfg(flags=1))),
            "struct_size": lambda: (predict(cfg(size=20)), predict(cfg(size=28)), compensate(cfg(size=0)), compensate(cfg(size=20))),
            "n_refs": lambda: (predict(cfg(), n=0), predict(cfg(), refs=(p_ref,) * 5), predict(cfg(), n=-1), compensate(cfg(), n=0), compensate(cfg(), refs=(p_ref,) * 5)),
            "another context's picture": lambda: (predict(cfg(), refs=(p_ref, foreign)), predict(cfg(), a=foreign), compensate(cfg(), refs=(p_ref, foreign))),
            "NULL field": lambda: (compensate(cfg(), field=None),),
            "NULL config": lambda: (lib.mlt_picture_predict_refs(m._h, p_cur._h, handles(two), 2, None, dst._h, mv.ctypes.data, idx.ctypes.data, cost.ctypes.data),
                                    lib.mlt_picture_compensate_refs(m._h, handles(two), 2, None, mv.ctypes.data, idx.ctypes.data, dst._h)),
            "NULL picture": lambda: (predict(cfg(), a=None), predict(cfg(), d=None), predict(cfg(), refs=(p_ref, None)), compensate(cfg(), refs=(None, p_ref)),
                                     lib.mlt_picture_predict_refs(m._h, p_cur._h, None, 2, C.byref(cfg()), dst._h, mv.ctypes.data, idx.ctypes.data, cost.ctypes.data)),
            "table entry >= n_refs": lambda: (compensate(cfg(), table=bad_table), compensate(cfg(), refs=(p_ref,))),
        }
        for what, call in bad.items():
            codes = call()
            assert all(rc == MLT_ERR_ARG for rc in codes), (what, codes)
            assert lib.mlt_last_error(m._h), what
            assert (mv == 5).all() and (idx == 1).all() and (cost == 9).all(), what
            assert _same(dst.download(), marker), what
        assert compensate(cfg(), table=bad_table) == MLT_ERR_ARG and b"(3, 2)" in lib.mlt_last_error(m._h)   # the block, as (column, row)
        assert _same(wrapped.download(), marker) and _same(p_ref.download(), ref) and _same(p_cur.download(), cur)
        assert m.profile_read() == [], "a refused call launched something"
        m.profile_enable(False)
        # range, lambda and subpel are not read by the compensation; block 0 is 16; the same picture may be listed more than once
        c = cfg(block=0, rng=999, lam=-5, subpel=77)
        assert compensate(c, refs=(p_ref, p_ref), field=np.zeros((3, 5, 2), np.int16)) == 0 and _same(dst.download(), np.clip(ref, 0, 1023))
    finally:
        m.profile_enable(False)
        _close(p_cur, p_ref, p_ref2, dst, small, wrapped, foreign)
        other.close()


def test_profile_rows_carry_the_launch_counts(gpu, ctx):
    pkg, m1 = gpu, ctx
    ref = _noise((H, W), 71, 0, 1024)
    cur = _shifted(ref, 1, 0)
    m2 = pkg.MltCnn(sizes=(16,), devices=[0, 0])
    try:
        for m, ndev in ((m1, 1), (m2, 2)):
            lib = m._lib
            p_cur, p_a, p_b, p_c = _pictures(m, cur, ref, ref, ref)
            dst = m.picture(W, H).upload(np.zeros((H, W), np.int16))
            hs = [lib.mlt_device_ctx(m._h, g) for g in range(ndev)]
            assert all(hs)
            for h in hs:
                assert lib.mlt_profile_enable(h, 1) == 0
            m.predict_picture_refs(p_cur, [p_a, p_b, p_c], dst, block=16, search_range=2, subpel=2)          # 15 blocks, three references
            m.predict_picture_refs(p_cur, [p_a], dst, block=8, search_range=1, subpel=0, want_field=False)   # 60 blocks, one
            m.compensate_refs([p_a, p_b], np.zeros((3, 5, 2), np.int16), np.zeros((3, 5), np.uint8), dst, block=16)
            m.compensate_refs([p_a, p_b], np.zeros((3, 5, 2), np.int16), None, dst, block=16)
            for h in hs:
                rows = (pkg.capi.MltKernelTime * 16)()
                k = lib.mlt_profile_read(h, rows, 16)
                got = {rows[i].name.decode(): (rows[i].launches, rows[i].bytes) for i in range(k)}
                assert lib.mlt_profile_enable(h, 0) == 0
                assert set(got) == {"motion_search", "motion_refine", "picture_compensate"}, got
                assert got["motion_search"][0] == 3 + 1 and got["motion_refine"][0] == 2 and got["picture_compensate"][0] == 4, got
                # algorithmic bytes: both pictures read, a vector and a cost per block | cur and every reference read, an integer vector per reference and block, a
                # vector, a cost and an index per block | the reference read and the prediction written, a vector (and with a table an index) per block
                assert got["motion_search"][1] == 4 * (W * H * 4) + (3 * 15 + 60) * 8
                assert got["motion_refine"][1] == W * H * 2 * (4 + 2) + 15 * (4 * 3 + 9) + 60 * (4 + 9)
                assert got["picture_compensate"][1] == 4 * (W * H * 4) + (15 + 60 + 15) * 5 + 15 * 4
            _close(p_cur, p_a, p_b, p_c, dst)
    finally:
        m2.close()


def test_picture_map_motion_refine_builds_the_prediction_on_the_device(gpu, ctx):
    """tools/picture_map.py --motion ... --motion-refine: frame f of a sequence is predicted from frames f - 1, f - 2, ... (clipped at frame 0) by
    mlt_picture_predict_refs."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import picture_map as pm
    pkg, m = gpu, ctx
    base = _smooth((H + 8, W + 8), 81)
    seq = np.stack([base[4:4 + H, 4:4 + W], base[3:3 + H, 5:5 + W], base[5:5 + H, 2:2 + W], base[4:4 + H, 6:6 + W]])
    motion = (16, 3, 2, 2, 2)   # block, range, lambda, subpel, n_refs
    with pm.uploaded(m, seq, seq, motion) as pics:
        assert len(pics) == 4
        for f, (p_org, p_pred) in enumerate(pics):
            refs = [seq[max(f - 1, 0)], seq[max(f - 2, 0)]]
            assert _same(p_org.download(), seq[f])
            assert _same(p_pred.download(), pkg.motion.predict_refs(seq[f], refs, 16, 3, 2, 2)[0]), f
