"""GPU (MI355X): prediction pictures -- mlt_picture_compensate, mlt_picture_predict and mlt_picture_download against the numpy restatement
fastintercu-vvc_amd/motion.py (itself held to scalar loops by tests/test_motion_cpu.py).  The rule is integer arithmetic, so EVERY assertion is byte equality; no
tolerance appears anywhere in this file.

Shapes are the smallest at which the kernels can go wrong: 77 x 45 (odd width, nothing a multiple of 8: every block size has clipped border blocks, an odd block
width of 13 exercises the search's half pair, a row of 8-sample store items is cut by the right border) and 80 x 72 for (block, range) = (64, 64), the LDS maximum,
where only the top-left block is complete."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MLT_ERR_ARG = 1
W, H = 77, 45


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


def _shifted(ref, sx, sy):
    h, w = ref.shape
    ys, xs = np.mgrid[0:h, 0:w]
    return ref[np.clip(ys + sy, 0, h - 1), np.clip(xs + sx, 0, w - 1)]


def _wrap(m, arr2d, offset_elems, pitch):
    """arr2d as a wrapped picture: a torch int16 tensor of offset_elems + H * pitch elements of seeded noise, the plane starting at element offset_elems (the idea of
    tests/test_pictures_gpu.py's helper)."""
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


# ---- compensation ----
def _special_vectors():
    """All 16 fractions on small whole-sample parts, vectors far outside each of the four borders (with fractions), the int16 extremes."""
    v = [(4 * ((f * 5) % 7 - 3) + (f & 3), 4 * ((f * 3) % 5 - 2) + (f >> 2)) for f in range(16)]
    v += [(-4 * 200 + 1, 6), (4 * 200 + 3, -5), (7, -4 * 150 + 2), (-2, 4 * 150 + 1), (-4 * 300, -4 * 300), (4 * 300 + 2, 4 * 300 + 2)]
    v += [(-32768, 32767), (32767, -32768), (-32768, -32768), (32767, 32767)]
    return v


def _fields(bx, by, seed):
    """Fields over bx x by blocks that together hold every special vector; the other blocks take seeded vectors of a few samples."""
    special = _special_vectors()
    n = bx * by
    rng = np.random.default_rng(seed)
    fields = []
    for k in range(0, len(special), n):
        mv = rng.integers(-40, 41, size=(n, 2)).astype(np.int16)
        part = special[k:k + n]
        slots = rng.permutation(n)[:len(part)]
        mv[slots] = np.array(part, np.int16)
        fields.append(mv.reshape(by, bx, 2))
    assert {tuple(v) for f in fields for v in f.reshape(-1, 2)} >= set(special)
    return fields


@pytest.mark.parametrize("wrapped", [False, True], ids=["owned", "wrapped_odd_pitch"])
@pytest.mark.parametrize("block", [8, 16, 64])
def test_compensate_equals_the_restatement(gpu, ctx, block, wrapped):
    pkg, m = gpu, ctx
    ref = _noise((H, W), 100 + block)
    assert ref.min() < 0 and ref.max() > 1023
    bx, by = pkg.capi.motion_blocks(W, H, block)
    assert (bx, by) == (-(-W // block), -(-H // block))
    # wrapped: an odd pitch and a base one element behind a 16-byte boundary -- 2-byte aligned, not 16
    p_ref = _wrap(m, ref, 1, W + 2) if wrapped else m.picture(W, H).upload(ref)
    dst = m.picture(W, H).upload(np.full((H, W), -1, np.int16))
    try:
        fields = _fields(bx, by, 7 * block)
        seen = set()
        for mv in fields:
            m.compensate(p_ref, mv, dst, block=block)
            want = pkg.motion.compensate(ref, mv, block)
            got = dst.download()
            assert _same(got, want), (block, wrapped, np.argwhere(got != want)[:4])
            seen |= {(int(x) & 3, int(y) & 3) for x, y in mv.reshape(-1, 2)}
        assert len(seen) == 16
    finally:
        _close(p_ref, dst)


# ---- search + compensation ----
def _contents(w, h, block, R, seed):
    """-> {name: (cur, ref)}: a clamped integer shift of seeded noise with a few samples disturbed, a constant pair, a pair of horizontal period 4."""
    ref = _noise((h, w), seed)
    sx, sy = min(R, 3), -min(R, 2)
    cur = _shifted(ref, sx, sy).copy()
    cur[::5, ::3] += 1
    const = np.full((h, w), 517, np.int16)
    f = np.array([100, 400, 250, 900], np.int16)
    xs = np.arange(w)
    return {"shift": (cur, ref), "constant": (const, const.copy()), "period4": (np.tile(f[(xs + 2) % 4], (h, 1)), np.tile(f[xs % 4], (h, 1)))}


SEARCH_CASES = [(77, 45, 8, 0), (77, 45, 8, 1), (77, 45, 16, 7), (77, 45, 32, 16), (80, 72, 64, 64)]


@pytest.mark.parametrize("content", ["shift", "constant", "period4"])
@pytest.mark.parametrize("case", SEARCH_CASES, ids=lambda c: "%dx%d_b%d_r%d" % c)
def test_predict_picture_equals_the_restatement(gpu, ctx, case, content):
    pkg, m = gpu, ctx
    w, h, block, R = case
    cur, ref = _contents(w, h, block, R, 200 + block + R)[content]
    sad = pkg.motion.sad_volume(cur, ref, block, R)   # once for both lambdas
    p_cur, p_ref = _pictures(m, cur, ref)
    dst, dst2 = _pictures(m, np.full((h, w), -1, np.int16), np.full((h, w), -2, np.int16))
    try:
        for lam in (0, 3):
            want_mv, want_cost = pkg.motion.pick(sad, lam)
            out = m.predict_picture(p_cur, p_ref, dst, block=block, search_range=R, lam=lam)
            assert _same(out["mv"], want_mv), (case, content, lam, np.argwhere(out["mv"] != want_mv)[:4])
            assert _same(out["cost"], want_cost), (case, content, lam, np.argwhere(out["cost"] != want_cost)[:4])
            got = dst.download()
            assert _same(got, pkg.motion.compensate(ref, want_mv, block)), (case, content, lam)
            m.compensate(p_ref, out["mv"], dst2, block=block)
            assert _same(dst2.download(), got), (case, content, lam)
        if content == "constant":
            assert not want_mv.any() and not want_cost.any()
    finally:
        _close(p_cur, p_ref, dst, dst2)


def test_download_keeps_the_gaps_of_a_strided_buffer(gpu, ctx):
    m = ctx
    plane = _noise((H, W), 31)
    pic = m.picture(W, H).upload(plane)
    wrapped = _wrap(m, plane, 1, W + 2)
    try:
        for p in (pic, wrapped):
            host = np.full((H, W + 5), -7, np.int16)
            p.download(host[:, :W])
            assert _same(np.ascontiguousarray(host[:, :W]), plane) and (host[:, W:] == -7).all()
        assert _same(pic.download(), plane)
    finally:
        _close(pic, wrapped)


def test_tree_on_a_predicted_picture_is_the_tree_on_the_uploaded_restatement(gpu, ctx):
    pkg, m = gpu, ctx
    org = np.ascontiguousarray(pkg.synth.natural_patches(128, 1, 5)[0][0][:H, :W]).astype(np.int16)
    ref = _shifted(org, 2, -1).copy()
    ref[::4, ::4] += 3
    want = ("leaf_map", "logits", "decisions", "candidates")
    p_org, p_ref = _pictures(m, org, ref)
    dst = m.picture(W, H).upload(np.zeros((H, W), np.int16))
    try:
        assert m.predict_picture(p_org, p_ref, dst, block=16, search_range=4, lam=2, want_field=False) == {}
        got = m.predict_tree(p_org, dst, 3, 30, top=32, min_size=16, want=want)   # no synchronisation in between: the stream orders the two calls
        plane, _, _ = pkg.motion.predict(org, ref, 16, 4, 2)
        up = m.picture(W, H).upload(plane)
        exp = m.predict_tree(p_org, up, 3, 30, top=32, min_size=16, want=want)
        up.close()
        assert len(got["nodes"]) == len(exp["nodes"]) >= 2
        for k in ("nodes",) + want:
            assert _same(got[k], exp[k]), k
        assert _same(dst.download(), plane)
    finally:
        _close(p_org, p_ref, dst)


def test_picture_map_motion_builds_the_prediction_on_the_device(gpu, ctx):
    """tools/picture_map.py --motion: the maps from two originals equal the maps from (original, the restatement's prediction); frame f of a sequence takes
    frame f - 1 as its reference and frame 0 itself."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import picture_map as pm
    pkg, m = gpu, ctx
    ref = _noise((H, W), 81, 0, 1024)
    org = _shifted(ref, 1, 2).copy()
    org[::4, ::7] += 5
    motion = (16, 3, 2)
    got = pm.run_maps(m, org, ref, (32, 16), 2, 30, motion=motion)
    plane, _, _ = pkg.motion.predict(org, ref, *motion)
    want = pm.run_maps(m, org, plane, (32, 16), 2, 30)
    assert set(got) == set(want) == {32, 16}
    for s in got:
        for k in ("xy", "split", "confidence", "mask"):
            assert _same(got[s][k], want[s][k]), (s, k)
    seq = np.stack([ref, org, _shifted(org, -1, 0)])
    with pm.uploaded(m, seq, seq, motion) as pics:
        assert len(pics) == 3
        for f, (p_org, p_pred) in enumerate(pics):
            assert _same(p_org.download(), seq[f])
            assert _same(p_pred.download(), pkg.motion.predict(seq[f], seq[max(f - 1, 0)], *motion)[0]), f


def test_two_device_context_predicts_the_single_device_bytes(gpu, ctx):
    pkg, m1 = gpu, ctx
    ref = _noise((H, W), 51, 0, 1024)
    org = _shifted(ref, -2, 1).copy()
    org[::3, ::5] += 2
    xy = np.array([(0, 0), (16, 0), (61, 0), (5, 7), (33, 29), (61, 29), (0, 29)], np.int32)   # 7 CUs of 16: both shards get some
    poc, qp = np.arange(7, dtype=np.int32), np.full(7, 32, np.int32)

    def run(m):
        p_org, p_ref = _pictures(m, org, ref)
        dst = m.picture(W, H).upload(np.zeros((H, W), np.int16))
        try:
            field = m.predict_picture(p_org, p_ref, dst, block=16, search_range=5, lam=1)
            return field, m.predict_at(16, p_org, dst, xy, poc, qp), dst.download()
        finally:
            _close(p_org, p_ref, dst)

    one = run(m1)
    m2 = pkg.MltCnn(sizes=(16,), blobs={16: _blobs(pkg)[16]}, head_index={16: 0}, devices=[0, 0])
    try:
        assert m2.num_devices() == 2
        two = run(m2)
    finally:
        m2.close()
    plane, mv, cost = pkg.motion.predict(org, ref, 16, 5, 1)
    for f, p, d in (one, two):
        assert _same(f["mv"], mv) and _same(f["cost"], cost) and _same(d, plane)
    for k in one[1]:
        assert _same(one[1][k], two[1][k]), k


def test_errors_leave_everything_untouched(gpu, ctx):
    pkg, m = gpu, ctx
    lib = m._lib
    ref = _noise((H, W), 61)
    cur = _shifted(ref, 1, 1)
    marker = np.full((H, W), 7, np.int16)
    p_cur, p_ref, dst = _pictures(m, cur, ref, marker)
    small = m.picture(W - 1, H).upload(np.zeros((H, W - 1), np.int16))
    wrapped = _wrap(m, marker, 0, W + 3)
    other = pkg.MltCnn(device=0, sizes=(16,))
    foreign = other.picture(W, H).upload(ref)
    mv = np.full((3, 5, 2), 5, np.int16)
    cost = np.full((3, 5), 9, np.uint32)

    def cfg(block=16, rng=4, lam=0, flags=0, size=None):
        c = pkg.capi.motion_config(block, rng, lam, flags)
        if size is not None:
            c.struct_size = size
        return c

    def predict(c, a=p_cur, b=p_ref, d=dst):
        return lib.mlt_picture_predict(m._h, a._h, b._h, C.byref(c), d._h, mv.ctypes.data, cost.ctypes.data)

    def compensate(c, b=p_ref, d=dst, field=mv):
        return lib.mlt_picture_compensate(m._h, b._h, C.byref(c), field.ctypes.data if field is not None else None, d._h)

    try:
        m.profile_enable(True)
        bad = {
            "wrapped dst": lambda: (predict(cfg(), d=wrapped), compensate(cfg(), d=wrapped)),
            "dst is ref": lambda: (predict(cfg(), d=p_ref), compensate(cfg(), d=p_ref)),
            "dst is cur": lambda: (predict(cfg(), d=p_cur),),
            "unequal geometry": lambda: (predict(cfg(), b=small), predict(cfg(), a=small), compensate(cfg(), b=small), compensate(cfg(), d=small)),
            "block 24": lambda: (predict(cfg(block=24)), compensate(cfg(block=24))),
            "range 65": lambda: (predict(cfg(rng=65)), predict(cfg(rng=-1))),
            "lambda 65536": lambda: (predict(cfg(lam=65536)), predict(cfg(lam=-1))),
            "flags 1": lambda: (predict(cfg(flags=1)), compensate(cfg(flags=1))),
            "struct_size": lambda: (predict(cfg(size=16)), predict(cfg(size=24)), compensate(cfg(size=0))),
            "another context's picture": lambda: (predict(cfg(), b=foreign), predict(cfg(), a=foreign), compensate(cfg(), b=foreign)),
            "NULL field": lambda: (compensate(cfg(), field=None),),
            "NULL config": lambda: (lib.mlt_picture_predict(m._h, p_cur._h, p_ref._h, None, dst._h, mv.ctypes.data, cost.ctypes.data),
                                    lib.mlt_picture_compensate(m._h, p_ref._h, None, mv.ctypes.data, dst._h)),
            "NULL picture": lambda: (lib.mlt_picture_predict(m._h, None, p_ref._h, C.byref(cfg()), dst._h, mv.ctypes.data, cost.ctypes.data),
                                     lib.mlt_picture_predict(m._h, p_cur._h, p_ref._h, C.byref(cfg()), None, mv.ctypes.data, cost.ctypes.data),
                                     lib.mlt_picture_compensate(m._h, None, C.byref(cfg()), mv.ctypes.data, dst._h)),
        }
        for what, call in bad.items():
            codes = call()
            assert all(rc == MLT_ERR_ARG for rc in codes), (what, codes)
            assert lib.mlt_last_error(m._h), what
            assert (mv == 5).all() and (cost == 9).all(), what
            assert _same(dst.download(), marker), what
        assert _same(wrapped.download(), marker) and _same(p_ref.download(), ref) and _same(p_cur.download(), cur)
        assert m.profile_read() == [], "a refused call launched something"
        m.profile_enable(False)
        # range and lambda are not read by the compensation; block 0 is 16
        c = cfg(block=0, rng=999, lam=-5)
        field = np.zeros((3, 5, 2), np.int16)
        assert compensate(c, field=field) == 0 and _same(dst.download(), np.clip(ref, 0, 1023))
    finally:
        m.profile_enable(False)
        _close(p_cur, p_ref, dst, small, wrapped, foreign)
        other.close()


def test_profile_rows_one_launch_of_each_kernel_per_device(gpu, ctx):
    pkg, m1 = gpu, ctx
    ref = _noise((H, W), 71, 0, 1024)
    cur = _shifted(ref, 1, 0)
    m2 = pkg.MltCnn(sizes=(16,), devices=[0, 0])
    try:
        for m, ndev in ((m1, 1), (m2, 2)):
            lib = m._lib
            p_cur, p_ref = _pictures(m, cur, ref)
            dst = m.picture(W, H).upload(np.zeros((H, W), np.int16))
            handles = [lib.mlt_device_ctx(m._h, g) for g in range(ndev)]
            assert all(handles)
            for h in handles:
                assert lib.mlt_profile_enable(h, 1) == 0
            m.predict_picture(p_cur, p_ref, dst, block=16, search_range=2)
            m.predict_picture(p_cur, p_ref, dst, block=8, search_range=1, want_field=False)
            m.compensate(p_ref, np.zeros((3, 5, 2), np.int16), dst, block=16)
            for h in handles:
                rows = (pkg.capi.MltKernelTime * 16)()
                k = lib.mlt_profile_read(h, rows, 16)
                got = {rows[i].name.decode(): (rows[i].launches, rows[i].bytes) for i in range(k)}
                assert lib.mlt_profile_enable(h, 0) == 0
                assert set(got) == {"motion_search", "picture_compensate"}, got
                assert got["motion_search"][0] == 2 and got["picture_compensate"][0] == 3, got
                # algorithmic bytes: both pictures read | the reference read and the prediction written, + the field
                assert got["motion_search"][1] == 2 * (W * H * 4) + (15 + 60) * 8
                assert got["picture_compensate"][1] == 3 * (W * H * 4) + (15 + 60 + 15) * 4
            _close(p_cur, p_ref, dst)
    finally:
        m2.close()
