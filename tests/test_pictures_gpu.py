"""GPU (MI355X): device-resident pictures -- mlt_predict_at against the dense entry points it is built on.  Shipped configuration (flags = 0) throughout.

picture_gather_kernel only produces the dense planes the batch path consumes, so every assertion between the two paths is BYTE equality; the bounds against the
reference are the project's own (none of them taken from what the device returns):
  LOGIT_TOL = 1e-3   the logit contract (tests/test_hip_parity.py)
  UNDECIDED_CAP      CUs whose REFERENCE top-2 margin is at or below twice the exact arithmetic's noise (4e-5): helpers.check_splits counts them from the fixture
                     logits alone, whatever the device returns.  DESIGN.md (c) states 5 in the near-tie fixtures + the 2 CUs of the exact-tie fixture; that is the 128
                     model's figure (near_tie 2 + near_tie_w13 3 + argmax_tie 2 = 7, the cap asserted for it).  The 2-class decision head of the CU models puts more
                     of its near-tie CUs inside +-4e-5: counted from tests/golden/golden_{64,32,16}.json on the CPU, the same three cases hold 4 + 7 + 2 = 13,
                     3 + 3 + 2 = 8 and 2 + 6 + 2 = 10 such CUs.  No device can bring those counts under 7 -- they are properties of the fixtures -- so each size's
                     cap is its own fixture count; every other CU's split must equal the reference's.

The mosaic is the smallest layout on which the gather can go wrong: n CUs of size S pasted into a picture of width W = 3 S + 13 in rows of three, row r at
y = r (S + 5), x offsets (0, S + 1, 2 S + 13) in even and (4, S + 7, 2 S + 13) in odd rows -- x mod 8 takes 0, 1, 4, 5 and 7, the third column is flush with the right
edge, the last row with the bottom edge, odd rows have odd y -- and seeded noise everywhere between the CUs."""
import ctypes as C

import numpy as np
import pytest

from helpers import SIZES, check_splits, head_slices, load_golden, materialise

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3
UNDECIDED_CAP = {128: 5 + 2, 64: 13, 32: 8, 16: 10}
FIXTURE_CASES = ("texture", "flat", "partial_flat", "dither", "out_of_range_pels", "argmax_tie", "near_tie", "near_tie_w13")
MLT_ERR_ARG, MLT_ERR_SIZE_DISABLED = 1, 4
ALL = ("split", "logits", "decisions", "candidates")


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


def _ctx(pkg, size, blob, head=None, **kw):
    return pkg.MltCnn(device=0, sizes=(size,), blobs={size: blob}, head_index=None if head is None else {size: head}, **kw)


def _blob(pkg, size, seed=10):
    return pkg.weights.synthetic_blob(pkg.synth.ARCH_CTU if size == 128 else pkg.synth.ARCH_CU, seed)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def mosaic_positions(n, S):
    xs = ((0, S + 1, 2 * S + 13), (4, S + 7, 2 * S + 13))
    return np.array([(xs[(i // 3) & 1][i % 3], (i // 3) * (S + 5)) for i in range(n)], np.int32)


def mosaic(cus, S, seed, stride_extra=0, extra_rows=0):
    """-> (padded [H + extra_rows, W + stride_extra] int16 array of seeded noise with the CUs pasted in, W, H, xy)."""
    n = len(cus)
    R = (n + 2) // 3
    W, H = 3 * S + 13, R * S + 5 * (R - 1)
    xy = mosaic_positions(n, S)
    pic = np.random.default_rng(seed).integers(0, 1024, size=(H + extra_rows, W + stride_extra)).astype(np.int16)
    for (x, y), cu in zip(xy, cus):
        pic[y:y + S, x:x + S] = cu
    assert (n < 3 or xy[:, 0].max() + S == W) and xy[:, 1].max() + S == H and {int(v) % 8 for v in xy[:, 0]} <= {0, 1, 4, 5, 7}
    return pic, W, H, xy


def cut(pic, xy, S):
    return np.stack([pic[y:y + S, x:x + S] for x, y in xy]) if len(xy) else np.zeros((0, S, S), np.int16)


def _wrap(m, arr2d, W, H, offset_elems, pitch):
    """The H x W top-left part of arr2d as a torch int16 tensor of offset_elems + H * pitch elements, plane starting at element offset_elems -> wrapped picture."""
    import torch
    host = np.random.default_rng(99).integers(0, 1024, size=offset_elems + H * pitch).astype(np.int16)
    view = host[offset_elems:offset_elems + H * pitch].reshape(H, pitch)
    view[:, :W] = arr2d[:H, :W]
    t = torch.from_numpy(host).to(torch.device("cuda", 0))
    return m.wrap_picture(t.data_ptr() + 2 * offset_elems, pitch, W, H, keep=t)


def _aligned_odd_pitch(W, H):
    """The smallest odd pitch >= W + 2 for which an extent of (H - 1) pitch + W elements ends on a 16-byte boundary (H even)."""
    assert H % 2 == 0
    p = W + 2 if (W + 2) % 2 else W + 3
    while ((H - 1) * p + W) % 8:
        p += 2
    return p


def _check_against(out, split, logits, dec, cand, what):
    assert _same(out["split"], split), what
    assert _same(out["logits"], logits), what
    assert _same(out["decisions"], dec), what
    assert _same(out["candidates"], cand), what


@pytest.mark.parametrize("size", SIZES)
def test_predict_at_is_the_dense_path_on_the_fixtures(gpu, size):
    pkg = gpu
    golden = load_golden(size)
    cases = {c["name"]: c for c in golden["cases"]}
    dec_head = 2 if size == 128 else 0
    sl = head_slices([2, 3, 4] if size == 128 else [2, 3, 4, 6])[dec_head]
    undecided, worst, reruns_total = 0, 0.0, 0
    for name in FIXTURE_CASES:
        case = cases[name]
        blob, org, pred, poc, qp, exp, exp_arg = materialise(pkg, golden, case)
        what = f"{size}/{name}"
        m = _ctx(pkg, size, blob)
        m.set_candidate_policy(size, float(np.float32(0.9)), 0)
        split, _ = m.predict_batch(org, pred, poc, qp)
        r0 = m.arithmetic(size)["guard_reruns"]
        cand, dec, logits = m.predict_batch_candidates(org, pred, poc, qp)
        dense_reruns = m.arithmetic(size)["guard_reruns"] - r0
        # library-owned pictures, uploaded from host arrays with stride W + 3
        org_pic, W, H, xy = mosaic(org, size, 1000 + size, stride_extra=3)
        pred_pic, _, _, _ = mosaic(pred, size, 2000 + size, stride_extra=3)
        assert np.array_equal(cut(org_pic, xy, size), org) and np.array_equal(cut(pred_pic, xy, size), pred)
        p_org, p_pred = m.picture(W, H).upload(org_pic[:, :W]), m.picture(W, H).upload(pred_pic[:, :W])
        r0 = m.arithmetic(size)["guard_reruns"]
        out = m.predict_at(size, p_org, p_pred, xy, poc, qp, want=ALL)
        at_reruns = m.arithmetic(size)["guard_reruns"] - r0
        _check_against(out, split, logits, dec, cand, what)
        assert at_reruns == dense_reruns, (what, at_reruns, dense_reruns)
        reruns_total += at_reruns
        # the reference
        err = float(np.abs(out["logits"] - exp).max())
        worst = max(worst, err)
        assert err <= LOGIT_TOL, (what, err)
        undecided += check_splits(out["split"], exp, [r[dec_head] for r in exp_arg], sl, True, LOGIT_TOL, what)
        # the same mosaics wrapped: plane at element 1 of a device tensor, odd pitch W + 2 -- rows alternate between 2- and 4-byte alignment (element path)
        w_org, w_pred = _wrap(m, org_pic, W, H, 1, W + 2), _wrap(m, pred_pic, W, H, 1, W + 2)
        _check_against(m.predict_at(size, w_org, w_pred, xy, poc, qp, want=ALL), split, logits, dec, cand, what + " wrapped")
        # ... and wrapped with an extent that starts and ends 16-byte aligned under an odd pitch: the vector paths, with a byte offset that changes per row
        # (one row of noise below the mosaic where that takes an even height)
        He = H + (H & 1)
        e_org, _, _, _ = mosaic(org, size, 1000 + size, extra_rows=He - H)
        e_pred, _, _, _ = mosaic(pred, size, 2000 + size, extra_rows=He - H)
        pitch = _aligned_odd_pitch(W, He)
        a_org, a_pred = _wrap(m, e_org, W, He, 0, pitch), _wrap(m, e_pred, W, He, 0, pitch)
        _check_against(m.predict_at(size, a_org, a_pred, xy, poc, qp, want=ALL), split, logits, dec, cand, what + " wrapped, aligned extent")
        # mixed sources: org wrapped (element path), pred library-owned (vector paths)
        _check_against(m.predict_at(size, w_org, p_pred, xy, poc, qp, want=ALL), split, logits, dec, cand, what + " mixed")
        m.close()
    print(f"size {size}: max|dlogit| vs fixtures {worst:.2e}, {undecided} CUs the reference itself cannot decide (cap {UNDECIDED_CAP[size]}), {reruns_total} guard re-runs")
    assert undecided <= UNDECIDED_CAP[size], undecided
    if size == 128:
        assert reruns_total > 0, "flat / dither / near-tie content must reach the guards through the picture path too"


def _device_batch(pkg, m, size, org, pred, poc, qp):
    """mlt_predict_batch_device on the cut planes -> (split, logits)."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(poc)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (org, pred, poc, qp)]
    d_lg = torch.zeros((n, m.num_logits(size)), dtype=torch.float32, device=dev)
    d_split = torch.full((n,), -7, dtype=torch.int32, device=dev)
    m.predict_batch_device(n, size, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d_split.data_ptr(), d_lg.data_ptr())
    m.synchronize()
    return d_split.cpu().numpy(), d_lg.cpu().numpy()


@pytest.mark.parametrize("size", [16, 128])
def test_positions_across_a_chunk_boundary(gpu, size):
    """16: 4096 + 37 arbitrary positions (one more than a pass of 4096 CUs holds), entry 5 repeated at entry 4100, against mlt_predict_batch on the numpy cuts.
    128: 130 overlapping positions -- the streaming launch class starts at 128 CUs -- against mlt_predict_batch_device on the cut planes."""
    pkg = gpu
    W, H, n = (1048, 280, 4096 + 37) if size == 16 else (700, 400, 130)
    rng = np.random.default_rng(4242 + size)
    org_pic = rng.integers(0, 1024, size=(H, W)).astype(np.int16)
    pred_pic = np.clip(org_pic.astype(np.int32) + rng.integers(-24, 25, size=(H, W)), 0, 1023).astype(np.int16)
    xy = np.stack([rng.integers(0, W - size + 1, size=n), rng.integers(0, H - size + 1, size=n)], axis=1).astype(np.int32)
    if size == 16:
        xy[4100] = xy[5]
    poc, qp = pkg.synth.make_scalars(n, 77)
    if size == 16:
        poc[4100], qp[4100] = poc[5], qp[5]
    m = _ctx(pkg, size, _blob(pkg, size))
    p_org, p_pred = m.picture(W, H).upload(org_pic), m.picture(W, H).upload(pred_pic)
    out = m.predict_at(size, p_org, p_pred, xy, poc, qp, want=("split", "logits"))
    c_org, c_pred = cut(org_pic, xy, size), cut(pred_pic, xy, size)
    if size == 16:
        split, logits = m.predict_batch(c_org, c_pred, poc, qp)
        assert out["logits"][4100].tobytes() == out["logits"][5].tobytes() and out["split"][4100] == out["split"][5]
    else:
        split, logits = _device_batch(pkg, m, size, c_org, c_pred, poc, qp)
    assert _same(out["split"], split) and _same(out["logits"], logits)
    assert len(np.unique(out["logits"], axis=0)) > n // 2   # (not n copies of one CU)
    m.close()


def test_upload_again_replaces_the_content_in_stream_order(gpu):
    pkg = gpu
    size, W, H, n = 64, 333, 201, 24
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 1024, size=(2, H, W)).astype(np.int16) for _ in range(2)]
    xy = np.stack([rng.integers(0, W - size + 1, size=n), rng.integers(0, H - size + 1, size=n)], axis=1).astype(np.int32)
    poc, qp = pkg.synth.make_scalars(n, 5)
    m = _ctx(pkg, size, _blob(pkg, size))
    p_org, p_pred = m.picture(W, H), m.picture(W, H)
    results = []
    for f in frames:
        p_org.upload(f[0])
        p_pred.upload(f[1])
        results.append(m.predict_at(size, p_org, p_pred, xy, poc, qp, want=("split", "logits")))
    for f, r in zip(frames, results):
        split, logits = m.predict_batch(cut(f[0], xy, size), cut(f[1], xy, size), poc, qp)
        assert _same(r["split"], split) and _same(r["logits"], logits)
    assert not _same(results[0]["logits"], results[1]["logits"])
    m.close()


def test_two_device_contexts_on_gpu_0(gpu):
    pkg = gpu
    size, W, H, n = 128, 500, 300, 21
    rng = np.random.default_rng(6)
    org_pic = rng.integers(0, 1024, size=(H, W)).astype(np.int16)
    pred_pic = np.clip(org_pic.astype(np.int32) + rng.integers(-24, 25, size=(H, W)), 0, 1023).astype(np.int16)
    xy = np.stack([rng.integers(0, W - size + 1, size=n), rng.integers(0, H - size + 1, size=n)], axis=1).astype(np.int32)
    poc, qp = pkg.synth.make_scalars(n, 6)
    blob = _blob(pkg, size)
    m1 = _ctx(pkg, size, blob)
    one = m1.predict_at(size, m1.picture(W, H).upload(org_pic), m1.picture(W, H).upload(pred_pic), xy, poc, qp, want=ALL)
    m1.close()
    m2 = pkg.MltCnn(sizes=(size,), blobs={size: blob}, devices=[0, 0])
    assert m2.num_devices() == 2
    p_org, p_pred = m2.picture(W, H).upload(org_pic), m2.picture(W, H).upload(pred_pic)
    two = m2.predict_at(size, p_org, p_pred, xy, poc, qp, want=ALL)
    for k in ALL:
        assert _same(one[k], two[k]), k
    single = m2.predict_at(size, p_org, p_pred, xy[:1], poc[:1], qp[:1], want=ALL)   # one CU: no sharding
    for k in ALL:
        assert _same(one[k][:1], single[k]), k
    import torch
    t = torch.zeros((H * W,), dtype=torch.int16, device=torch.device("cuda", 0))
    with pytest.raises(pkg.MltError) as ei:
        m2.wrap_picture(t.data_ptr(), W, W, H)
    assert ei.value.code == MLT_ERR_ARG
    m2.close()


def test_bad_arguments_launch_nothing(gpu):
    pkg = gpu
    size, W, H, n = 64, 200, 100, 4
    rng = np.random.default_rng(8)
    org_pic, pred_pic = rng.integers(0, 1024, size=(2, H, W)).astype(np.int16)
    blob = _blob(pkg, size)
    m, other = _ctx(pkg, size, blob), _ctx(pkg, size, blob)
    p_org, p_pred = m.picture(W, H).upload(org_pic), m.picture(W, H).upload(pred_pic)
    smaller = m.picture(W, H - 1).upload(pred_pic[:H - 1])
    foreign = other.picture(W, H).upload(pred_pic)
    good = np.array([(0, 0), (W - size, H - size), (7, 3), (W - size, 0)], np.int32)
    poc, qp = pkg.synth.make_scalars(n, 8)
    nl = m.num_logits(size)

    def call(sz, a, b, xy, count=n, outputs=True):
        xy = np.ascontiguousarray(xy, np.int32)
        split = np.full(n, -7, np.int32)
        logits = np.full((n, nl), -7.0, np.float32)
        dec = np.zeros(n, pkg.capi.DECISION_DTYPE)
        cand = np.zeros(n, pkg.capi.CANDIDATES_DTYPE)
        dec["raw_mode"] = -7
        cand["count"] = -7
        ptrs = [x.ctypes.data if outputs else None for x in (split, logits, dec, cand)]
        rc = m._lib.mlt_predict_at(m._h, sz, a._h, b._h, count, xy.ctypes.data, poc.ctypes.data, qp.ctypes.data, *ptrs)
        untouched = (split == -7).all() and (logits == -7.0).all() and (dec["raw_mode"] == -7).all() and (cand["count"] == -7).all()
        return rc, untouched, split, logits

    bad_x, bad_y = good.copy(), good.copy()
    bad_x[2] = (W - size + 1, 0)    # x + S == W + 1
    bad_y[3] = (0, -1)
    assert call(size, p_org, p_pred, bad_x)[:2] == (MLT_ERR_ARG, True)
    assert b"position 2" in m._lib.mlt_last_error(m._h)
    assert call(size, p_org, p_pred, bad_y)[:2] == (MLT_ERR_ARG, True)
    assert b"position 3" in m._lib.mlt_last_error(m._h)
    assert call(size, p_org, smaller, good)[:2] == (MLT_ERR_ARG, True)            # pictures of different geometry
    assert call(size, p_org, foreign, good)[:2] == (MLT_ERR_ARG, True)            # a picture of another context
    assert call(128, p_org, p_pred, np.zeros((n, 2), np.int32))[:2] == (MLT_ERR_SIZE_DISABLED, True)   # a size not loaded
    assert call(size, p_org, p_pred, good, outputs=False)[0] == MLT_ERR_ARG      # all outputs NULL
    assert call(size, p_org, p_pred, good, count=0)[:2] == (0, True)             # n = 0
    for w, h in ((15, 64), (64, 16385)):
        hnd = C.c_void_p()
        assert m._lib.mlt_picture_create(m._h, w, h, C.byref(hnd)) == MLT_ERR_ARG and not hnd.value
    assert m._lib.mlt_picture_upload(m._h, foreign._h, pred_pic.ctypes.data, W) == MLT_ERR_ARG
    assert m._lib.mlt_picture_destroy(m._h, foreign._h) == MLT_ERR_ARG
    # a following valid call still returns the right answer
    rc, untouched, split, logits = call(size, p_org, p_pred, good)
    ref_split, ref_logits = m.predict_batch(cut(org_pic, good, size), cut(pred_pic, good, size), poc, qp)
    assert rc == 0 and not untouched and _same(split, ref_split) and _same(logits, ref_logits)
    smaller.close()
    m.close()
    other.close()
