"""GPU: QP sweeps (include/mltcnn.h: mlt_predict_batch_device_sweep, mlt_predict_at_sweep) -- one network pass, the heads under up to 32 QPs per CU.

The contract is byte identity: slab q of a sweep is what the twin without a sweep returns with every qp[i] = qps[q] (tobytes() equality of split modes, logits,
decision and candidate records), although the guards -- which see the logits, and so the qp -- flag different CUs under different points.

  1  slab = twin on every size, through the device-pointer entry and through the picture entry at unaligned positions; texture mixed with CUs of the flat-guard
     families, so the exact re-run's union is non-empty through a QP-independent guard; 4 points, 1 point, 32 points with duplicates, 0 and negatives
  2  per-QP flags on a designed decision head whose top-2 margin is T |qp - poc| exactly: CU i is flagged at point q iff qps[q] == poc_i; the other heads' bytes
     show, per slab, who was re-run; guard_reruns grows by the union; the same under a gate and under a candidate policy against the twins
  3  one trunk pass: the profile of a 4-point sweep has heads_sweep x 1, no heads, and every other kernel as often as ONE twin call
  4  chunks (max_batch 64, n 150) and shards (ordinal 0 listed twice)
  5  errors leave the outputs untouched

Seed-13 weights; contexts as tests/test_designed_heads_gpu.py builds its own."""
import ctypes as C

import numpy as np
import pytest

import designed_heads as dh
import flat_guard_families as ff

pytestmark = pytest.mark.gpu
F = np.float32
SEED = 13
T, TOL = 2.0 ** -8, 2.0 ** -10
NAMES = ("split", "logits", "decisions", "candidates")
QPS_4 = [22, 27, 32, 37]
QPS_32 = list(range(-3, 25)) + [0, 22, 22, -3]     # 32 points: duplicates, 0, negatives, not sorted at the end


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


def _blob(pkg, size):
    return pkg.weights.synthetic_blob(dh.arch_of(size), SEED)


def _reruns(m, size):
    return m.arithmetic(size)["guard_reruns"]


def _mixed_content(pkg, size, n, seed=5):
    """n CUs: texture, every fourth one replaced by a CU of the flat-guard families (flagged and unflagged ones alternate there)."""
    org, pred = (a.copy() for a in pkg.synth.make_patches_bulk(size, n, seed))
    at = np.arange(0, n, 4)
    fam = ff.batch(pkg, size, 8, len(at))
    org[at], pred[at] = fam.org, fam.pred
    assert fam.flagged.any() and not fam.flagged.all()
    return org, pred, int(fam.flagged.sum())


class Device:
    """CU planes and poc in device memory; the sweep and its twin calls through the device-pointer entries -> {name: array} (sweep: leading [Q] axis)."""

    def __init__(self, pkg, m, size, org, pred, poc):
        import torch
        self.pkg, self.m, self.size, self.n = pkg, m, size, len(poc)
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.d = [torch.from_numpy(np.ascontiguousarray(x)).to(self.dev) for x in (org, pred, np.asarray(poc, np.int32))]

    def _outputs(self, rows):
        t = self.torch
        nl = self.m.num_logits(self.size)
        return {"split": t.full((rows,), -7, dtype=t.int32, device=self.dev), "logits": t.zeros((rows, nl), dtype=t.float32, device=self.dev),
                "decisions": t.zeros((rows * 48,), dtype=t.uint8, device=self.dev), "candidates": t.zeros((rows * 40,), dtype=t.uint8, device=self.dev)}

    def _host(self, o, shape):
        cap = self.pkg.capi
        return {"split": o["split"].cpu().numpy().reshape(shape), "logits": o["logits"].cpu().numpy().reshape(shape + (-1,)),
                "decisions": np.frombuffer(o["decisions"].cpu().numpy().tobytes(), cap.DECISION_DTYPE).reshape(shape).copy(),
                "candidates": np.frombuffer(o["candidates"].cpu().numpy().tobytes(), cap.CANDIDATES_DTYPE).reshape(shape).copy()}

    def sweep(self, qps, want=NAMES):
        o = self._outputs(len(qps) * self.n)
        p = lambda k: o[k].data_ptr() if k in want else None
        self.m.predict_batch_device_sweep(self.n, self.size, self.d[0].data_ptr(), self.d[1].data_ptr(), self.d[2].data_ptr(), qps,
                                          p("split"), p("logits"), p("decisions"), p("candidates"))
        self.m.synchronize()
        return {k: v for k, v in self._host(o, (len(qps), self.n)).items() if k in want}

    def twin(self, qp):
        """every qp[i] = qp: split + logits from mlt_predict_batch_device, records + logits from its candidates form (the logits of the two must agree)"""
        t = self.torch
        d_qp = t.full((self.n,), int(qp), dtype=t.int32, device=self.dev)
        o, o2 = self._outputs(self.n), self._outputs(self.n)
        a = [x.data_ptr() for x in self.d] + [d_qp.data_ptr()]
        self.m.predict_batch_device(self.n, self.size, *a, o["split"].data_ptr(), o["logits"].data_ptr())
        self.m.predict_batch_device(self.n, self.size, *a, None, o2["logits"].data_ptr(), d_decisions=o2["decisions"].data_ptr(), d_candidates=o2["candidates"].data_ptr())
        self.m.synchronize()
        h, h2 = self._host(o, (self.n,)), self._host(o2, (self.n,))
        assert h["logits"].tobytes() == h2["logits"].tobytes()
        h["decisions"], h["candidates"] = h2["decisions"], h2["candidates"]
        return h


def _compare(what, sweep, twin_of, qps):
    """every slab of every output against the twin's bytes (one twin call per distinct qp)"""
    twins = {}
    for q, qp in enumerate(qps):
        if qp not in twins:
            twins[qp] = twin_of(qp)
        for k in sweep:
            got, want = np.ascontiguousarray(sweep[k][q]), np.ascontiguousarray(twins[qp][k])
            if got.tobytes() != want.tobytes():
                rows = np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(got))])
                raise AssertionError(f"{what}: slab {q} (qp {qp}) differs from its twin in {k} at {len(rows)} CUs, first {rows[:8].tolist()}: "
                                     f"{got[rows[0]]} against {want[rows[0]]}")


def _picture_pair(m, size, org, pred, off=(1, 3)):
    """The CUs laid out on a grid inside one picture pair, the grid shifted by `off` (odd: no CU starts on an aligned sample) -> (org_pic, pred_pic, xy)."""
    n = len(org)
    cols = 20 if n >= 20 else n
    rows = -(-n // cols)
    W, H = cols * size + off[0] + 2, rows * size + off[1] + 2
    g = np.random.default_rng(3)
    po, pp = g.integers(0, 1024, (H, W)).astype(np.int16), g.integers(0, 1024, (H, W)).astype(np.int16)
    xy = np.zeros((n, 2), np.int32)
    for i in range(n):
        x, y = off[0] + (i % cols) * size, off[1] + (i // cols) * size
        po[y:y + size, x:x + size], pp[y:y + size, x:x + size] = org[i], pred[i]
        xy[i] = (x, y)
    return m.picture(W, H).upload(po), m.picture(W, H).upload(pp), xy


# ---- 1: slab = twin, every size ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (128, 64, 32, 16))
def test_every_slab_is_its_twin_byte_for_byte(gpu, size):
    pkg = gpu
    Fl = pkg.capi
    n = 300 if size == 128 else 70     # 300: above the 256-CU streaming threshold, a multiple of nothing
    m = pkg.MltCnn(device=0, sizes=(size,), blobs={size: _blob(pkg, size)}, flags=Fl.FLAG_NO_CALIBRATION | (0 if size == 128 else Fl.FLAG_FAST_SMALL))
    a = m.arithmetic(size)
    assert a["exact"] == 0 and a["flat_guard"] == 1 and a["decision_guard"] == 1, a
    org, pred, n_flat = _mixed_content(pkg, size, n)
    poc = np.random.default_rng(size).integers(0, 64, n).astype(np.int32)
    dev = Device(pkg, m, size, org, pred, poc)
    p_org, p_pred, xy = _picture_pair(m, size, org, pred)
    for qps in (QPS_4, [32], QPS_32):
        assert 1 <= len(qps) <= 32
        r0 = _reruns(m, size)
        sw = dev.sweep(qps)
        grew = _reruns(m, size) - r0
        assert n_flat <= grew <= n, (grew, n_flat)      # the union holds at least the CUs the (QP-independent) flat guard flags
        per_twin = []

        def twin(qp):
            before = _reruns(m, size)
            out = dev.twin(qp)
            per_twin.append((_reruns(m, size) - before) // 2)     # (two calls per twin)
            return out
        _compare(f"{size} device entry, {len(qps)} points", sw, twin, qps)
        assert max(per_twin) <= grew <= sum(per_twin), (grew, per_twin)
        print(f"{size}: Q = {len(qps)}: the sweep re-ran {grew} CUs (flat families {n_flat}); the twins {per_twin}")
        sp = m.predict_at_sweep(size, p_org, p_pred, xy, poc, qps)
        assert all(sp[k].shape[:2] == (len(qps), n) for k in NAMES)
        _compare(f"{size} picture entry, {len(qps)} points", sp, lambda qp: m.predict_at(size, p_org, p_pred, xy, poc, np.full(n, qp, np.int32)), qps)
        # (the gathered CUs are the dense ones: the two entries agree as well)
        assert all(sp[k].tobytes() == sw[k].tobytes() for k in NAMES)
    only_logits = dev.sweep(QPS_4, want=("logits",))
    assert only_logits["logits"].tobytes() == dev.sweep(QPS_4)["logits"].tobytes()
    p_org.close(); p_pred.close()
    m.close()


# ---- 2: per-QP flags on a designed decision head --------------------------------------------------------------------------------------------------------------
DESIGN = (np.array([0, -T, 0, 0], F), np.array([0, T, 0, 0], F), np.array([0, 0, dh.FAR, dh.FAR], F))     # logits (0, T (qp - poc), far, far): top-2 margin T |qp - poc|
QPS_D = [3, 5, 5, 9, 40]
N_D = 240


@pytest.fixture(scope="module")
def designed(gpu):
    pkg = gpu
    Fl = pkg.capi
    org, pred = pkg.synth.make_patches_bulk(128, N_D, 77)     # texture only
    poc = (np.arange(N_D) % 12).astype(np.int32)
    plain = _blob(pkg, 128)
    ex = pkg.MltCnn(device=0, sizes=(128,), blobs={128: plain}, flags=Fl.FLAG_EXACT_128)
    fa = pkg.MltCnn(device=0, sizes=(128,), blobs={128: plain}, flags=Fl.FLAG_NO_CALIBRATION | Fl.FLAG_NO_DECISION_GUARD | Fl.FLAG_NO_FLAT_GUARD)
    assert ex.arithmetic(128)["exact"] == 1 and fa.arithmetic(128)["exact"] == 0 and fa.arithmetic(128)["decision_guard"] == 0
    m = pkg.MltCnn(device=0, sizes=(128,), blobs={128: dh.designed_blob(0, SEED, 2, *DESIGN)}, head_index={128: 2},
                   flags=Fl.FLAG_NO_CALIBRATION | Fl.FLAG_NO_FLAT_GUARD, tolerance=TOL, guard_margin=T)
    a = m.arithmetic(128)
    assert a["guard_margin"] == T and a["decision_guard"] == 1 and a["flat_guard"] == 0 and a["exact"] == 0 and a["mag_guard_kind"] == 0, a
    refs = {}     # qp -> (exact logits, unguarded fast logits) of the plain blob: what the OTHER heads return when a CU was / was not re-run
    for qp in sorted(set(QPS_D)):
        full = np.full(N_D, qp, np.int32)
        refs[qp] = (ex.predict_batch(org, pred, poc, full)[1], fa.predict_batch(org, pred, poc, full)[1])
    yield pkg, m, org, pred, poc, refs
    for c in (ex, fa, m):
        c.close()


def test_flags_follow_the_point(designed):
    pkg, m, org, pred, poc, refs = designed
    m.set_confidence_gate(128, 0.0)
    m.set_candidate_policy(128, 0.0, 0)
    sl = slice(dh.head_offset(0, 2), dh.head_offset(0, 2) + 4)
    other = np.ones(9, bool)
    other[sl] = False
    dev = Device(pkg, m, 128, org, pred, poc)
    r0 = _reruns(m, 128)
    sw = dev.sweep(QPS_D)
    grew = _reruns(m, 128) - r0
    union = int(np.isin(poc, [3, 5, 9]).sum())
    assert union == 3 * (N_D // 12)
    assert grew == union, f"(a) guard_reruns grew by {grew}, the union of the flagged CUs has {union}"
    blind_total = 0
    for q, qp in enumerate(QPS_D):
        l = dh.designed_logits(*DESIGN, poc, np.full(N_D, qp, np.int32))
        srt = np.sort(l, axis=1)
        margin = srt[:, -1] - srt[:, -2]
        assert np.array_equal(margin, (F(T) * np.abs(qp - poc).astype(F)).astype(F)) and margin.dtype == F     # T |qp - poc|, exact in fp32
        want = poc == qp                                 # margin 0 < T: flagged; margin exactly T (|qp - poc| = 1) is not below T: not flagged
        assert np.array_equal(want, ~(margin >= F(T)))
        assert sw["logits"][q][:, sl].tobytes() == l.tobytes(), f"slab {q}: designed logits"
        le, lf = (np.ascontiguousarray(r[:, other]).view(np.uint32) for r in refs[qp])
        got = np.ascontiguousarray(sw["logits"][q][:, other]).view(np.uint32)
        blind = (le == lf).all(axis=1)
        blind_total += int(blind.sum())
        is_ex, is_fa = (got == le).all(axis=1), (got == lf).all(axis=1)
        bad = np.flatnonzero(~blind & ((is_ex != want) | (is_fa == want)))
        assert bad.size == 0, (f"(b) slab {q} (qp {qp}): {bad.size} CUs on the wrong side, first {bad[:8].tolist()} (poc {poc[bad[:8]].tolist()}): "
                               f"exact {is_ex[bad[:8]].tolist()}, fast {is_fa[bad[:8]].tolist()}")
        assert (is_ex | is_fa)[blind].all()
    share = blind_total / (len(QPS_D) * N_D)
    print(f"CUs whose exact and fast bytes coincide on the seeded heads: {blind_total} of {len(QPS_D) * N_D} (share {share:.4f}, cap 0.02)")
    assert share <= 0.02
    r0 = _reruns(m, 128)
    dev.twin(40)
    assert _reruns(m, 128) - r0 == 0, "(c) the flat and magnitude guards flag nothing on this content"
    _compare("designed head", sw, dev.twin, QPS_D)


@pytest.mark.parametrize("gate,policy", [(0.6, (0.0, 0)), (0.0, (0.9, 2)), (0.5, (0.9, 2))])
def test_designed_head_under_a_gate_and_a_policy(designed, gate, policy):
    pkg, m, org, pred, poc, refs = designed
    m.set_confidence_gate(128, gate)
    m.set_candidate_policy(128, *policy)
    try:
        dev = Device(pkg, m, 128, org, pred, poc)
        r0 = _reruns(m, 128)
        sw = dev.sweep(QPS_D)
        grew = _reruns(m, 128) - r0
        assert grew >= int(np.isin(poc, [3, 5, 9]).sum())
        _compare(f"gate {gate}, policy {policy}", sw, dev.twin, QPS_D)
        print(f"gate {gate}, policy {policy}: {grew} CUs re-run")
    finally:
        m.set_confidence_gate(128, 0.0)
        m.set_candidate_policy(128, 0.0, 0)


# ---- 3: one trunk pass -------------------------------------------------------------------------------------------------------------------------------------------
def _profile(m, call):
    m.profile_enable(True)
    call()
    got = {r["name"]: r["launches"] for r in m.profile_read()}
    m.profile_enable(False)
    return got


def test_one_trunk_pass(gpu):
    pkg = gpu
    Fl = pkg.capi
    n = 300
    m = pkg.MltCnn(device=0, sizes=(128,), blobs={128: _blob(pkg, 128)}, flags=Fl.FLAG_NO_CALIBRATION | Fl.FLAG_NO_DECISION_GUARD)
    a = m.arithmetic(128)
    assert a["exact"] == 0 and a["flat_guard"] == 1 and a["decision_guard"] == 0 and a["mag_guard_kind"] == 0, a
    poc = np.arange(n, dtype=np.int32) % 16
    for flagged in (False, True):
        if flagged:
            org, pred, n_flat = _mixed_content(pkg, 128, n)
        else:
            (org, pred), n_flat = pkg.synth.make_patches_bulk(128, n, 5), 0
        dev = Device(pkg, m, 128, org, pred, poc)
        dev.sweep(QPS_4); dev.twin(32)     # (buffers, plans and the exact pass's workspace exist before anything is counted)
        r0 = _reruns(m, 128)
        sweep = _profile(m, lambda: dev.sweep(QPS_4, want=("split", "logits")))
        assert _reruns(m, 128) - r0 == n_flat
        t = dev.torch
        d_qp = t.full((n,), 32, dtype=t.int32, device=dev.dev)
        o = dev._outputs(n)
        twin = _profile(m, lambda: (m.predict_batch_device(n, 128, dev.d[0].data_ptr(), dev.d[1].data_ptr(), dev.d[2].data_ptr(), d_qp.data_ptr(), o["split"].data_ptr(),
                                                            o["logits"].data_ptr()), m.synchronize()))
        passes = 2 if flagged else 1
        print(f"flagged {flagged}: sweep {sweep}\n  twin {twin}")
        assert sweep.get("heads_sweep") == passes and "heads" not in sweep, sweep
        assert twin.get("heads") == passes and "heads_sweep" not in twin, twin
        rest = lambda p: {k: v for k, v in p.items() if k not in ("heads", "heads_sweep", "guard_scatter")}
        assert rest(sweep) == rest(twin), (rest(sweep), rest(twin))     # every other kernel: as often as ONE twin call, not four
    m.close()


# ---- 4: chunks and shards ------------------------------------------------------------------------------------------------------------------------------------
def test_chunks_and_shards(gpu):
    pkg = gpu
    Fl = pkg.capi
    n, qps = 150, [37, 22, 30]
    blob = _blob(pkg, 128)
    org, pred, n_flat = _mixed_content(pkg, 128, n, seed=9)
    poc = (np.arange(n) % 7).astype(np.int32)
    m = pkg.MltCnn(device=0, sizes=(128,), blobs={128: blob}, flags=Fl.FLAG_NO_CALIBRATION, max_batch=64)     # 150 CUs: chunks of 64, 64, 22
    dev = Device(pkg, m, 128, org, pred, poc)
    r0 = _reruns(m, 128)
    sw = dev.sweep(qps)
    assert _reruns(m, 128) - r0 >= n_flat
    _compare("chunked device entry", sw, dev.twin, qps)
    p_org, p_pred, xy = _picture_pair(m, 128, org, pred)
    sp = m.predict_at_sweep(128, p_org, p_pred, xy, poc, qps)
    _compare("chunked picture entry", sp, lambda qp: m.predict_at(128, p_org, p_pred, xy, poc, np.full(n, qp, np.int32)), qps)
    p_org.close(); p_pred.close()
    m.close()
    m2 = pkg.MltCnn(sizes=(128,), blobs={128: blob}, devices=[0, 0], flags=Fl.FLAG_NO_CALIBRATION)
    assert m2.num_devices() == 2
    q_org, q_pred, xy2 = _picture_pair(m2, 128, org, pred)
    s2 = m2.predict_at_sweep(128, q_org, q_pred, xy2, poc, qps)
    for k in NAMES:
        assert s2[k].tobytes() == sp[k].tobytes(), f"two shards: {k} differs from the one-device bytes"
    q_org.close(); q_pred.close()
    m2.close()


# ---- 5: errors -----------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(gpu):
    pkg = gpu
    Fl = pkg.capi
    import torch
    n = 6
    m = pkg.MltCnn(device=0, sizes=(128,), blobs={128: _blob(pkg, 128)}, flags=Fl.FLAG_NO_CALIBRATION)
    lib, h = m._lib, m._h
    org, pred = pkg.synth.make_patches_bulk(128, n, 5)
    poc = np.zeros(n, np.int32)
    p_org, p_pred, xy = _picture_pair(m, 128, org, pred)
    good = np.array(QPS_4, np.int32)
    many = np.arange(33, dtype=np.int32)
    split = np.full((33 * n,), -7, np.int32)
    logits = np.full((33 * n, 9), F(-7), F)

    def at(size, xy_, qps_ptr, n_qps, s=split, l=logits):
        return lib.mlt_predict_at_sweep(h, size, p_org._h, p_pred._h, n, xy_.ctypes.data, poc.ctypes.data, qps_ptr, n_qps, None if s is None else s.ctypes.data,
                                        None if l is None else l.ctypes.data, None, None)
    ERR_ARG, ERR_SIZE = 1, 4
    assert at(128, xy, good.ctypes.data, 0) == ERR_ARG
    assert at(128, xy, many.ctypes.data, 33) == ERR_ARG
    assert at(128, xy, None, 4) == ERR_ARG
    assert at(128, xy, good.ctypes.data, 4, s=None, l=None) == ERR_ARG
    bad = xy.copy()
    bad[4] = (p_org.width - 127, 0)
    assert at(128, bad, good.ctypes.data, 4) == ERR_ARG
    msg = lib.mlt_last_error(h).decode()
    assert "position 4 " in msg and "mlt_predict_at_sweep" in msg, msg
    assert at(64, xy, good.ctypes.data, 4) == ERR_SIZE
    assert lib.mlt_predict_at_sweep(h, 128, p_org._h, p_pred._h, 0, None, None, good.ctypes.data, 4, split.ctypes.data, None, None, None) == 0     # n == 0
    assert (split == -7).all() and (logits == F(-7)).all()

    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (org, pred, poc)]
    d_split = torch.full((33 * n,), -7, dtype=torch.int32, device=dev)

    def batch(size, qps_ptr, n_qps, out=d_split):
        return lib.mlt_predict_batch_device_sweep(h, n, size, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), qps_ptr, n_qps, None if out is None else out.data_ptr(), None, None, None)
    assert batch(128, good.ctypes.data, 0) == ERR_ARG
    assert batch(128, many.ctypes.data, 33) == ERR_ARG
    assert batch(128, None, 4) == ERR_ARG
    assert batch(128, good.ctypes.data, 4, out=None) == ERR_ARG
    assert batch(64, good.ctypes.data, 4) == ERR_SIZE
    assert lib.mlt_predict_batch_device_sweep(h, 0, 128, None, None, None, good.ctypes.data, 4, d_split.data_ptr(), None, None, None) == 0
    m.synchronize()
    assert (d_split.cpu().numpy() == -7).all()
    # ... and the same context still answers
    assert batch(128, good.ctypes.data, 4) == 0
    m.synchronize()
    assert (d_split.cpu().numpy()[:4 * n] >= 0).all() and (d_split.cpu().numpy()[4 * n:] == -7).all()
    p_org.close(); p_pred.close()
    m.close()
