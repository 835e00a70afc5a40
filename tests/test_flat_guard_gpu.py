"""GPU (MI355X): the flat-content guard's statistic at its thresholds, per device implementation.

The statistic (csrc/mlt_kernels.h: near-flat and exactly flat quads per CU) is computed by four device implementations -- layer0_stream_kernel,
stem_block_kernel (<false> and the hi+lo-weights <true>), flat_stat_kernel<true> and flat_stat_kernel<false> -- chosen by size, batch size, tier
and alignment.  The inputs are the families of tests/flat_guard_families.py: every CU carries EXACTLY T or T - 1 exactly flat quads, or H or H - 1
near-flat ones, so a quad dropped or counted twice, a stale or uncleared sum, `<` for `<=` at the range or a wrong cast order changes a flag.

Observable, per configuration: a context with the flat guard as its only guard, and an exact context.  For every call
  (a) arithmetic()["guard_reruns"] grows by exactly the number of CUs synth.flat_guard_flags flags (the host restatement, held to the scalar
      reference on these very CUs when the families are built), and
  (b) CU i's logits and split are the exact context's bytes IF AND ONLY IF it is flagged.
(b) says which CUs the device flagged, (a) how many; an unflagged CU whose fast logits happened to equal the exact bytes would break (a) against (b)
and fail: no CU is excused.  Nothing here rests on a measured tolerance -- integer and byte equality only.  The one figure taken from the project
is the streaming launch's workgroup cap (256, read from the launch plan): the large batch has 2 x cap + 88 CUs.

Which launch computes the statistic is asserted per configuration from arithmetic() and the dispatcher's launch plan (mlt_plan_describe):
  128, seed 10, MLT_FLAG_NO_CALIBRATION, n >= 128, device entry   layer0_stream_kernel (five-stage form), 600 CUs in ONE launch: workgroups 0 .. 87 run three CUs
  the same through mlt_predict_batch                            layer0_stream_kernel on the host path's 512-CU sub-chunks (512 + 88)
  ... n = 100, n = 1, mlt_predict, deferred batches, pictures    stem_block_kernel<false>
  128, seed 21 (calibrated: hi+lo weights in layer0, 1, 3)       stem_block_kernel<true>
  128, seed 11 (calibrated: hi+lo weights in layer1)             layer0_stream_kernel, four-stage form (its own hand-over of the statistic)
  128, tolerance 2e-4 (exact-lite, 1/16)                         flat_stat_kernel<true>, S = 128
  64, MLT_FLAG_FAST_SMALL                                        stem_block_kernel<false>, H = 32
  32 / 16, MLT_FLAG_FAST_SMALL                                   flat_stat_kernel<true>, 256 / 64 quads for 256 threads
  128 / 16, device planes one int16 off 8-byte alignment         flat_stat_kernel<false>
stem_block_kernel<true>: of the committed seeds 13, 24, 11, 21 only 21 is calibrated into a tier with hi+lo weights in layer0.0 (test_hi_lo_weights_in_layer0
reads w2_units & 3 of all four on the device and asserts it); no forcing is needed.  mlt_predict gathers its CU into dense, aligned staging on the
host, so CUs cut at an odd column of a wider picture reach the device aligned: that call is checked for the same flags, but flat_stat_kernel<false>
is reached through the device-pointer entry only."""
import ctypes as C

import numpy as np
import pytest

import flat_guard_families as ff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


def _blob(pkg, size, seed=10):
    return pkg.weights.synthetic_blob(pkg.synth.arch_for_size(size), seed)


def _ctx(pkg, size, blob, **kw):
    return pkg.MltCnn(device=0, sizes=(size,), blobs={size: blob}, **kw)


def _plan(pkg, blob, size, n, tier=0, w2_units=0, x_units=0, aligned=3):
    """The dispatcher's launch plan (one detailed record per launch) for n CUs of `size` in the given tier."""
    lib = pkg.capi.load_library()
    lib.mlt_plan_describe.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 15)
    k = lib.mlt_plan_describe(blob, len(blob), size, n, tier, w2_units, x_units, aligned, buf, 1 << 15)
    lines = buf.value.decode().splitlines()
    assert k == len(lines) and k > 0
    return lines


def _plan_of(pkg, blob, size, n, a, aligned=3):
    """... in the tier arithmetic() reports (fp16 tiers only: the plan hook lists no statistic for the whole-network exact tiers)."""
    assert a["exact"] in (0, 2, 3, 4)
    return _plan(pkg, blob, size, n, 0, a["w2_units"], a["x_units"], aligned)


def _flat_div(a):
    """SizeState::flat_div (csrc/mlt_runtime.h): 16 for the exact-lite tier and for a tier admitted behind the magnitude guard, else 8."""
    return 16 if a["exact"] == 5 or a["mag_guard_kind"] == 2 else 8


def _reruns(m, size):
    return sum(m.arithmetic_of_device(i, size)["guard_reruns"] for i in range(m.num_devices()))


class Case:
    """A batch of family CUs, its expected flags (synth.flat_guard_flags) and the exact context's bytes for every CU."""

    def __init__(self, pkg, fam, blob, exact_flags):
        self.pkg, self.fam, self.size, self.n = pkg, fam, fam.size, len(fam)
        near, exact, self.flagged = pkg.synth.flat_guard_flags(fam.org, fam.pred, flat_div=fam.div)
        assert np.array_equal(near, fam.near) and np.array_equal(exact, fam.exact) and np.array_equal(self.flagged, fam.flagged)
        assert 0 < self.flagged.sum() < self.n
        self.poc, self.qp = pkg.synth.make_scalars(self.n, 4242)
        ex = _ctx(pkg, self.size, blob, flags=exact_flags)
        assert ex.arithmetic(self.size)["exact"] == 1
        self.ref_split, self.ref_logits = ex.predict_batch(fam.org, fam.pred, self.poc, self.qp)
        ex.close()
        assert np.isfinite(self.ref_logits).all()
        self._dev = {}

    def device(self, offset=0):
        """(org, pred, poc, qp) as device tensors; offset: the planes start that many int16 elements into their allocations."""
        import torch
        if offset not in self._dev:
            dev = torch.device("cuda", 0)
            planes = []
            for a in (self.fam.org, self.fam.pred):
                t = torch.zeros(a.size + 8, dtype=torch.int16, device=dev)
                t[offset:offset + a.size] = torch.from_numpy(np.array(a).reshape(-1)).to(dev)   # (a writable copy: the family arrays are read-only)
                planes.append(t)
            self._dev[offset] = (planes[0], planes[1], torch.from_numpy(self.poc).to(dev), torch.from_numpy(self.qp).to(dev))
        return self._dev[offset]

    def check(self, what, idx, split, logits, reruns):
        """(b) bytes equal the exact context's iff flagged, for the CUs idx of the batch in call order; (a) the counter advanced by their number."""
        idx = np.asarray(idx)
        split, logits = np.asarray(split, np.int32).reshape(len(idx)), np.asarray(logits, np.float32).reshape(len(idx), -1)
        same = (logits.view(np.uint32) == self.ref_logits[idx].view(np.uint32)).all(axis=1) & (split == self.ref_split[idx])
        want = self.flagged[idx]
        bad = np.flatnonzero(same != want)
        for j in bad[:16]:
            i = int(idx[j])
            print(f"{what}: CU {j} of the call (batch index {i}) {self.fam.label[i]}: intended near {self.fam.near[i]} exact {self.fam.exact[i]}, "
                  f"expected {'flagged' if want[j] else 'not flagged'}, device {'returned the exact bytes' if same[j] else 'kept the fast result'}")
        assert bad.size == 0, f"{what}: {bad.size} of {len(idx)} CUs on the wrong side of the guard"
        assert reruns == int(want.sum()), f"{what}: {reruns} re-runs, the reference flags {int(want.sum())}"

    def host(self, m, what, idx):
        idx = np.asarray(idx)
        r0 = _reruns(m, self.size)
        s, l = m.predict_batch(self.fam.org[idx], self.fam.pred[idx], self.poc[idx], self.qp[idx])
        self.check(what, idx, s, l, _reruns(m, self.size) - r0)

    def dev(self, m, what, n, offset=0, first=0):
        """mlt_predict_batch_device on CUs first .. first + n of the batch."""
        import torch
        o, p, poc, qp = self.device(offset)
        cs = self.size * self.size
        nl = m.num_logits(self.size)
        d_split = torch.full((n,), -7, dtype=torch.int32, device=o.device)
        d_lg = torch.zeros((n, nl), dtype=torch.float32, device=o.device)
        r0 = _reruns(m, self.size)
        m.predict_batch_device(n, self.size, o.data_ptr() + 2 * (offset + first * cs), p.data_ptr() + 2 * (offset + first * cs),
                               poc.data_ptr() + 4 * first, qp.data_ptr() + 4 * first, d_split.data_ptr(), d_lg.data_ptr())
        m.synchronize()
        self.check(what, np.arange(first, first + n), d_split.cpu().numpy(), d_lg.cpu().numpy(), _reruns(m, self.size) - r0)

    def single(self, m, what, idx, org=None, pred=None):
        """mlt_predict, one CU per call (org / pred: other views of the same CUs, e.g. cut out of a wider picture)."""
        for i in idx:
            r0 = _reruns(m, self.size)
            s, l = m.predict(self.fam.org[i] if org is None else org[i], self.fam.pred[i] if pred is None else pred[i], int(self.poc[i]), int(self.qp[i]))
            self.check(f"{what} (CU {i})", [i], [s], l, _reruns(m, self.size) - r0)


def _wg_cap0(pkg, blob):
    """The streaming launch's workgroup cap, from the plan of a batch that exceeds any cap."""
    line = _plan(pkg, blob, 128, 4096)[0]
    assert line.startswith("layer0_stream_h64")
    return int(line.split("grid=")[1].split()[0].rstrip("}"))


@pytest.fixture(scope="module")
def big(gpu):
    """128 x 128, seed 10, MLT_FLAG_NO_CALIBRATION | MLT_FLAG_NO_DECISION_GUARD: the single pass with the flat guard alone; 2 x cap + 88 = 600 CUs of all families."""
    pkg = gpu
    blob = _blob(pkg, 128)
    cap = _wg_cap0(pkg, blob)
    assert cap == 256
    case = Case(pkg, ff.batch(pkg, 128, 8, 2 * cap + 88), blob, pkg.capi.FLAG_EXACT_128)
    m = _ctx(pkg, 128, blob, flags=pkg.capi.FLAG_NO_CALIBRATION | pkg.capi.FLAG_NO_DECISION_GUARD)
    a = m.arithmetic(128)
    assert a["exact"] == 0 and a["calibrated"] == 0 and a["flat_guard"] == 1 and a["decision_guard"] == 0 and a["mag_guard_kind"] == 0 and _flat_div(a) == 8, a
    yield case, m, blob, cap, a
    m.close()


def test_streaming_kernel_three_cus_per_workgroup(big):
    """layer0_stream_kernel: per half-wave ballots summed into two alternating LDS slots per persistent workgroup, handed to a.flat with the CU's last row.
    600 CUs in one launch of 256 workgroups: workgroups 0 .. 87 run CUs b, b + 256, b + 512 and reuse a slot for the third; then the prefixes."""
    case, m, blob, cap, a = big
    n = case.n
    assert n == 2 * cap + 88 == 600
    for k in (n, 513, 257, 129, 128):
        p = _plan_of(case.pkg, blob, 128, k, a)
        assert p[0].startswith("layer0_stream_h64(stem+layer0+layer1.0.conv1+sc)") and f"grid={min(k, cap)}" in p[0] and "flat=0x2000" in p[0] and "flat_is_clear=0" in p[0], p[0]
        assert not any(l.startswith("guard_flat_stat") for l in p)
    # flagged and unflagged CUs alternate inside a workgroup's sequence: a sum carried over, or a slot not cleared, has CUs to show on
    f = case.flagged
    seqs = {(bool(f[b]), bool(f[b + cap]), bool(f[b + 2 * cap])) for b in range(n - 2 * cap)}
    assert {(True, False, True), (False, True, False), (False, False, True), (True, True, False)} <= seqs, seqs
    case.dev(m, "stream n = 600", n)
    case.dev(m, "stream n = 600 again", n)
    for k in (128, 129, 257, 513):
        case.dev(m, f"stream prefix {k}", k)
    case.host(m, "stream, host entry (512 + 88)", np.arange(n))
    case.dev(m, "stream, CUs 300 .. 599", 300, first=300)


def test_tiled_kernel_and_latency_path(big):
    """stem_block_kernel<false>: raw patches with a halo, the "own quad" bit so that halo quads count once, one atomicAdd per wave into the pre-cleared a.flat[n].
    n = 100 (tiled launches) and n = 1 (the latency variants behind the same first kernel)."""
    case, m, blob, cap, a = big
    for k in (100, 1):
        p = _plan_of(case.pkg, blob, 128, k, a)
        assert p[0].startswith("stem+block_s2_2to32_h64(layer0.0) [single pass") and "flat=0x2000" in p[0] and "flat_is_clear=0" in p[0], p[0]
        assert not any(l.startswith("guard_flat_stat") or l.startswith("layer0_stream") for l in p)
    assert all("latency tiles" in l for l in _plan_of(case.pkg, blob, 128, 1, a)[3:14])
    for lo in (0, 100, 200, 300, 400, 500):
        case.dev(m, f"tiled n = 100, CUs {lo} ..", 100, first=lo)
    case.host(m, "tiled n = 100, host entry", np.arange(100))
    for i in range(0, 48):
        case.dev(m, f"n = 1, CU {i}", 1, first=i)


def test_hi_lo_weights_in_layer0(gpu):
    """stem_block_kernel<true>: a calibrated tier with hi+lo weights in layer0.0.  Which of the committed seeds lands in one is read on the device (w2_units & 3 of
    seeds 13, 24, 11, 21) and asserted: seed 21 does (hi+lo weights in layer0, layer1 and layer3, layer2 exact), the other three keep layer0 on the single pass."""
    pkg = gpu
    F = pkg.capi
    found, m = {}, None
    for seed in (13, 24, 11, 21):
        c = _ctx(pkg, 128, _blob(pkg, 128, seed), flags=F.FLAG_NO_DECISION_GUARD | F.FLAG_NO_MAGNITUDE_GUARD)
        found[seed] = c.arithmetic(128)["w2_units"] & 3
        if found[seed] & 1 and m is None:
            m, blob = c, _blob(pkg, 128, seed)
        else:
            c.close()
    assert found == {13: 0, 24: 0, 11: 0, 21: 3}, found
    a = m.arithmetic(128)
    assert a["calibrated"] == 1 and a["exact"] in (2, 3, 4) and (a["x_units"] & 3) == 0 and a["flat_guard"] == 1 and a["decision_guard"] == 0 and a["mag_guard_kind"] == 0, a
    div = _flat_div(a)
    assert div == 8
    case = Case(pkg, ff.family(pkg, 128, div), blob, F.FLAG_EXACT_128)
    for k in (600, case.n, 1):   # (no streaming form of the two-plane layer0: large batches run the tiled kernel too)
        p = _plan_of(pkg, blob, 128, k, a)
        assert p[0].startswith("stem+block_s2_2to32_h64(layer0.0) [hi+lo weights") and "flat=0x2000" in p[0], p[0]
        assert not any(l.startswith("guard_flat_stat") or l.startswith("layer0_stream") for l in p)
    case.dev(m, "hi+lo weights in layer0, whole family", case.n)
    case.host(m, "hi+lo weights in layer0, host entry", np.arange(case.n))
    for i in range(0, 16):
        case.dev(m, f"hi+lo weights in layer0, n = 1, CU {i}", 1, first=i)
    case.single(m, "hi+lo weights in layer0, mlt_predict", range(0, case.n, 7))
    m.close()


def test_four_stage_streaming_form(gpu):
    """layer0_stream_kernel without the fifth stage (a tier with hi+lo weights in layer1: layer0's output goes to HBM) hands the statistic over in its own
    place.  Seed 11 is calibrated into such a tier; 2 x 256 + 88 CUs in one launch again."""
    pkg = gpu
    F = pkg.capi
    blob = _blob(pkg, 128, 11)
    m = _ctx(pkg, 128, blob, flags=F.FLAG_NO_DECISION_GUARD | F.FLAG_NO_MAGNITUDE_GUARD)
    a = m.arithmetic(128)
    assert a["exact"] == 3 and (a["w2_units"] & 3) == 0 and (a["w2_units"] & 0xC) and a["x_units"] == 0 and a["flat_guard"] == 1 and a["mag_guard_kind"] == 0, a
    div = _flat_div(a)
    assert div == 8
    case = Case(pkg, ff.batch(pkg, 128, div, 600), blob, F.FLAG_EXACT_128)
    p = _plan_of(pkg, blob, 128, 600, a)
    assert p[0].startswith("layer0_stream_h64(stem+layer0.0+layer0.1)") and "grid=256" in p[0] and "flat=0x2000" in p[0], p[0]
    case.dev(m, "four-stage stream n = 600", 600)
    case.dev(m, "four-stage stream n = 257", 257)
    m.close()


def test_exact_lite_tier_standalone_kernel_at_one_sixteenth(gpu):
    """flat_stat_kernel<true> at S = 128 (4096 quads for 256 threads), thresholds at Q // 16: a tolerance no fp16 tier meets lands in the exact-lite tier."""
    pkg = gpu
    F = pkg.capi
    blob = _blob(pkg, 128)
    m = _ctx(pkg, 128, blob, tolerance=2e-4, flags=F.FLAG_NO_DECISION_GUARD | F.FLAG_NO_MAGNITUDE_GUARD)
    a = m.arithmetic(128)
    assert a["exact"] == 5 and a["flat_guard"] == 1 and a["decision_guard"] == 0 and a["mag_guard_kind"] == 0, a
    div = _flat_div(a)
    assert div == 16     # (csrc/mlt_runtime.h: 16 iff the exact-lite tier or a tier admitted behind the magnitude guard)
    fam = ff.family(pkg, 128, div)
    assert ff.thresholds(128, div)[1] == 256
    case = Case(pkg, fam, blob, F.FLAG_EXACT_128)
    case.dev(m, "exact-lite, whole family", case.n)
    case.host(m, "exact-lite, host entry", np.arange(case.n))
    case.dev(m, "exact-lite, n = 1", 1, first=3)
    case.single(m, "exact-lite, mlt_predict", range(0, case.n, 11))
    # the same CUs against the thresholds of 1/8 would be another set of flags: the divisor is part of what is checked
    assert not np.array_equal(pkg.synth.flat_guard_flags(fam.org, fam.pred, flat_div=8)[2], case.flagged)
    m.close()


@pytest.mark.parametrize("size", (64, 32, 16))
def test_small_models_fast(gpu, size):
    """MLT_FLAG_FAST_SMALL: 64 x 64 runs stem_block_kernel (H = 32: one tile row pair per CU), 32 x 32 and 16 x 16 the standalone flat_stat_kernel<true>
    with 256 and 64 quads -- fewer than the workgroup has threads.  n = 70 and n = 1 (and the whole family where it has more than 70 CUs)."""
    pkg = gpu
    F = pkg.capi
    blob = _blob(pkg, size)
    m = _ctx(pkg, size, blob, flags=F.FLAG_FAST_SMALL | F.FLAG_NO_DECISION_GUARD)
    a = m.arithmetic(size)
    assert a["exact"] == 0 and a["flat_guard"] == 1 and a["decision_guard"] == 0 and a["mag_guard_kind"] == 0 and _flat_div(a) == 8, a
    case = Case(pkg, ff.batch(pkg, size, 8, len(ff.family(pkg, size, 8))), blob, F.FLAG_NO_CALIBRATION)
    assert case.n >= 70
    for k in (70, 1):
        p = _plan_of(pkg, blob, size, k, a)
        if size == 64:
            assert p[0].startswith("stem+block_s2_2to32_h32(layer0.0) [single pass") and "flat=0x2000" in p[0], p[0]
            assert not any(l.startswith("guard_flat_stat") for l in p)
        else:
            assert p[0].startswith("guard_flat_stat") and "quads=1" in p[0] and p[1].startswith("stem5x5"), p[:2]
    case.dev(m, f"{size}: n = 70", 70)
    if case.n > 70:
        case.dev(m, f"{size}: whole family", case.n)
    case.host(m, f"{size}: host entry", np.arange(70))
    for i in range(24):
        case.dev(m, f"{size}: n = 1, CU {i}", 1, first=i)
    case.single(m, f"{size}: mlt_predict", range(24, 40))
    m.close()


@pytest.mark.parametrize("size", (128, 16))
def test_unaligned_planes(gpu, size):
    """flat_stat_kernel<false> (2-byte loads): device planes whose data pointers are one int16 past an 8-byte boundary.  And mlt_predict on CUs cut at an odd
    column of a wider host picture (gathered into aligned staging by the host: same flags)."""
    pkg = gpu
    F = pkg.capi
    blob = _blob(pkg, size)
    m = _ctx(pkg, size, blob, flags=(F.FLAG_NO_CALIBRATION if size == 128 else F.FLAG_FAST_SMALL) | F.FLAG_NO_DECISION_GUARD)
    a = m.arithmetic(size)
    assert a["exact"] == 0 and a["flat_guard"] == 1 and _flat_div(a) == 8
    case = Case(pkg, ff.family(pkg, size, 8), blob, F.FLAG_EXACT_128 if size == 128 else F.FLAG_NO_CALIBRATION)
    for k in (case.n, 1):
        p = _plan_of(pkg, blob, size, k, a, aligned=2)
        assert p[0].startswith("guard_flat_stat") and "quads=0" in p[0] and p[1].startswith("stem5x5"), p[:2]
    o, _, _, _ = case.device(1)
    assert (o.data_ptr() + 2) % 8 == 2
    case.dev(m, f"{size}: unaligned, whole family", case.n, offset=1)
    case.dev(m, f"{size}: unaligned, n = 1", 1, offset=1, first=5)
    case.dev(m, f"{size}: aligned again", case.n)
    pick = list(range(0, case.n, 9))
    wide_o = np.random.default_rng(5).integers(0, 1024, (len(pick), size, size + 24)).astype(np.int16)
    wide_p = np.random.default_rng(6).integers(0, 1024, (len(pick), size, size + 10)).astype(np.int16)
    wide_o[:, :, 7:7 + size] = case.fam.org[pick]
    wide_p[:, :, 3:3 + size] = case.fam.pred[pick]
    case.single(m, f"{size}: mlt_predict at odd columns", pick, org={i: wide_o[j, :, 7:7 + size] for j, i in enumerate(pick)},
                pred={i: wide_p[j, :, 3:3 + size] for j, i in enumerate(pick)})
    m.close()


def test_statistic_does_not_survive_from_call_to_call(big):
    """mlt_predict's captured graph has no memset of the statistic: the heads kernel's tail consumes and clears it.  T - 1 x 3, T, T - 1, unaligned T - 1,
    unaligned T, aligned T - 1, T: the re-run counter advances at the T calls only (a sum that survived a replay would flag the second T - 1 call)."""
    import torch
    case, m, blob, cap, a = big
    lab = case.fam.label
    t_cus = [i for i in range(case.n) if lab[i].startswith("E/") and "/T#" in lab[i]]
    u_cus = [i for i in range(case.n) if lab[i].startswith("E/") and "/T-1#" in lab[i]]
    assert len(t_cus) >= 3 and len(u_cus) >= 6 and case.flagged[t_cus].all() and not case.flagged[u_cus].any()
    assert all(case.fam.exact[i] == 512 for i in t_cus[:3]) and all(case.fam.exact[i] == 511 for i in u_cus[:6])
    S = 128

    def unaligned(i):   # the CU inside a wider picture at an odd column, from a buffer that is itself one int16 off
        buf = np.random.default_rng(i).integers(0, 1024, 1 + S * (S + 6)).astype(np.int16)
        o = buf[1:].reshape(S, S + 6)[:, 3:3 + S]
        o[:] = case.fam.org[i]
        buf2 = np.random.default_rng(i + 1).integers(0, 1024, 1 + S * (S + 2)).astype(np.int16)
        p = buf2[1:].reshape(S, S + 2)[:, 1:1 + S]
        p[:] = case.fam.pred[i]
        return {i: o}, {i: p}

    seq = [(u_cus[0], False), (u_cus[1], False), (u_cus[2], False), (t_cus[0], False), (u_cus[3], False), (u_cus[4], True), (t_cus[1], True), (u_cus[5], False), (t_cus[2], False)]
    r_start = _reruns(m, S)
    for step, (i, odd) in enumerate(seq):
        o, p = unaligned(i) if odd else (None, None)
        case.single(m, f"mlt_predict sequence, step {step}", [i], org=o, pred=p)
    assert _reruns(m, S) - r_start == 3
    # the device entry with n = 1 uses the batch slot, mlt_predict its own: interleaved, aligned and not, neither leaves a sum to the other
    for step, (i, odd) in enumerate(seq):
        case.dev(m, f"device n = 1 sequence, step {step}", 1, offset=1 if odd else 0, first=i)
        case.single(m, f"interleaved mlt_predict, step {step}", [seq[(step + 4) % len(seq)][0]])
    # a batch, then single CUs again (the batch's slot and the single-CU slot are different words)
    case.dev(m, "batch between single calls", 100)
    case.single(m, "mlt_predict after a batch", [u_cus[0], t_cus[0], u_cus[1]])


def test_chunk_loop_selection_kernel_and_deferred_batches(big, monkeypatch):
    """Host state around the statistic: ragged chunks of the device entry (MLT_CHUNK=200: 200 + 200 + 200 on 600 CUs, every chunk a
    streaming launch of its own; 200 + 200 + 50 on 450, the last chunk tiled), the selection as a launch of its own (MLT_GUARD_SELECT_KERNEL=1: reads the statistic without clearing it), deferred batches of 24."""
    case, m, blob, cap, a = big
    pkg = case.pkg
    flags = pkg.capi.FLAG_NO_CALIBRATION | pkg.capi.FLAG_NO_DECISION_GUARD
    monkeypatch.setenv("MLT_TUNING", "1")
    monkeypatch.setenv("MLT_CHUNK", "200")
    mc = _ctx(pkg, 128, blob, flags=flags)
    monkeypatch.delenv("MLT_CHUNK")
    monkeypatch.setenv("MLT_GUARD_SELECT_KERNEL", "1")
    ms = _ctx(pkg, 128, blob, flags=flags)
    monkeypatch.delenv("MLT_GUARD_SELECT_KERNEL")
    monkeypatch.delenv("MLT_TUNING")
    case.dev(mc, "MLT_CHUNK=200, device entry", case.n)
    case.host(mc, "MLT_CHUNK=200, host entry", np.arange(case.n))
    case.dev(mc, "MLT_CHUNK=200, 450 CUs (200 + 200 + 50: the last chunk tiled)", 450)
    mc.close()
    case.dev(ms, "guard_select_kernel, n = 600", case.n)
    case.dev(ms, "guard_select_kernel, n = 100", 100)
    case.dev(ms, "guard_select_kernel, n = 100 again (nothing clears the statistic but the next call's memset)", 100)
    case.dev(ms, "guard_select_kernel, n = 1", 1, first=2)
    case.single(ms, "guard_select_kernel context, mlt_predict", range(0, 12))
    ms.close()
    # mlt_submit / mlt_flush / mlt_wait: 24 CUs of mixed families, twice (the second generation finds the first one's statistic in the other buffer set)
    for lo in (0, 24, 48):
        idx = list(range(lo, lo + 24))
        assert 0 < case.flagged[idx].sum() < 24
        r0 = _reruns(m, 128)
        tk = [m.submit(case.fam.org[i], case.fam.pred[i], int(case.poc[i]), int(case.qp[i])) for i in idx]
        m.flush(128)
        out = [m.wait(128, t) for t in tk]
        case.check(f"deferred batch {lo} ..", idx, [o[0] for o in out], np.stack([o[1] for o in out]), _reruns(m, 128) - r0)


def test_two_shards_on_one_device(big):
    """A devices = [0, 0] context splits the batch into contiguous shards, one per device context: the per-CU statistic must not shift with the shard."""
    case, m, blob, cap, a = big
    pkg = case.pkg
    m2 = pkg.MltCnn(devices=[0, 0], sizes=(128,), blobs={128: blob}, flags=pkg.capi.FLAG_NO_CALIBRATION | pkg.capi.FLAG_NO_DECISION_GUARD)
    assert m2.num_devices() == 2
    for i in range(2):
        ai = m2.arithmetic_of_device(i, 128)
        assert ai["exact"] == 0 and ai["flat_guard"] == 1 and ai["decision_guard"] == 0
    case.host(m2, "two shards, n = 600", np.arange(case.n))
    case.host(m2, "two shards, n = 301", np.arange(301))
    m2.close()


def test_pictures_feed_the_same_dense_path(big):
    """12 E-family CUs of 128 x 128 tiled into a 512 x 384 picture pair: mlt_predict_at on mlt_grid_positions gathers them into the dense staging the batch
    path consumes -- the same flags, the same bytes as the dense call on the same CUs."""
    case, m, blob, cap, a = big
    pkg = case.pkg
    idx = [i for i in range(case.n) if case.fam.label[i].startswith("E/")][:12]
    assert len(idx) == 12 and 0 < case.flagged[idx].sum() < 12
    xy = pkg.capi.grid_positions(512, 384, 128)
    assert xy.shape == (12, 2)
    org = np.zeros((384, 512), np.int16)
    pred = np.zeros((384, 512), np.int16)
    for (x, y), i in zip(xy, idx):
        org[y:y + 128, x:x + 128] = case.fam.org[i]
        pred[y:y + 128, x:x + 128] = case.fam.pred[i]
    po, pp = m.picture(512, 384).upload(org), m.picture(512, 384).upload(pred)
    r0 = _reruns(m, 128)
    out = m.predict_at(128, po, pp, xy, case.poc[idx], case.qp[idx], want=("split", "logits"))
    case.check("predict_at on the grid", idx, out["split"], out["logits"], _reruns(m, 128) - r0)
    s, l = m.predict_batch(case.fam.org[idx], case.fam.pred[idx], case.poc[idx], case.qp[idx])
    assert out["split"].tobytes() == s.tobytes() and out["logits"].tobytes() == l.tobytes()
    po.close(); pp.close()
