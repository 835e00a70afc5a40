"""GPU (MI355X): every arithmetic tier, every mixture of them and every hand-off between their launch units against float64, on weights for which no tier
rounds (tests/shift_weights.py; the conditions and the tolerance are established on the CPU by tests/test_shift_cpu.py).

With the shift weights every activation of an impulse CU is a short sum of equal powers of two: the single pass, hi+lo weights, the exact and exact-lite
arithmetic and every mixed plan must land on G[k, plane, y, x] x amplitude to RHO_SHIFT ~ 1e-6 -- three orders of magnitude below the tracer weights' rho_fast, the
tolerance every mixed plan had so far.  A lo plane read where zeros were meant, a wrong tap, a wrong stride-2 phase, a wrong padding row, a wrong channel half
of a chunk-major hand-off are errors of per cents of a response.

Per configuration, before it is trusted: arithmetic() reports exactly the intended exact / w2_units / x_units, and the launch plan for those masks names the
kernels of that arithmetic, unit by unit.  All guards are off (an impulse CU is flat: the flat guard would re-run every one exactly).

Assertions (_hold): every CU and every logit with a non-zero expectation within RHO_SHIFT relative; every logit whose expectation is exactly 0 exactly 0.0 on the
device.  Across configurations: the subset's logits agree between any two configurations of a size to 2 x RHO_SHIFT.  Stale planes: in every mixed context and
in the exact one a call of n dense CUs, then the same n as impulse and zero CUs, then n / 2 (the workspace is carved by n: the second call lands on the first
call's lo planes), n = 96 and 600.  Power: the device's own single-pass sweep is beyond 10 x RHO_SHIFT of the adjoint of each of the eight single-pixel mutations.

docs/NUMERICS.md ("Rounding-free weights") has the device's figures."""
import time

import numpy as np
import pytest

import shift_weights as ws
import tracer_weights as tw

pytestmark = pytest.mark.gpu
CHUNK = 4096
_REF, _BLOB = {}, {}
_SUBSET = {}          # {(size, tap set): {configuration: logits of the subset, amplitudes 512 and 37}}
_SPREAD = {}          # {(size, tap set): largest pairwise |a - b| / expected met so far}
_SWEEPS = {}          # {tap set: (plane, pos, logits)} of the 128 single-pass full sweeps
SUBSET_AMPS = (512, 37)


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


def G_of(size, tapset=0):
    if (size, tapset) not in _REF:
        _REF[(size, tapset)] = ws.adjoint(ws.shift_state_dict(size, tapset), size)
    return _REF[(size, tapset)]


def _blob(size, tapset=0, low=False):
    key = (size, tapset, low)
    if key not in _BLOB:
        _BLOB[key] = ws.shift_blob(size, tapset, ws.stem_gain(size, 1 if low else 512))
    return _BLOB[key]


def OFF(F):
    return F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD | F.FLAG_NO_MAGNITUDE_GUARD


def _ctx(pkg, size, tapset=0, low=False, **kw):
    return pkg.MltCnn(device=0, sizes=(size,), blobs={size: _blob(size, tapset, low)}, **kw)


def _forced(pkg, monkeypatch, size, env, tapset=0):
    """A context whose tier the tuning switches force (set around the constructor only): no calibration flag, every guard off; the realisation of the weights'
    rounding pinned; a tolerance no fp16 tier can meet where the search reaches the forced mask only after everything cheaper has failed."""
    env = dict(env, MLT_TUNING="1", MLT_ROUNDING="0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return _ctx(pkg, size, tapset, flags=OFF(pkg.capi), tolerance=1e-30 if ws.needs_tolerance(env) else 0.0)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _run(m, org, pred, step=CHUNK):
    n = len(org)
    z = np.zeros(n, np.int32)
    return np.concatenate([m.predict_batch(org[i:i + step], pred[i:i + step], z[i:i + step], z[i:i + step])[1] for i in range(0, n, step)])


def _cus(size, plane, pos, amp):
    """org, pred of impulse CUs of mixed planes (plane 0: org = pred = amp at the pixel; plane 1: pred alone)."""
    m = len(pos)
    org = np.zeros((m, size * size), np.int16)
    pred = np.zeros((m, size * size), np.int16)
    r = np.arange(m)
    pred[r, pos] = amp
    o = plane == 0
    org[r[o], pos[o]] = amp
    return org.reshape(m, size, size), pred.reshape(m, size, size)


def _hold(what, size, got, want, describe):
    """Non-zero expectations: |got - want| / want <= RHO_SHIFT; zero expectations: exactly 0.0.  Prints the per-head worst; -> the worst over all heads / rho."""
    rho = ws.RHO_SHIFT[size]
    hk = tw.head_of_logit(tw.arch_of(size))
    assert got.shape == want.shape and got.dtype == np.float32 and (want >= 0).all()
    assert np.isfinite(got).all(), f"{what}: non-finite logits"
    zero = want == 0.0
    dirty = np.argwhere(zero & (got != 0.0))
    for i, k in dirty[:8]:
        print(f"  {what}: CU {i} {describe(int(i))} logit {k}: device {got[i, k]:.9g}, expected exactly 0")
    assert len(dirty) == 0, f"{what}: {len(dirty)} logits whose expectation is exactly 0 are not 0.0 on the device"
    rel = np.where(zero, 0.0, np.abs(got.astype(np.float64) - want) / np.where(zero, 1.0, want))
    heads = [float(rel[:, hk == h].max()) for h in range(hk.max() + 1)]
    print(f"{what}: {len(got)} CUs ({int(zero.sum())} logits exactly 0); worst relative error per head {[f'{v:.2e}' for v in heads]} = {[f'{v / rho:.2f}' for v in heads]} x rho_shift")
    over = rel / rho
    if (over > 1).any():
        for i, k in zip(*np.unravel_index(np.argsort(over, axis=None)[::-1][:16], over.shape)):
            if over[i, k] > 1:
                print(f"  {what}: CU {i} {describe(int(i))} logit {k}: device {got[i, k]:.9g} expected {want[i, k]:.9g} relative {rel[i, k]:.3e} = {over[i, k]:.1f} x rho_shift")
    bad = (over > 1).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(got)} CUs beyond rho_shift (worst {over.max():.1f} x)"
    return max(heads) / rho


def _subset(size):
    sub = tw.subset_positions(size)
    order = np.random.default_rng([size, 9]).permutation(2 * len(sub))
    return np.repeat([0, 1], len(sub))[order], np.tile(sub, 2)[order]


def _sample(size):
    pos = tw.sample_positions(size, 24, 40)
    return np.repeat([0, 1], len(pos)), np.tile(pos, 2)


def _subset_run(what, m, size, tapset=0, amps=SUBSET_AMPS, step=CHUNK, low=False, record=None):
    """The 512-position subset of both planes at each amplitude; record: the name under which the logits enter the comparison across configurations."""
    G = G_of(size, tapset) * (ws.STEM_LOW if low else 1.0)
    gots, wants = [], []
    for amp in amps:
        # (37 is rounding-free where the CPU test has held it: on the subset for tap set 0, on the family's sample positions for the others)
        plane, pos = _subset(size) if amp != 37 or tapset == 0 else _sample(size)
        got = _run(m, *_cus(size, plane, pos, amp), step=step)
        want = tw.expected_impulse(G, plane, pos, amp)
        _hold(f"{what}, amplitude {amp}", size, got, want, lambda i: f"plane {plane[i]} ({pos[i] // size},{pos[i] % size})")
        gots.append(got); wants.append(want)
    got, want = np.concatenate(gots), np.concatenate(wants)
    if record is not None:
        assert tuple(amps) == SUBSET_AMPS and not low
        key = (size, tapset)
        for other, o in _SUBSET.setdefault(key, {}).items():
            d = np.abs(got.astype(np.float64) - o.astype(np.float64))
            assert (d[want == 0.0] == 0.0).all()
            worst = float((d[want > 0] / want[want > 0]).max())
            _SPREAD[key] = max(_SPREAD.get(key, 0.0), worst)
            assert worst <= 2 * ws.RHO_SHIFT[size], f"{record} against {other}: the subset's logits differ by {worst:.3e} relative = {worst / ws.RHO_SHIFT[size]:.1f} x rho_shift"
        _SUBSET[key][record] = got
    return got


def _sweep(what, m, size, tapset=0, amp=512):
    plane, pos = tw.sweep(size)
    got = np.concatenate([_run(m, *_cus(size, plane[i:i + CHUNK], pos[i:i + CHUNK], amp)) for i in range(0, len(pos), CHUNK)])
    assert len(got) == 2 * size * size
    _hold(what, size, got, tw.expected_impulse(G_of(size, tapset), plane, pos, amp), lambda i: f"plane {plane[i]} ({pos[i] // size},{pos[i] % size})")
    return plane, pos, got


def _stale(what, pkg, m, size, tapset=0):
    """n dense CUs, then the SAME n as impulse and zero CUs, then n / 2 of them: the second call's lo planes are the first call's."""
    G = G_of(size, tapset)
    plane, pos = _subset(size)
    for n in ws.STALE_N:
        do, dp = pkg.synth.make_patches_bulk(size, n, 33)
        dense = _run(m, do, dp)
        assert np.isfinite(dense).all() and (dense != 0).any()
        zero = tw.leakage_family(size, n, n // 8)[2]
        org, pred = _cus(size, plane[:n], pos[:n], 512)
        org[zero] = 0; pred[zero] = 0
        want = tw.expected_impulse(G, plane[:n], pos[:n], 512)
        want[zero] = 0.0
        assert int(zero.sum()) == n // 8 + 2 and (want[~zero] > 0).any()
        for k in (n, n // 2):
            got = _run(m, org[:k], pred[:k])
            assert (got[zero[:k]] == 0.0).all(), f"{what}: zero CUs behind a dense call of {n} have non-zero logits (call of {k})"
            _hold(f"{what}, {k} impulse / zero CUs behind {n} dense", size, got, want[:k], lambda i: f"batch index {i} plane {plane[i]} ({pos[i] // size},{pos[i] % size})")


def _check(pkg, m, size, exact, w2_units, x_units, n=CHUNK, tapset=0):
    a = m.arithmetic(size)
    assert (a["exact"], a["w2_units"], a["x_units"]) == (exact, w2_units, x_units), (a, hex(w2_units), hex(x_units))
    assert a["flat_guard"] == 0 and a["decision_guard"] == 0 and a["mag_guard_kind"] == 0, a
    if size == 128 and (w2_units or x_units):
        ws.check_plan_arithmetic(ws.plan_lines(pkg, _blob(size, tapset), size, n, 0, w2_units, x_units), w2_units, x_units)
    return a


# ---- 128 x 128, uniform ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tapset", ws.TAPSETS)
def test_128_single_pass_full_sweep(gpu, tapset):
    pkg = gpu
    m = _ctx(pkg, 128, tapset, flags=OFF(pkg.capi) | pkg.capi.FLAG_NO_CALIBRATION)
    a = _check(pkg, m, 128, 0, 0, 0)
    assert a["calibrated"] == 0
    p = ws.plan_lines(pkg, _blob(128, tapset), 128, CHUNK)
    assert [l.split("(")[0] for l in p[:4]] == ["layer0_stream_h64", "layer1_stream_h32", "stage_128_h16", "stage_256_h8"] and all("single pass" in l for l in p[1:4]), p
    t0 = time.time()
    _SWEEPS[tapset] = _sweep(f"128 single pass, tap set {tapset}, full sweep", m, 128, tapset)
    _subset_run(f"128 single pass, tap set {tapset}, subset", m, 128, tapset, record="single pass")
    if tapset == 0:
        for step in (100, 16, 1):
            names = [l.split(" [")[0] for l in ws.plan_lines(pkg, _blob(128), 128, step)]
            assert names[0].startswith("stem+block_s2_2to32_h64") and (len(names) == 15) == (step != 100), (step, names)
            _subset_run(f"128 single pass, subset in calls of {step}", m, 128, amps=(512,) if step == 1 else SUBSET_AMPS, step=step, record=None if step == 1 else f"single pass, calls of {step}")
    assert m.arithmetic(128)["guard_reruns"] == 0
    m.close()
    print(f"128 single pass, tap set {tapset}: {time.time() - t0:.1f} s")


def test_128_single_pass_masked_padding(gpu, monkeypatch):
    pkg = gpu
    monkeypatch.setenv("MLT_TUNING", "1")
    monkeypatch.setenv("MLT_NO_LDS_OOB", "1")
    m = _ctx(pkg, 128, flags=OFF(pkg.capi) | pkg.capi.FLAG_NO_CALIBRATION)
    monkeypatch.delenv("MLT_NO_LDS_OOB")
    monkeypatch.delenv("MLT_TUNING")
    _check(pkg, m, 128, 0, 0, 0)
    _subset_run("128 single pass, masked padding, subset", m, 128, record="single pass, masked padding")
    _subset_run("128 single pass, masked padding, subset in calls of 100", m, 128, step=100, record="single pass, masked padding, calls of 100")
    m.close()


def test_128_single_pass_sweep_tells_every_mutation_from_the_network(gpu):
    """Against the adjoint of a network with ONE output pixel of ONE layer scaled by 8 / 9 the device's own sweep is beyond 10 x rho_shift at some CU, for each of
    the eight mutations (in the first tap set, the centre set first, that has a path through the pixel)."""
    assert sorted(_SWEEPS) == list(ws.TAPSETS), "run the whole module: the sweeps of test_128_single_pass_full_sweep are compared here"
    rho = ws.RHO_SHIFT[128]
    for name, mut in tw.mutations(128):
        worst = 0.0
        for ts in (ws.CENTRE,) + tuple(t for t in ws.TAPSETS if t != ws.CENTRE):     # (the centre set has a path through every pixel of every map)
            plane, pos, got = _SWEEPS[ts]
            want = tw.expected_impulse(ws.adjoint(ws.shift_state_dict(128, ts), 128, mutation=mut, check=False), plane, pos, 512)
            nz = want > 0
            over = np.abs(got.astype(np.float64) - want)[nz] / want[nz] / rho
            worst = max(worst, float(over.max()))
            print(f"mutation {name}, tap set {ts}: {int((over > 10).sum())} logits of the device's sweep beyond 10 x rho_shift (worst {over.max():.0f} x)")
            if worst > 10:
                break
        assert worst > 10, name


def test_128_single_pass_amplitude_1(gpu):
    pkg = gpu
    m = _ctx(pkg, 128, low=True, flags=OFF(pkg.capi) | pkg.capi.FLAG_NO_CALIBRATION)
    _check(pkg, m, 128, 0, 0, 0)
    _subset_run("128 single pass, stem x 1024", m, 128, amps=(1,), low=True)
    _subset_run("128 single pass, stem x 1024, calls of 100", m, 128, amps=(1,), low=True, step=100)
    m.close()


@pytest.mark.parametrize("tapset", ws.TAPSETS)
def test_128_hi_lo_weights_everywhere(gpu, monkeypatch, tapset):
    pkg = gpu
    m = _forced(pkg, monkeypatch, 128, {"MLT_W2_MASK": "15"}, tapset)
    _check(pkg, m, 128, 2, 0xFF, 0, tapset=tapset)
    if tapset == 0:
        _sweep("128 hi+lo weights everywhere, full sweep", m, 128)
        _stale("128 hi+lo weights everywhere", pkg, m, 128)
    _subset_run(f"128 hi+lo weights everywhere, tap set {tapset}, subset", m, 128, tapset, record="hi+lo weights everywhere")
    assert m.arithmetic(128)["guard_reruns"] == 0
    m.close()


@pytest.mark.parametrize("tapset", ws.TAPSETS)
def test_128_exact(gpu, tapset):
    pkg = gpu
    m = _ctx(pkg, 128, tapset, flags=pkg.capi.FLAG_EXACT_128)
    assert m.arithmetic(128)["exact"] == 1
    p = ws.plan_lines(pkg, _blob(128, tapset), 128, CHUNK, tier=1)
    assert len(p) == 17 and all("[exact" in l and "exact-lite" not in l for l in p[:16]), p
    if tapset == 0:
        _sweep("128 exact, full sweep", m, 128)
        _stale("128 exact", pkg, m, 128)
    _subset_run(f"128 exact, tap set {tapset}, subset", m, 128, tapset, record="exact")
    m.close()
    if tapset == 0:
        ml = _ctx(pkg, 128, low=True, flags=pkg.capi.FLAG_EXACT_128)
        _subset_run("128 exact, stem x 1024", ml, 128, amps=(1,), low=True)
        ml.close()


def test_128_exact_lite(gpu):
    pkg = gpu
    F = pkg.capi
    m = _ctx(pkg, 128, flags=F.FLAG_EXACT_128 | F.FLAG_EXACT_LITE)
    assert m.arithmetic(128)["exact"] in (1, 5), m.arithmetic(128)
    p = ws.plan_lines(pkg, _blob(128), 128, CHUNK, tier=5)
    assert len(p) == 17 and all("[exact-lite" in l for l in p[1:16]), p
    _sweep("128 exact-lite, full sweep", m, 128)
    _subset_run("128 exact-lite, subset", m, 128, record="exact-lite")
    m.close()
    ml = _ctx(pkg, 128, low=True, flags=F.FLAG_EXACT_128 | F.FLAG_EXACT_LITE)
    _subset_run("128 exact-lite, stem x 1024", ml, 128, amps=(1,), low=True)
    ml.close()


# ---- 128 x 128, mixed -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env,w2_units,x_units,full", ws.MIXED_128, ids=[c[0].replace(" ", "_") for c in ws.MIXED_128])
def test_128_mixed(gpu, monkeypatch, name, env, w2_units, x_units, full):
    pkg = gpu
    t0 = time.time()
    m = _forced(pkg, monkeypatch, 128, env)
    a = _check(pkg, m, 128, 4 if x_units else 3, w2_units, x_units)
    for n in ws.STALE_N + (1,):
        ws.check_plan_arithmetic(ws.plan_lines(pkg, _blob(128), 128, n, 0, w2_units, x_units), w2_units, x_units)
    t1 = time.time()
    _subset_run(f"128 mixed ({name})", m, 128, record=name)
    _subset_run(f"128 mixed ({name}), calls of 100", m, 128, amps=(512,), step=100)
    if full:
        _sweep(f"128 mixed ({name}), full sweep", m, 128)
    _stale(f"128 mixed ({name})", pkg, m, 128)
    assert m.arithmetic(128)["guard_reruns"] == 0
    m.close()
    print(f"128 mixed ({name}): load {t1 - t0:.1f} s ({a['calib_cus']} calibration CUs), runs {time.time() - t1:.1f} s")


def test_128_stale_plane_batches_are_two_batch_classes(gpu):
    pkg = gpu
    differ = 0
    for name, env, w2, x, _ in ws.MIXED_128:
        a, b = (tuple(l for l in ws.plan_lines(pkg, _blob(128), 128, n, 0, w2, x)) for n in ws.STALE_N)
        differ += a != b
    assert differ >= len(ws.MIXED_128) // 2, differ


# ---- 64 x 64 -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tapset", ws.TAPSETS)
def test_64_fast_small(gpu, tapset):
    pkg = gpu
    F = pkg.capi
    flags = F.FLAG_FAST_SMALL | OFF(F)
    m = _ctx(pkg, 64, tapset, flags=flags)
    _check(pkg, m, 64, 0, 0, 0)
    p = ws.plan_lines(pkg, _blob(64, tapset), 64, CHUNK)
    assert all("single pass" in l for l in p if not l.startswith(("heads", "guard_flat_stat"))) and p[0].startswith("stem+block_s2_2to32_h32"), p
    _sweep(f"64 single pass, tap set {tapset}, full sweep", m, 64, tapset)
    _subset_run(f"64 single pass, tap set {tapset}, subset", m, 64, tapset, record="single pass")
    if tapset == 0:
        _subset_run("64 single pass, subset in calls of 100", m, 64, step=100, record="single pass, calls of 100")
        _stale("64 single pass", pkg, m, 64)
    assert m.arithmetic(64)["guard_reruns"] == 0
    m.close()
    if tapset == 0:
        ml = _ctx(pkg, 64, low=True, flags=flags)
        _subset_run("64 single pass, stem x 1024", ml, 64, amps=(1,), low=True)
        ml.close()


@pytest.mark.parametrize("tapset", ws.TAPSETS)
def test_64_exact(gpu, tapset):
    pkg = gpu
    m = _ctx(pkg, 64, tapset, flags=pkg.capi.FLAG_NO_CALIBRATION)
    assert m.arithmetic(64)["exact"] == 1
    p = ws.plan_lines(pkg, _blob(64, tapset), 64, CHUNK, tier=1)
    assert len(p) == 21 and all("[exact" in l for l in p[:20]), p
    _sweep(f"64 exact, tap set {tapset}, full sweep", m, 64, tapset)
    _subset_run(f"64 exact, tap set {tapset}, subset", m, 64, tapset, record="exact")
    if tapset == 0:
        _stale("64 exact", pkg, m, 64)
    m.close()
    if tapset == 0:
        ml = _ctx(pkg, 64, low=True, flags=pkg.capi.FLAG_NO_CALIBRATION)
        _subset_run("64 exact, stem x 1024", ml, 64, amps=(1,), low=True)
        ml.close()


@pytest.mark.parametrize("k", (1, 2))
def test_64_single_pass_prefix(gpu, monkeypatch, k):
    """MLT_SMALL_PREFIX = k: the single pass in stages 0 .. k - 1, exact behind it -- what rho_fast held to 1e-3."""
    pkg = gpu
    m = _forced(pkg, monkeypatch, 64, {"MLT_SMALL_PREFIX": str(k)})
    x_units = 0x3FF & ~((1 << (2 * k)) - 1)
    a = m.arithmetic(64)
    assert (a["exact"], a["w2_units"], a["x_units"]) == (4, 0, x_units) and a["flat_guard"] == 0 and a["decision_guard"] == 0, a
    p = ws.plan_lines(pkg, _blob(64), 64, CHUNK, 0, 0, x_units)
    n_fast = 2 if k == 1 else 6
    assert all("single pass" in l for l in p[:n_fast]) and all("[exact" in l for l in p[n_fast:-1]) and p[-1].startswith("heads") and len(p) == n_fast + 4 * (5 - k) + 1, p
    _sweep(f"64 single-pass prefix of {k}, full sweep", m, 64)
    _subset_run(f"64 single-pass prefix of {k}, subset", m, 64, record=f"single-pass prefix of {k}")
    _stale(f"64 single-pass prefix of {k}", pkg, m, 64)
    assert m.arithmetic(64)["guard_reruns"] == 0
    m.close()


# ---- across configurations --------------------------------------------------------------------------------------------------------------------------------------------
def test_zz_configurations_agree(gpu):
    """Every pair of configurations of a size was compared on the subset as it was recorded (_subset_run: 2 x rho_shift); here: that all of them were, and the
    largest difference met."""
    want128 = {"single pass", "single pass, calls of 100", "single pass, calls of 16", "single pass, masked padding", "single pass, masked padding, calls of 100",
               "hi+lo weights everywhere", "exact", "exact-lite"} | {c[0] for c in ws.MIXED_128}
    want64 = {"single pass", "single pass, calls of 100", "exact", "single-pass prefix of 1", "single-pass prefix of 2"}
    assert set(_SUBSET.get((128, 0), {})) == want128 and set(_SUBSET.get((64, 0), {})) == want64, "run the whole module: every configuration records its subset"
    for ts in ws.TAPSETS[1:]:
        assert set(_SUBSET[(128, ts)]) == {"single pass", "hi+lo weights everywhere", "exact"} and set(_SUBSET[(64, ts)]) == {"single pass", "exact"}
    for key in sorted(_SUBSET):
        rho = ws.RHO_SHIFT[key[0]]
        same = all(np.array_equal(v.view(np.uint32), next(iter(_SUBSET[key].values())).view(np.uint32)) for v in _SUBSET[key].values())
        print(f"size {key[0]} tap set {key[1]}: {len(_SUBSET[key])} configurations, largest pairwise difference {_SPREAD[key]:.3e} relative = {_SPREAD[key] / rho:.2f} x rho_shift"
              f"{' (every configuration returns the same bytes)' if same else ''}")
        assert _SPREAD[key] <= 2 * rho
