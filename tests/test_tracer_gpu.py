"""GPU (MI355X): every pixel position of every convolution path against the float64 adjoint of the tracer weights (tests/tracer_weights.py).

With the tracer weights logit_k = G[k] . (org plane, residual plane) exactly, G from one float64 forward and K backward passes on torch's CPU operators.  A CU
with ONE non-zero pixel therefore has a known answer G[k, plane, y, x] > 0, and a kernel that is wrong at one border column, one ring wrap, one tile seam
or one padded read moves the CUs whose impulse passes through that place by per cents -- in front of the pooling, where no map area divides it away.

Metric: for EVERY CU and EVERY logit |device - expected| / expected, held to tw.RHO_FAST (arithmetics with fp16 activations: the single pass, hi+lo weights,
the small models' prefix tier) or tw.RHO_EXACT (the (hi, lo)-pair arithmetic and every CU a guard re-runs with it) -- both from the CPU emulation of
tests/test_tracer_cpu.py, which also shows that each of eight single-pixel mutations lies beyond 2 x RHO_FAST.  No tolerance here comes from a device run; no
CU and no logit is left out of a comparison; a failure prints the worst (plane, y, x, logit).  Scalars: poc = qp = 0 (their head columns are zero anyway).

Content (tw.*): the full impulse sweep (every pixel, each plane alone, amplitude 1023, batch order shuffled); impulses of 1, 37 and 700 in each plane and in
both at once on a seeded 512-position subset (with the stem 2^10 larger: see GAINS_LOW); non-zero surroundings (the outermost ring, everything but the ring,
full rows and columns, 32 dense texture CUs); leakage (600 all-1023 CUs with 42 zero CUs among them: a zero CU's logits are exactly 0.0).

Which kernels ran is asserted per configuration from arithmetic() and the dispatcher's launch plan.  Times and the device's figures as measured on an MI355X
are in docs/NUMERICS.md ("Tracer weights").  Per test, as pytest reports them there: the first test's set-up 2.2 s (G of size 128, the library check), every
test's call 0.05 .. 1.2 s (the full sweeps of 32768 CUs 0.3 .. 0.6 s each: the planes are zero pages but for one pixel); the whole module about 10 s."""
import ctypes as C
import time

import numpy as np
import pytest

import tracer_weights as tw

pytestmark = pytest.mark.gpu
CHUNK = 4096          # CUs generated and passed per call at most: 2 x 4096 x 128 x 128 int16 = 268 MB of host memory
_REF, _BLOB = {}, {}


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


@pytest.fixture(scope="module")
def ref():
    """ref(size, low=False) -> G[K, 2, S, S] of the base weight set (low: of the set with the stem 2^10 larger), computed once per size."""
    def get(size, low=False):
        if (size, low) not in _REF:
            _REF[(size, low)] = tw.adjoint(tw.tracer_state_dict(tw.arch_of(size), gains=tw.GAINS_LOW if low else tw.GAINS), size)
        return _REF[(size, low)]
    return get


def _blob(size, low=False):
    key = (tw.arch_of(size), low)
    if key not in _BLOB:
        _BLOB[key] = tw.tracer_blob(key[0], gains=tw.GAINS_LOW if low else tw.GAINS)
    return _BLOB[key]


def _ctx(pkg, size, low=False, **kw):
    return pkg.MltCnn(device=0, sizes=(size,), blobs={size: _blob(size, low)}, **kw)


def _plan(pkg, size, n, tier=0, w2_units=0, x_units=0):
    lib = pkg.capi.load_library()
    lib.mlt_plan_describe.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 15)
    blob = _blob(size)
    k = lib.mlt_plan_describe(blob, len(blob), size, n, tier, w2_units, x_units, 1, buf, 1 << 15)
    lines = buf.value.decode().splitlines()
    assert k == len(lines) and k > 0
    return lines


def _names(lines):
    return [l.split(" [")[0] for l in lines]


def _run(m, org, pred, step=CHUNK):
    """Logits of the CUs through mlt_predict_batch, `step` CUs per call, poc = qp = 0."""
    n = len(org)
    z = np.zeros(n, np.int32)
    out = [m.predict_batch(org[i:i + step], pred[i:i + step], z[i:i + step], z[i:i + step])[1] for i in range(0, n, step)]
    return np.concatenate(out)


def _hold(what, size, got, want, exact, describe):
    """Every CU, every logit: |got - want| / want <= rho; prints the per-head worst and, on a failure, the worst CUs."""
    rho = tw.rho(size, exact)
    hk = tw.head_of_logit(tw.arch_of(size))
    assert got.shape == want.shape and got.dtype == np.float32 and (want > 0).all()
    assert np.isfinite(got).all(), f"{what}: non-finite logits"
    rel = np.abs(got.astype(np.float64) - want) / want
    heads = [float(rel[:, hk == h].max()) for h in range(hk.max() + 1)]
    print(f"{what}: {len(got)} CUs, {'rho_exact' if exact else 'rho_fast'}; worst relative error per head {[f'{v:.2e}' for v in heads]} = "
          f"{[f'{v / r:.2f}' for v, r in zip(heads, (tw.RHO_EXACT if exact else tw.RHO_FAST)[size])]} x rho")
    over = rel / rho[None, :]
    if (over > 1).any():
        flat = np.argsort(over, axis=None)[::-1][:16]
        for i, k in zip(*np.unravel_index(flat, over.shape)):
            if over[i, k] > 1:
                print(f"  {what}: CU {i} {describe(int(i))} logit {k}: device {got[i, k]:.9g} expected {want[i, k]:.9g} relative {rel[i, k]:.3e} = {over[i, k]:.2f} x rho")
    bad = (over > 1).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(got)} CUs beyond rho (worst {over.max():.2f} x)"
    return heads


def _sweep(what, m, size, G, exact):
    """The full impulse sweep, generated per chunk.  -> (plane, pos, logits)."""
    plane, pos = tw.sweep(size)
    got = np.concatenate([_run(m, *tw.sweep_chunk(size, plane[i:i + CHUNK], pos[i:i + CHUNK])) for i in range(0, len(pos), CHUNK)])
    assert len(got) == 2 * size * size
    _hold(what, size, got, tw.expected_impulse(G, plane, pos), exact, lambda i: f"plane {plane[i]} ({pos[i] // size},{pos[i] % size})")
    return plane, pos, got


def _subset(size):
    """The 512-position subset, each plane alone, shuffled: (plane, pos)."""
    sub = tw.subset_positions(size)
    order = np.random.default_rng([size, 9]).permutation(2 * len(sub))
    return np.repeat([0, 1], len(sub))[order], np.tile(sub, 2)[order]


def _subset_run(what, m, size, G, exact, step=CHUNK):
    plane, pos = _subset(size)
    got = _run(m, *tw.sweep_chunk(size, plane, pos), step=step)
    _hold(what, size, got, tw.expected_impulse(G, plane, pos), exact, lambda i: f"plane {plane[i]} ({pos[i] // size},{pos[i] % size})")
    return plane, pos, got


def _amplitudes(what, m_low, size, G_low, exact, step=CHUNK):
    sub = tw.subset_positions(size)
    org, pred, want, lab = [], [], [], []
    for amp in (1, 37, 700):
        for plane in (0, 1, 2):
            o, p = tw.impulses(size, plane, sub, amp)
            org.append(o); pred.append(p)
            want.append(tw.expected_impulse(G_low, plane, sub, amp))
            lab += [(amp, plane, int(q)) for q in sub]
    org, pred, want = np.concatenate(org), np.concatenate(pred), np.concatenate(want)
    order = np.random.default_rng([size, 10]).permutation(len(org))
    got = np.concatenate([_run(m_low, org[order[i:i + CHUNK]], pred[order[i:i + CHUNK]], step) for i in range(0, len(order), CHUNK)])
    assert len(got) == 9 * len(sub)
    _hold(what, size, got, want[order], exact, lambda i: "amplitude %d plane %d (both = 2) (%d,%d)" % (lab[order[i]][0], lab[order[i]][1], lab[order[i]][2] // size, lab[order[i]][2] % size))


def _surroundings(what, pkg, m, size, G, exact, reps=1):
    """Ring, all but the ring, rows, columns and 32 dense CUs; reps > 1: the family repeated, to reach the launches of larger batches."""
    labels, ro, rp = tw.ring_families(size)
    bo, bp = pkg.synth.make_patches_bulk(size, 32, 32)
    org, pred = np.concatenate([ro, bo] * reps), np.concatenate([rp, bp] * reps)
    labels = (labels + [f"dense {i}" for i in range(32)]) * reps
    _hold(what, size, _run(m, org, pred), tw.expected(G, org, pred), exact, lambda i: labels[i])
    return len(org)


def _leakage(what, m, size, G, exact, n=600):
    org, pred, zero = tw.leakage_family(size, n)
    got = _run(m, org, pred)
    dirty = np.flatnonzero((got[zero] != 0.0).any(axis=1))
    assert dirty.size == 0, f"{what}: zero CUs at batch indices {np.flatnonzero(zero)[dirty].tolist()} have non-zero logits {got[zero][dirty][:4].tolist()}"
    bright = np.flatnonzero(~zero)
    want = np.repeat(tw.expected(G, org[bright[:1]], pred[bright[:1]]), len(bright), axis=0)
    _hold(what + ", bright CUs", size, got[bright], want, exact, lambda i: f"batch index {bright[i]}")


RAW = lambda F: F.FLAG_NO_CALIBRATION | F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD | F.FLAG_NO_MAGNITUDE_GUARD
FUSED_128 = ["layer0_stream_h64(stem+layer0+layer1.0.conv1+sc)", "layer1_stream_h32(conv2+conv1+conv2)", "stage_128_h16(s2+sc,conv2,conv1,conv2)",
             "stage_256_h8(s2+sc,conv2,conv1,conv2)", "heads"]
TILED_128 = ["stem+block_s2_2to32_h64(layer0.0)", "block_s1_32_h64(conv1+conv2)", "conv3x3_s2_32to64_h32+sc", "chain3_s1_64_h32(conv2+conv1+conv2)",
             "stage_128_h16(s2+sc,conv2,conv1,conv2)", "conv3x3_s2_128to256_h8+sc"]


# ---- 128 x 128, the raw fast kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fast128(gpu, ref):
    """The single pass without calibration and without any guard: impulse CUs are almost entirely flat, the flat guard would keep the fast kernels from ever
    seeing them.  Holds the context and, once computed, the full sweep's logits (the byte reference of the small-batch runs)."""
    pkg = gpu
    m = _ctx(pkg, 128, flags=RAW(pkg.capi))
    a = m.arithmetic(128)
    assert a["exact"] == 0 and a["calibrated"] == 0 and a["flat_guard"] == 0 and a["decision_guard"] == 0 and a["mag_guard_kind"] == 0 and a["w2_units"] == 0 and a["x_units"] == 0, a
    state = {"m": m, "G": ref(128)}
    yield state
    assert m.arithmetic(128)["guard_reruns"] == 0
    m.close()


def _fast_sweep(state):
    if "sweep" not in state:
        state["sweep"] = _sweep("128 raw fast, full sweep (streaming kernels, whole-stage chains)", state["m"], 128, state["G"], False)
    return state["sweep"]


def test_128_raw_fast_full_sweep(gpu, fast128):
    """32768 CUs in 8 calls of 4096: layer0_stream_kernel (ring of rows per persistent workgroup), layer1_stream_kernel, the whole-stage chain kernels."""
    p = _plan(gpu, 128, CHUNK)
    assert _names(p) == FUSED_128 and all("single pass" in l for l in p[1:4]), p
    t0 = time.time()
    _fast_sweep(fast128)
    print(f"128 raw fast full sweep: {time.time() - t0:.1f} s")


def test_128_raw_fast_sweep_tells_every_mutation_from_the_network(fast128):
    """The check can fail: against the adjoint of a network with ONE output pixel of ONE layer scaled by 8/9 (tw.mutations), the device's own sweep is beyond
    rho_fast at some CU, for each of the eight mutations -- the device's error and the tolerance together leave room to see them."""
    plane, pos, got = _fast_sweep(fast128)
    rho = tw.rho(128, exact=False)
    sd = tw.tracer_state_dict(0)
    for name, mut in tw.mutations(128):
        want = tw.expected_impulse(tw.adjoint(sd, 128, mutation=mut, check=False), plane, pos)
        over = np.abs(got.astype(np.float64) - want) / want / rho[None, :]
        print(f"mutation {name}: {int((over > 1).any(axis=1).sum())} CUs of the device's sweep beyond rho_fast (worst {over.max():.1f} x)")
        assert over.max() > 1, name


@pytest.mark.parametrize("n", (100, 16, 1))
def test_128_raw_fast_small_batches_same_bytes_as_the_sweep(gpu, fast128, n):
    """The 512-position subset (1024 CUs) in calls of n CUs: stem_block_kernel + the chain kernels (100), the latency variants (16) and the single-CU path (1).
    Held to rho_fast, and every CU's logits are the bytes of the same CU in the full sweep."""
    p = _plan(gpu, 128, n)
    if n == 100:
        assert _names(p)[:6] == TILED_128 and all("latency tiles" in l for l in p[5:9]) and all("single pass" in l for l in p[:9]), p
    else:
        assert len(p) == 15 and _names(p)[:3] == TILED_128[:3] and all("latency tiles" in l for l in p[3:14]) and _names(p)[-1] == "heads", p
    plane, pos, full = _fast_sweep(fast128)
    t0 = time.time()
    sp, spos, got = _subset_run(f"128 raw fast, subset in calls of {n}", fast128["m"], 128, fast128["G"], False, step=n)
    where = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(plane, pos))}
    idx = np.array([where[(int(a), int(b))] for a, b in zip(sp, spos)])
    diff = np.flatnonzero((got.view(np.uint32) != full[idx].view(np.uint32)).any(axis=1))
    for i in diff[:8]:
        print(f"  plane {sp[i]} ({spos[i] // 128},{spos[i] % 128}): n = {n}: {got[i].tolist()} sweep: {full[idx[i]].tolist()}")
    assert diff.size == 0, f"{diff.size} of {len(got)} CUs differ in their bytes between calls of {n} and the full sweep"
    print(f"128 raw fast subset in calls of {n}: {time.time() - t0:.1f} s")


def test_128_raw_fast_masked_padding(gpu, fast128, monkeypatch):
    """MLT_TUNING=1 MLT_NO_LDS_OOB=1: the chain kernels with zero masks in place of the reads beyond the LDS allocation; large and small launches."""
    pkg = gpu
    monkeypatch.setenv("MLT_TUNING", "1")
    monkeypatch.setenv("MLT_NO_LDS_OOB", "1")
    m = _ctx(pkg, 128, flags=RAW(pkg.capi))
    monkeypatch.delenv("MLT_NO_LDS_OOB")
    monkeypatch.delenv("MLT_TUNING")
    assert m.arithmetic(128)["exact"] == 0
    _subset_run("128 raw fast, masked padding, subset in one call", m, 128, fast128["G"], False)
    _, _, got = _subset_run("128 raw fast, masked padding, subset in calls of 100", m, 128, fast128["G"], False, step=100)
    _leakage("128 raw fast, masked padding, leakage", m, 128, fast128["G"], False)
    m.close()


def test_128_raw_fast_amplitudes(gpu, ref):
    pkg = gpu
    m = _ctx(pkg, 128, low=True, flags=RAW(pkg.capi))
    assert m.arithmetic(128)["exact"] == 0
    _amplitudes("128 raw fast, amplitudes 1 / 37 / 700", m, 128, ref(128, True), False)
    _amplitudes("128 raw fast, amplitudes 1 / 37 / 700 in calls of 100", m, 128, ref(128, True), False, step=100)
    m.close()


def test_128_raw_fast_surroundings_and_leakage(gpu, fast128):
    """Ring / rows / columns / dense: 106 CUs in one call (tiled kernels) and three times over in one call (318: streaming kernels).  Leakage: 600 CUs in one call --
    the streaming launches' 256 persistent workgroups run two or three CUs each on the same LDS rings -- and the first 100 of them (chain kernels)."""
    m, G = fast128["m"], fast128["G"]
    n = _surroundings("128 raw fast, surroundings", gpu, m, 128, G, False)
    assert n < 128 and _names(_plan(gpu, 128, n))[:5] == TILED_128[:5]
    assert 3 * n >= 128 and _names(_plan(gpu, 128, 3 * n)) == FUSED_128
    _surroundings("128 raw fast, surroundings x 3", gpu, m, 128, G, False, reps=3)
    _leakage("128 raw fast, leakage", m, 128, G, False)
    _leakage("128 raw fast, leakage, 100 CUs", m, 128, G, False, n=100)


# ---- 128 x 128, the other arithmetics ------------------------------------------------------------------------------------------------------------------------
def test_128_hi_lo_weights(gpu, ref, monkeypatch):
    """MLT_TUNING=1 MLT_W2_MASK=15: hi+lo weights in every stage (tiled two-plane kernels at every batch size), fp16 activations: held to rho_fast; its measured error
    is printed next to the single pass's (docs/NUMERICS.md)."""
    pkg = gpu
    F = pkg.capi
    monkeypatch.setenv("MLT_TUNING", "1")
    monkeypatch.setenv("MLT_W2_MASK", "15")
    m = _ctx(pkg, 128, flags=F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD | F.FLAG_NO_MAGNITUDE_GUARD)
    monkeypatch.delenv("MLT_W2_MASK")
    monkeypatch.delenv("MLT_TUNING")
    a = m.arithmetic(128)
    assert a["exact"] == 2 and a["w2_units"] == 0xFF and a["x_units"] == 0 and a["flat_guard"] == 0 and a["decision_guard"] == 0 and a["mag_guard_kind"] == 0, a
    p = _plan(pkg, 128, CHUNK, 0, a["w2_units"], a["x_units"])
    assert len(p) == 9 and all("hi+lo weights" in l for l in p[:8]) and _names(p)[0] == TILED_128[0], p
    t0 = time.time()
    _sweep("128 hi+lo weights, full sweep", m, 128, ref(128), False)
    _leakage("128 hi+lo weights, leakage", m, 128, ref(128), False)
    assert m.arithmetic(128)["guard_reruns"] == 0
    m.close()
    print(f"128 hi+lo weights: {time.time() - t0:.1f} s")


@pytest.fixture(scope="module")
def exact128(gpu, ref):
    pkg = gpu
    m = _ctx(pkg, 128, flags=pkg.capi.FLAG_EXACT_128)
    a = m.arithmetic(128)
    assert a["exact"] == 1, a
    p = _plan(pkg, 128, CHUNK, tier=1)
    assert len(p) == 17 and all("[exact" in l and "exact-lite" not in l for l in p[:16]), p
    state = {"m": m}
    yield state
    m.close()


def test_128_exact(gpu, ref, exact128):
    t0 = time.time()
    m = exact128["m"]
    exact128["sweep"] = _sweep("128 exact, full sweep", m, 128, ref(128), True)[2]
    _surroundings("128 exact, surroundings", gpu, m, 128, ref(128), True)
    _leakage("128 exact, leakage", m, 128, ref(128), True)
    print(f"128 exact: {time.time() - t0:.1f} s")


def test_128_exact_amplitudes(gpu, ref):
    m = _ctx(gpu, 128, low=True, flags=gpu.capi.FLAG_EXACT_128)
    assert m.arithmetic(128)["exact"] == 1
    _amplitudes("128 exact, amplitudes 1 / 37 / 700", m, 128, ref(128, True), True)
    m.close()


def test_128_exact_lite(gpu, ref, exact128):
    """MLT_FLAG_EXACT_128 | MLT_FLAG_EXACT_LITE: both cross terms in one scaled FP8 MFMA; held to rho_fast, its measured error recorded (docs/NUMERICS.md)."""
    pkg = gpu
    F = pkg.capi
    m = _ctx(pkg, 128, flags=F.FLAG_EXACT_128 | F.FLAG_EXACT_LITE)
    assert m.arithmetic(128)["exact"] in (1, 5), m.arithmetic(128)
    p = _plan(pkg, 128, CHUNK, tier=5)
    assert len(p) == 17 and all("[exact-lite" in l for l in p[1:16]), p
    t0 = time.time()
    got = _sweep("128 exact-lite, full sweep", m, 128, ref(128), False)[2]
    _leakage("128 exact-lite, leakage", m, 128, ref(128), False)
    if "sweep" in exact128:   # another arithmetic than the exact one did run: the bytes differ
        assert not np.array_equal(got, exact128["sweep"])
    m.close()
    print(f"128 exact-lite: {time.time() - t0:.1f} s")


def test_128_default_flags(gpu, ref):
    """flags = 0, the shipped configuration.  The load-time calibration holds the tiers to |dlogit| <= 1e-3 ABSOLUTE on logits that reach hundreds with these weights:
    no fp16 tier is admitted (on the MI355X it ends on the exact-lite tier, `exact` = 5), and whatever non-exact tier it keeps runs behind the flat-content guard.  An
    impulse CU is flat almost everywhere: EVERY CU of the subset is counted in guard_reruns and meets rho_exact."""
    pkg = gpu
    G = ref(128)
    m = _ctx(pkg, 128)
    a = m.arithmetic(128)
    print("128 default flags:", a)
    assert a["calibrated"] == 1 and a["exact"] != 1 and a["flat_guard"] == 1 and a["decision_guard"] == 1, a
    plane, pos = _subset(128)
    r0 = a["guard_reruns"]
    _subset_run("128 default flags, subset", m, 128, G, True)
    assert m.arithmetic(128)["guard_reruns"] - r0 == len(pos) == 1024
    _subset_run("128 default flags, subset in calls of 100", m, 128, G, True, step=100)
    assert m.arithmetic(128)["guard_reruns"] - r0 == 2 * len(pos)
    _leakage("128 default flags, leakage", m, 128, G, True)
    assert m.arithmetic(128)["guard_reruns"] - r0 == 2 * len(pos) + 600       # zero CUs and all-1023 CUs are flat as well
    m.close()


# ---- 64 / 32 / 16 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (64, 32, 16))
def test_small_default(gpu, ref, size):
    """flags = 0: the exact arithmetic (32, 16; 64: whatever the calibration keeps, behind the guards -- every impulse CU is flat and re-run exactly)."""
    pkg = gpu
    t0 = time.time()
    m = _ctx(pkg, size)
    a = m.arithmetic(size)
    print(f"{size} default flags:", a)
    if size != 64:
        assert a["exact"] == 1, a
        p = _plan(pkg, size, CHUNK, tier=1)
        assert len(p) == 21 and all("[exact" in l for l in p[:20]), p
    else:
        assert a["exact"] == 1 or (a["flat_guard"] == 1 and a["decision_guard"] == 1), a
    G = ref(size)
    r0 = a["guard_reruns"]
    _sweep(f"{size} default flags, full sweep", m, size, G, True)
    if a["exact"] != 1:
        assert m.arithmetic(size)["guard_reruns"] - r0 == 2 * size * size
    _surroundings(f"{size} default flags, surroundings", pkg, m, size, G, True)
    if size == 16:
        _leakage("16 default flags, leakage", m, size, G, True)
    m.close()
    ml = _ctx(pkg, size, low=True, flags=pkg.capi.FLAG_NO_CALIBRATION)
    assert ml.arithmetic(size)["exact"] == 1
    _amplitudes(f"{size} exact, amplitudes 1 / 37 / 700", ml, size, ref(size, True), True)
    ml.close()
    print(f"{size} default: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("size", (64, 32, 16))
def test_small_fast(gpu, ref, size):
    """MLT_FLAG_FAST_SMALL without the guards: stem_block_kernel (64) / stem5 + per-conv kernels (32, 16: centre-tap kernels on the 1 x 1 maps)."""
    pkg = gpu
    F = pkg.capi
    t0 = time.time()
    flags = F.FLAG_FAST_SMALL | F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD | F.FLAG_NO_MAGNITUDE_GUARD
    m = _ctx(pkg, size, flags=flags)
    a = m.arithmetic(size)
    assert a["exact"] == 0 and a["flat_guard"] == 0 and a["decision_guard"] == 0 and a["w2_units"] == 0 and a["x_units"] == 0, a
    p = _plan(pkg, size, CHUNK)
    assert all("single pass" in l for l in p if not l.startswith(("heads", "guard_flat_stat"))), p
    assert _names(p)[0] == ("stem+block_s2_2to32_h32(layer0.0)" if size == 64 else "guard_flat_stat"), p
    assert sum("centre tap" in l for l in p) == {64: 0, 32: 3, 16: 7}[size]
    G = ref(size)
    _sweep(f"{size} fast, full sweep", m, size, G, False)
    _subset_run(f"{size} fast, subset in calls of 1", m, size, G, False, step=1) if size == 16 else _subset_run(f"{size} fast, subset in calls of 100", m, size, G, False, step=100)
    _surroundings(f"{size} fast, surroundings", pkg, m, size, G, False)
    if size == 16:
        _leakage("16 fast, leakage", m, size, G, False)
    assert m.arithmetic(size)["guard_reruns"] == 0
    m.close()
    ml = _ctx(pkg, size, low=True, flags=flags)
    _amplitudes(f"{size} fast, amplitudes 1 / 37 / 700", ml, size, ref(size, True), False)
    ml.close()
    print(f"{size} fast: {time.time() - t0:.1f} s")


def test_64_single_pass_prefix(gpu, ref, monkeypatch):
    """MLT_TUNING=1 MLT_SMALL_PREFIX=1: layer0 on the fused single-pass kernels, exact from layer1 on (the 64 x 64 model's calibrated tier on the seeded sets); fp16
    activations in layer0: rho_fast."""
    pkg = gpu
    F = pkg.capi
    monkeypatch.setenv("MLT_TUNING", "1")
    monkeypatch.setenv("MLT_SMALL_PREFIX", "1")
    m = _ctx(pkg, 64, flags=F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD)
    monkeypatch.delenv("MLT_SMALL_PREFIX")
    monkeypatch.delenv("MLT_TUNING")
    a = m.arithmetic(64)
    assert a["exact"] == 4 and a["x_units"] == 0x3FC and a["w2_units"] == 0 and a["flat_guard"] == 0 and a["decision_guard"] == 0, a
    p = _plan(pkg, 64, CHUNK, 0, 0, a["x_units"])
    assert _names(p)[:2] == ["stem+block_s2_2to32_h32(layer0.0)", "block_s1_32_h32(conv1+conv2)"] and all("single pass" in l for l in p[:2]) and all("[exact" in l for l in p[2:18]), p
    _sweep("64 single-pass layer0 + exact rest, full sweep", m, 64, ref(64), False)
    _surroundings("64 single-pass layer0 + exact rest, surroundings", pkg, m, 64, ref(64), False)
    assert m.arithmetic(64)["guard_reruns"] == 0
    m.close()
