"""GPU (MI355X): bias, ReLU and BN folding per pixel against float64, on the gated weights (tests/gated_weights.py; everything relied on here is established on the
CPU by tests/test_gated_cpu.py).

The tracer and the shift weights hold the MFMA sums of every kernel to float64 per pixel, with every epilogue a no-op: no bias, no clipping ReLU, identity BatchNorm.
With the gated weights every site of a map of at least 8 x 8 adds a folded bias (blocks with a projection: conv2's +b and the shortcut's -2 b), has a quarter of
its channels negative in front of the ReLU and clips 20 .. 80 % of an impulse's cone.  A bias dropped at a tile seam, a ReLU applied before the shortcut add at one
position, a stale bias on a padded row move the CUs whose cone passes through that place; a gate that opens on the zero CU moves its logits off exactly 0.0.

Metric: for EVERY CU and EVERY logit |device - forward64| <= rho_k x M, M the logit of the same CU under the tracer network, rho = gw.RHO_GATED_FAST (fp16
activations) or gw.RHO_GATED_EXACT (the (hi, lo)-pair arithmetic and every CU a guard re-runs with it), both from the CPU emulation.  Every zero CU, wherever it
stands in the batch, has logits exactly 0.0; all logits are finite; guard_reruns is 0 where the guards are off.  No tolerance here comes from a device run.

The float64 reference does not depend on the configuration: it is computed once per size (`data`) and shared; its wall time is printed.  Which kernels ran is
asserted per configuration from arithmetic() and the dispatcher's launch plan.  The device's figures are in docs/NUMERICS.md ("Gated weights")."""
import ctypes as C
import time

import numpy as np
import pytest

import gated_weights as gw
import shift_weights as ws
import tracer_weights as tw
from test_tracer_gpu import FUSED_128, RAW, TILED_128, _names

pytestmark = pytest.mark.gpu
_DATA, _BLOB, _ONE_CALL, _WORST = {}, {}, {}, {}


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


def data(size):
    """The content of a size, its float64 reference and M, computed once and never written to."""
    if size not in _DATA:
        t0 = time.time()
        labels, org, pred, is_zero, is_imp = gw.content(size)
        ref = gw.reference(size, org, pred)
        t1 = time.time()
        d = dict(labels=labels, org=org, pred=pred, is_zero=is_zero, is_imp=is_imp, ref=ref, M=gw.magnitude(size, org, pred))
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _DATA[size] = d
        print(f"gated reference, size {size}: {len(org)} CUs ({len(gw.unique_rows(org, pred)[0])} distinct) in float64: {t1 - t0:.1f} s; M (tracer adjoint): {time.time() - t1:.1f} s")
    return _DATA[size]


def _blob(size):
    if size not in _BLOB:
        _BLOB[size] = gw.gated_blob(size)
    return _BLOB[size]


def _ctx(pkg, size, **kw):
    return pkg.MltCnn(device=0, sizes=(size,), blobs={size: _blob(size)}, **kw)


def _plan(pkg, size, n, tier=0, w2_units=0, x_units=0):
    return ws.plan_lines(pkg, _blob(size), size, n, tier, w2_units, x_units)


def _env_ctx(pkg, monkeypatch, size, env, **kw):
    """A context built with tuning switches set around the constructor only."""
    env = dict(env, MLT_TUNING="1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return _ctx(pkg, size, **kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _run(m, org, pred, step=None):
    n = len(org)
    step = n if step is None else step
    z = np.zeros(n, np.int32)
    return np.concatenate([m.predict_batch(org[i:i + step], pred[i:i + step], z[i:i + step], z[i:i + step])[1] for i in range(0, n, step)])


def _hold(what, size, got, exact, idx=None):
    """Every CU of the content (idx: of that part of it), every logit: |got - forward64| <= rho M; zero CUs exactly 0.0.  Prints the per-head worst as a multiple of
    rho and, on a failure, the worst (CU label, logit)."""
    d = data(size)
    idx = np.arange(len(d["ref"])) if idx is None else np.asarray(idx)
    want, M, zero = d["ref"][idx], d["M"][idx], d["is_zero"][idx]
    rho = gw.rho(size, exact)
    hk = tw.head_of_logit(tw.arch_of(size))
    assert got.shape == want.shape and got.dtype == np.float32, (got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite logits"
    dirty = np.flatnonzero((got[zero] != 0.0).any(axis=1))
    assert dirty.size == 0, f"{what}: zero CUs {[d['labels'][i] for i in idx[zero][dirty][:6]]} have non-zero logits {got[zero][dirty][:4].tolist()}"
    over = np.where(M > 0, np.abs(got.astype(np.float64) - want) / np.where(M > 0, rho[None, :] * M, 1.0), 0.0)
    heads = [float(over[:, hk == h].max()) for h in range(hk.max() + 1)]
    _WORST[what] = (size, "rho_exact" if exact else "rho_fast", heads)
    print(f"{what}: {len(got)} CUs ({int(zero.sum())} zero CUs exactly 0.0), {'rho_exact' if exact else 'rho_fast'}; worst |error| / (rho M) per head {[f'{v:.2f}' for v in heads]}")
    if (over > 1).any():
        for i, k in zip(*np.unravel_index(np.argsort(over, axis=None)[::-1][:16], over.shape)):
            if over[i, k] > 1:
                print(f"  {what}: CU {idx[i]} {d['labels'][idx[i]]} logit {k}: device {got[i, k]:.9g} expected {want[i, k]:.9g} M {M[i, k]:.6g}: {over[i, k]:.2f} x rho M")
    bad = (over > 1).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(got)} CUs beyond rho M (worst {over.max():.2f} x)"
    return got


def _whole(what, m, size, exact, step=None):
    d = data(size)
    return _hold(what, size, _run(m, d["org"], d["pred"], step), exact)


def _same_bytes(what, got, full, labels):
    diff = np.flatnonzero((got.view(np.uint32) != full.view(np.uint32)).any(axis=1))
    for i in diff[:8]:
        print(f"  {what}: {labels[i]}: {got[i].tolist()} one call: {full[i].tolist()}")
    assert diff.size == 0, f"{what}: {diff.size} of {len(got)} CUs differ in their bytes from the one-call run"


def _tells_mutations(what, size, got, exact):
    """The device's own results lie beyond rho M of each mutated float64 network at some CU of gw.mutation_cus."""
    d = data(size)
    rho = gw.rho(size, exact)
    t0 = time.time()
    muts = gw.seen_mutations(size)
    assert {m[0] for _, m in muts} == set(gw.KINDS)
    for name, mut in muts:
        idx = gw.mutation_cus(size, mut, d["labels"], d["org"], d["is_zero"], d["is_imp"])
        want = gw.reference(size, d["org"][idx], d["pred"][idx], mutation=mut)
        M = d["M"][idx]
        over = np.where(M > 0, np.abs(got[idx].astype(np.float64) - want) / np.where(M > 0, rho[None, :] * M, 1.0), 0.0)
        print(f"{what}: mutation {name}: {int((over > 1).any(axis=1).sum())} of {len(idx)} CUs beyond rho M (worst {over.max():.1f} x)")
        assert over.max() > 1, name
    print(f"{what}: {len(muts)} mutated float64 networks {time.time() - t0:.1f} s")


# ---- 128 x 128 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fast128(gpu):
    """The raw single pass: no calibration, no guard (an impulse CU is flat: the flat guard would keep the fast kernels from ever seeing it)."""
    pkg = gpu
    m = _ctx(pkg, 128, flags=RAW(pkg.capi))
    a = m.arithmetic(128)
    assert a["exact"] == 0 and a["calibrated"] == 0 and a["flat_guard"] == 0 and a["decision_guard"] == 0 and a["mag_guard_kind"] == 0 and a["w2_units"] == 0 and a["x_units"] == 0, a
    state = {"m": m}
    yield state
    assert m.arithmetic(128)["guard_reruns"] == 0
    m.close()


def _one_call_128(gpu, state):
    if 128 not in _ONE_CALL:
        n = len(data(128)["org"])
        p = _plan(gpu, 128, n)
        assert n >= 128 and _names(p) == FUSED_128 and all("single pass" in l for l in p[1:4]), p
        _ONE_CALL[128] = _whole("128 raw single pass, one call (streaming kernels, whole-stage chains)", state["m"], 128, False)
    return _ONE_CALL[128]


def test_128_raw_single_pass_one_call(gpu, fast128):
    _one_call_128(gpu, fast128)


def test_128_tells_every_mutation_from_the_network(gpu, fast128):
    _tells_mutations("128 raw single pass", 128, _one_call_128(gpu, fast128), False)


@pytest.mark.parametrize("n", (100, 16, 1))
def test_128_raw_single_pass_small_calls_same_bytes(gpu, fast128, n):
    """Calls of 100 (stem_block_kernel + the chain kernels), of 16 (latency tiles) and of 1 (a 64-CU subset): rho_fast, and every CU's logits are the bytes of the
    one-call run."""
    p = _plan(gpu, 128, n)
    if n == 100:
        assert _names(p)[:6] == TILED_128 and all("latency tiles" in l for l in p[5:9]) and all("single pass" in l for l in p[:9]), p
    else:
        assert len(p) == 15 and _names(p)[:3] == TILED_128[:3] and all("latency tiles" in l for l in p[3:14]) and _names(p)[-1] == "heads", p
    d = data(128)
    full = _one_call_128(gpu, fast128)
    idx = np.arange(len(full))
    if n == 1:
        idx = np.sort(np.concatenate([[0, len(full) - 1], np.random.default_rng([128, 11]).permutation(np.arange(1, len(full) - 1))[:62]]))
    got = _hold(f"128 raw single pass, calls of {n}", 128, _run(fast128["m"], d["org"][idx], d["pred"][idx], n), False, idx)
    _same_bytes(f"calls of {n}", got, full[idx], [d["labels"][i] for i in idx])


def test_128_masked_padding(gpu, monkeypatch):
    """MLT_TUNING=1 MLT_NO_LDS_OOB=1: zero masks in place of the reads beyond the LDS allocation; one call and calls of 100."""
    pkg = gpu
    m = _env_ctx(pkg, monkeypatch, 128, {"MLT_NO_LDS_OOB": "1"}, flags=RAW(pkg.capi))
    assert m.arithmetic(128)["exact"] == 0
    _whole("128 masked padding, one call", m, 128, False)
    _whole("128 masked padding, calls of 100", m, 128, False, step=100)
    assert m.arithmetic(128)["guard_reruns"] == 0
    m.close()


def test_128_hi_lo_weights(gpu, monkeypatch):
    pkg = gpu
    F = pkg.capi
    m = _env_ctx(pkg, monkeypatch, 128, {"MLT_W2_MASK": "15"}, flags=F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD | F.FLAG_NO_MAGNITUDE_GUARD)
    a = m.arithmetic(128)
    assert a["exact"] == 2 and a["w2_units"] == 0xFF and a["x_units"] == 0 and a["flat_guard"] == 0 and a["decision_guard"] == 0 and a["mag_guard_kind"] == 0, a
    p = _plan(pkg, 128, len(data(128)["org"]), 0, a["w2_units"], a["x_units"])
    assert len(p) == 9 and all("hi+lo weights" in l for l in p[:8]) and _names(p)[0] == TILED_128[0], p
    _whole("128 hi+lo weights everywhere", m, 128, False)
    assert m.arithmetic(128)["guard_reruns"] == 0
    m.close()


def test_128_exact(gpu):
    pkg = gpu
    m = _ctx(pkg, 128, flags=pkg.capi.FLAG_EXACT_128)
    assert m.arithmetic(128)["exact"] == 1
    p = _plan(pkg, 128, len(data(128)["org"]), tier=1)
    assert len(p) == 17 and all("[exact" in l and "exact-lite" not in l for l in p[:16]), p
    _whole("128 exact", m, 128, True)
    m.close()


def test_128_exact_lite(gpu):
    pkg = gpu
    F = pkg.capi
    m = _ctx(pkg, 128, flags=F.FLAG_EXACT_128 | F.FLAG_EXACT_LITE)
    assert m.arithmetic(128)["exact"] in (1, 5), m.arithmetic(128)
    p = _plan(pkg, 128, len(data(128)["org"]), tier=5)
    assert len(p) == 17 and all("[exact-lite" in l for l in p[1:16]), p
    _whole("128 exact-lite", m, 128, False)
    m.close()


def test_128_default_flags(gpu):
    """flags = 0.  Whatever tier the calibration keeps runs behind the guards; the zero, impulse and leakage CUs are flat: each is re-run exactly (rho_exact, and
    guard_reruns counts every one).  The ring families and the dense CUs are held to the tier's own tolerance."""
    pkg = gpu
    d = data(128)
    m = _ctx(pkg, 128)
    a = m.arithmetic(128)
    print("128 default flags:", a)
    assert a["calibrated"] == 1 and (a["exact"] == 1 or (a["flat_guard"] == 1 and a["decision_guard"] == 1)), a
    flat = np.array([l.startswith(("zero", "impulse", "leakage")) for l in d["labels"]])
    idx = np.flatnonzero(flat)
    r0 = a["guard_reruns"]
    _hold("128 default flags, flat CUs", 128, _run(m, d["org"][idx], d["pred"][idx]), True, idx)
    if a["exact"] != 1:
        assert m.arithmetic(128)["guard_reruns"] - r0 == len(idx)
    rest = np.flatnonzero(~flat)
    _hold("128 default flags, ring families and dense CUs", 128, _run(m, d["org"][rest], d["pred"][rest]), a["exact"] == 1, rest)
    m.close()


MIXED = [ws.MIXED_128[0], next(c for c in ws.MIXED_128 if c[3] != 0)]


@pytest.mark.parametrize("name,env,w2_units,x_units,full", MIXED, ids=[c[0].replace(" ", "_") for c in MIXED])
def test_128_mixed(gpu, monkeypatch, name, env, w2_units, x_units, full):
    """Two of ws.MIXED_128's forced plans: a fast-to-exact hand-off carries a ReLU'd, biased tensor."""
    pkg = gpu
    F = pkg.capi
    m = _env_ctx(pkg, monkeypatch, 128, dict(env, MLT_ROUNDING="0"), flags=F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD | F.FLAG_NO_MAGNITUDE_GUARD,
                 tolerance=1e-30 if ws.needs_tolerance(env) else 0.0)
    a = m.arithmetic(128)
    assert (a["exact"], a["w2_units"], a["x_units"]) == (4 if x_units else 3, w2_units, x_units), (a, hex(w2_units), hex(x_units))
    assert a["flat_guard"] == 0 and a["decision_guard"] == 0 and a["mag_guard_kind"] == 0, a
    for n in (len(data(128)["org"]), 100):
        ws.check_plan_arithmetic(_plan(pkg, 128, n, 0, w2_units, x_units), w2_units, x_units)
    _whole(f"128 mixed ({name})", m, 128, False)
    _whole(f"128 mixed ({name}), calls of 100", m, 128, False, step=100)
    assert m.arithmetic(128)["guard_reruns"] == 0
    m.close()


# ---- 64 / 32 / 16 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (64, 32, 16))
def test_small_default(gpu, size):
    """flags = 0: the exact arithmetic (32, 16; 64: whatever the calibration keeps, behind the guards)."""
    pkg = gpu
    m = _ctx(pkg, size)
    a = m.arithmetic(size)
    print(f"{size} default flags:", a)
    if size != 64:
        assert a["exact"] == 1, a
        p = _plan(pkg, size, len(data(size)["org"]), tier=1)
        assert len(p) == 21 and all("[exact" in l for l in p[:20]), p
    else:
        assert a["exact"] == 1 or (a["flat_guard"] == 1 and a["decision_guard"] == 1), a
    _whole(f"{size} default flags", m, size, True)
    m.close()


@pytest.mark.parametrize("size", (64, 32, 16))
def test_small_fast(gpu, size):
    """MLT_FLAG_FAST_SMALL without the guards."""
    pkg = gpu
    F = pkg.capi
    m = _ctx(pkg, size, flags=F.FLAG_FAST_SMALL | F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD | F.FLAG_NO_MAGNITUDE_GUARD)
    a = m.arithmetic(size)
    assert a["exact"] == 0 and a["flat_guard"] == 0 and a["decision_guard"] == 0 and a["w2_units"] == 0 and a["x_units"] == 0, a
    p = _plan(pkg, size, len(data(size)["org"]))
    assert all("single pass" in l for l in p if not l.startswith(("heads", "guard_flat_stat"))), p
    assert _names(p)[0] == ("stem+block_s2_2to32_h32(layer0.0)" if size == 64 else "guard_flat_stat"), p
    _ONE_CALL[size] = _whole(f"{size} fast", m, size, False)
    _whole(f"{size} fast, calls of 100", m, size, False, step=100)
    assert m.arithmetic(size)["guard_reruns"] == 0
    m.close()


@pytest.mark.parametrize("size", (64, 32, 16))
def test_small_tells_every_mutation_from_the_network(gpu, size):
    assert size in _ONE_CALL, "run the whole module: test_small_fast leaves the device's one-call results"
    _tells_mutations(f"{size} fast", size, _ONE_CALL[size], False)


def test_64_single_pass_prefix(gpu, monkeypatch):
    """MLT_TUNING=1 MLT_SMALL_PREFIX=1: layer0 on the fused single-pass kernels, exact from layer1 on: the hand-off carries a gated tensor."""
    pkg = gpu
    F = pkg.capi
    m = _env_ctx(pkg, monkeypatch, 64, {"MLT_SMALL_PREFIX": "1"}, flags=F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD)
    a = m.arithmetic(64)
    assert a["exact"] == 4 and a["x_units"] == 0x3FC and a["w2_units"] == 0 and a["flat_guard"] == 0 and a["decision_guard"] == 0, a
    p = _plan(pkg, 64, len(data(64)["org"]), 0, 0, a["x_units"])
    assert _names(p)[:2] == ["stem+block_s2_2to32_h32(layer0.0)", "block_s1_32_h32(conv1+conv2)"] and all("single pass" in l for l in p[:2]) and all("[exact" in l for l in p[2:18]), p
    _whole("64 single-pass layer0 + exact rest", m, 64, False)
    assert m.arithmetic(64)["guard_reruns"] == 0
    m.close()


def test_zz_report(gpu):
    """The device's worst |error| / (rho M) per head and configuration (docs/NUMERICS.md, "Gated weights")."""
    for what, (size, table, heads) in _WORST.items():
        print(f"| {what} | {table} | {' '.join(f'{v:.2f}' for v in heads)} |")
    assert _WORST
