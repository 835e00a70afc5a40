"""CPU: the tracer weights (tests/tracer_weights.py) -- their reference against the C oracle, the conditions under which the GPU test's relative metric means
something, the tolerance from the fp16 emulation, and the power of that tolerance against eight single-pixel mutations.  tests/test_tracer_gpu.py holds the
device to what is established here; nothing in this file or in the tolerance comes from a device run.

Agreement with the C oracle (fp32, sequential accumulation).  Bound: every conv output is a sum of at most 2304 positive products rounded to nearest in fp32;
in the random-walk model its own relative error is 2^-24 sqrt(2304) = 2.9e-6, and the errors of the 21 layers in front of the last head add at most
linearly: ORACLE_BOUND = 6e-5.  Measured on 36 impulse and 8 dense CUs per size: 128: 1.03e-6, 64: 7.2e-7, 32: 7.5e-7, 16: 6.8e-7 (tw.ORACLE_MEASURED holds 1.5e-6 for
all four; RHO_EXACT is not allowed below 8 x that).

Conditions, per size (test_conditions):
  - G > 0 everywhere, so every response of the sweep is > 0 and the relative metric is defined for every CU and logit; the sweep lists every (plane, pixel) once
  - every float64 activation < 2^14: the weights are positive, so the all-ones input bounds every content of the base weight set (128: 1304, 64: 1451,
    32: 245, 16: 43); the amplitude family runs the set with the stem 2^10 larger and is bounded by its own largest member (both planes at 700: 771 / 717 / 474 / 377)
  - the first-order underflow term (tw.underflow_terms) is at most 1 % of the smallest expected logit of each CU.  This is what the second weight set is for:
    with the base gains an impulse of 37 at size 128 is at 3.4 % and an impulse of 1 at 130 % (16 x 16: 0.55 % and 26 %); with the stem 2^10 larger they are at
    3.3e-5 and 2.1e-3 (64 x 64: 4.4e-5 and 3.1e-3, the largest; the amplitude-1023 sweep on the base set: 2.1e-3 and 3.1e-3).  Checked on every CU of the surroundings and dense families and on a seeded sample (four corners, 16 border and 32
    interior positions per plane; the corners have the smallest responses) of the impulse families -- the activations of all 2 S^2 impulse CUs in float64 would
    take minutes.

Tolerance (test_tolerance): tw.RHO_FAST / tw.RHO_EXACT are recomputed from the emulation and must be the committed tables to within 5 % (float64 summation
order may differ between CPUs and flip single fp16 roundings); RHO_FAST stays below a quarter of the worst case 3 L 2^-11.

Power (test_power): each of the eight mutations moves some impulse response of the sweep by more than 2 x RHO_FAST in some head."""
import time

import numpy as np
import pytest

import tracer_weights as tw

SIZES = (128, 64, 32, 16)
ORACLE_BOUND = 6e-5
_CACHE = {}


def tracer(size, low=False):
    """(state dict, G) of a size, computed once."""
    key = (size, low)
    if key not in _CACHE:
        sd = tw.tracer_state_dict(tw.arch_of(size), gains=tw.GAINS_LOW if low else tw.GAINS)
        _CACHE[key] = (sd, tw.adjoint(sd, size))
    return _CACHE[key]


@pytest.mark.parametrize("arch", (0, 1))
def test_blob_packs_and_round_trips(pkg, arch):
    for gains in (tw.GAINS, tw.GAINS_LOW):
        sd = tw.tracer_state_dict(arch, gains=gains)
        blob = tw.tracer_blob(arch, gains=gains)
        a, back = pkg.weights.unpack_blob(blob)
        assert a == arch
        for k, v in back.items():
            assert np.array_equal(v, sd[k]), k
            if v.ndim == 4 or k.startswith("branch") and k.endswith(".weight"):
                assert (v >= 0).all() and np.isfinite(v).all()
            if v.ndim == 4:
                # every folded conv weight is a normal fp16 number: the fast arithmetic packs them in fp16
                assert v.min() > 2.0 ** -14 and v.max() < 2.0 ** 14, (k, v.min(), v.max())
    assert np.array_equal(tw.tracer_state_dict(arch, gains=tw.GAINS_LOW)["conv1.weight"], tw.GAINS_LOW["stem"] * tw.tracer_state_dict(arch)["conv1.weight"])


@pytest.mark.parametrize("size", SIZES)
def test_stem_gain_scales_the_adjoint_exactly(size):
    assert np.array_equal(tracer(size, True)[1], tw.GAINS_LOW["stem"] * tracer(size)[1])


@pytest.mark.parametrize("size", SIZES)
def test_expected_agrees_with_the_c_oracle(pkg, size):
    from oracle import Oracle
    sd, G = tracer(size)
    orc = Oracle(tw.tracer_blob(tw.arch_of(size)))
    pos = tw.sample_positions(size, 6, 8)            # 4 corners + 6 border + 8 interior = 18 positions x 2 planes
    cases = [tw.impulses(size, plane, pos) for plane in (0, 1)]
    cases.append(pkg.synth.make_patches_bulk(size, 8, 31))
    org, pred = (np.concatenate([c[i] for c in cases]) for i in (0, 1))
    n = len(org)
    assert n >= 32 + 8
    want = tw.expected(G, org, pred)
    assert np.array_equal(want[:2 * len(pos)], np.concatenate([tw.expected_impulse(G, plane, pos) for plane in (0, 1)]))   # gather == dot product on impulses
    got, _ = orc.forward(org, pred, np.zeros(n, np.int32), np.zeros(n, np.int32), threads=8)
    rel = np.abs(got.astype(np.float64) - want) / want
    print(f"size {size}: expected vs C oracle, {n} CUs: max relative {rel.max():.2e} (impulses {rel[:2 * len(pos)].max():.2e}, dense {rel[2 * len(pos):].max():.2e})")
    assert rel.max() <= ORACLE_BOUND
    assert rel.max() <= tw.ORACLE_MEASURED[size], "tw.ORACLE_MEASURED (the floor under RHO_EXACT) is no longer what is measured"
    # poc / qp columns are zero: the scalars must not move a logit
    got2, _ = orc.forward(org[:4], pred[:4], np.full(4, 600, np.int32), np.full(4, 47, np.int32))
    assert np.array_equal(got2, got[:4])


@pytest.mark.parametrize("size", SIZES)
def test_conditions(pkg, size):
    sd, G = tracer(size)
    sdl, Gl = tracer(size, True)
    S2 = size * size
    # responses, and nothing left out
    assert (G > 0).all() and np.isfinite(G).all()
    plane, pos = tw.sweep(size)
    assert len(pos) == 2 * S2 == {128: 32768, 64: 8192, 32: 2048, 16: 512}[size]
    assert np.array_equal(np.sort(plane * S2 + pos), np.arange(2 * S2))
    assert not np.array_equal(plane * S2 + pos, np.arange(2 * S2))             # shuffled
    assert (tw.expected_impulse(G, plane, pos) > 0).all()
    sub = tw.subset_positions(size)
    assert len(sub) == min(512, S2) and len(np.unique(sub)) == len(sub)
    # activations below 2^14
    ones = np.ones((1, 2, size, size))
    top = tw.activation_report(sd, ones)
    assert top < 2.0 ** 14, top
    sample = tw.sample_positions(size, 16, 32)
    top_low = tw.activation_report(sdl, tw.preprocess(*tw.impulses(size, 2, sample, 700)))
    assert top_low < 2.0 ** 14, top_low
    # underflow: base weight set
    worst = {}
    labels, ro, rp = tw.ring_families(size)
    bo, bp = pkg.synth.make_patches_bulk(size, 32, 32)
    lo, lp, zero = tw.leakage_family(size)
    fams = [("impulse %d plane %d" % (tw.AMPLITUDE, p), sd, G) + tw.impulses(size, p, sample) for p in (0, 1)]
    fams += [("surroundings", sd, G, ro, rp), ("dense", sd, G, bo[:8], bp[:8]), ("leakage (bright CU)", sd, G, lo[~zero][:1], lp[~zero][:1])]
    fams += [("impulse %d plane %d, stem x 1024" % (a, p), sdl, Gl) + tw.impulses(size, p, sample, a) for a in (1, 37, 700) for p in (0, 1, 2)]
    for name, s_, g_, o, p in fams:
        x = tw.preprocess(o, p)
        want = tw.expected(g_, o, p)
        assert (want > 0).all(), name
        frac = (tw.underflow_terms(s_, size, x) / want.min(axis=1, keepdims=True)).max()
        worst[name] = frac
        assert frac <= 0.01, (name, frac)
    assert int(zero.sum()) == 42 and zero[0] and zero[-1] and (tw.expected(G, lo[zero], lp[zero]) == 0.0).all()
    print(f"size {size}: largest activation {top:.4g} (all-ones input), {top_low:.4g} (amplitude family); underflow term / smallest expected logit:",
          {k: f"{v:.1e}" for k, v in worst.items()})


@pytest.mark.parametrize("size", SIZES)
def test_tolerance(size):
    sd, _ = tracer(size)
    arch = tw.arch_of(size)
    t0 = time.time()
    err = tw.emulated_errors(sd, size, ("fp16", "hilo"))
    fast, exact = 8 * err["fp16"], np.maximum(8 * err["hilo"], 8 * tw.ORACLE_MEASURED[size])
    print(f"size {size}: rho_fast {[f'{v:.3e}' for v in fast]} rho_exact {[f'{v:.3e}' for v in exact]} (8 x hilo emulation {[f'{8 * v:.3e}' for v in err['hilo']]}) {time.time() - t0:.1f} s")
    for name, got, table in (("RHO_FAST", fast, tw.RHO_FAST), ("RHO_EXACT", exact, tw.RHO_EXACT)):
        want = np.asarray(table[size])
        assert want.shape == got.shape and (np.abs(want - got) <= 0.05 * got).all(), f"tw.{name}[{size}] = {want.tolist()} is not what the emulation gives: {got.tolist()}"
    for h, v in enumerate(tw.RHO_FAST[size]):
        assert v < 0.25 * 3 * tw.n_convs_before_head(arch, h) * 2.0 ** -11, (h, v)
    assert (np.asarray(tw.RHO_EXACT[size]) >= 8 * tw.ORACLE_MEASURED[size]).all()
    assert (np.asarray(tw.RHO_EXACT[size]) < np.asarray(tw.RHO_FAST[size])).all()


@pytest.mark.parametrize("size", SIZES)
def test_power(size):
    sd, G = tracer(size)
    rho_fast = tw.rho(size, exact=False)
    muts = tw.mutations(size)
    assert len(muts) == 8
    missed = []
    for name, mut in muts:
        Gm = tw.adjoint(sd, size, mutation=mut, check=False)
        move = np.abs(Gm - G) / G                                   # [K, 2, S, S]: every position of the sweep
        ratio = (move / (2 * rho_fast)[:, None, None, None])
        k, p, y, x = np.unravel_index(np.argmax(ratio), ratio.shape)
        print(f"size {size}: {name}: largest move {move.max():.2%}; {move[k, p, y, x] / rho_fast[k]:.0f} x rho_fast at logit {k} plane {p} ({y},{x}); "
              f"{int((ratio > 1).any(axis=0).sum())} impulse CUs beyond 2 x rho_fast")
        if not ratio.max() > 1:
            missed.append(name)
    assert not missed, f"mutations the tolerance cannot see: {missed}"
