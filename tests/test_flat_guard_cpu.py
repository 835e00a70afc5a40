"""CPU: the flat-content guard's statistic on the host.  The package's numpy restatement (synth.flat_guard_flags, what the GPU tests take
their expected flags from) against the scalar restatement of csrc/mlt_kernels.h in tests/flat_guard_families.py, on every family CU at all
four sizes and both divisors; the families' own promises (exact counts, covering, a background that counts nothing) are asserted by
their constructors and re-stated here on the results."""
import numpy as np
import pytest

import flat_guard_families as ff
from helpers import SIZES


def test_scalar_reference_on_hand_written_quads():
    """The header's text, case by case (org Pels, pred Pels) -> (near-flat, exactly flat)."""
    q = ff.scalar_quad_bits
    assert q([5, 5, 5, 5], [9, 9, 9, 9]) == (True, True)                       # constant in both planes
    assert q([0, 6, 0, 6], [0, 6, 0, 6]) == (True, False)                      # range exactly 6 (residual 0)
    assert q([0, 7, 0, 7], [0, 7, 0, 7]) == (False, False)                     # range 7, not linear
    assert q([0, 3, 4, 7], [0, 3, 4, 7]) == (False, False)                     # range 7, second differences exactly 2
    assert q([0, 40, 81, 121], [0, 40, 81, 121]) == (True, False)              # second differences +1 / -1 on a steep slope
    assert q([0, 40, 82, 122], [0, 40, 82, 122]) == (False, False)             # ... of 2
    assert q([10, 22, 34, 46], [10, 22, 34, 46]) == (True, True)               # exactly linear
    assert q([500] * 4, [500, 497, 494, 491]) == (True, True)                  # constant org over an exactly linear residual
    assert q([500] * 4, [500, 400, 100, 300]) == (False, False)                # one plane coherent, the other not
    assert q([1023, 1500, 2000, 1024], [1016, 1493, 1993, 1017]) == (True, True)   # org constant after the clip, residual 7 on the unclipped values
    assert q([1023, 1500, 2000, 1024], [1023, 1023, 1023, 1023]) == (False, False)  # ... a residual taken AFTER the clip would be 0 here; it is 0, 477, 977, 1
    assert q([-1, -5, -300, -32768], [0, 0, 0, 0]) == (True, True)             # negative Pels: >= 32768 after the cast, 1023 after the clip, in both planes
    assert q([-1, 0, -1, 0], [-8, -7, -8, -7]) == (False, False)               # 65535 / 0 after the cast: flat only for a signed restatement
    assert q([0, 6, 0, 6], [0, 6, 0, 6], flat_range=5) == (False, False)


def test_the_restatements_use_the_header_range(pkg):
    import inspect
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "fastintercu-vvc_amd", "csrc", "mlt_kernels.h")).read()
    dev = int(re.search(r"^#define MLT_FLAT_RANGE (\d+)", hdr, re.M).group(1))
    par = inspect.signature(pkg.synth.flat_guard_flags).parameters
    assert dev == ff.FLAT_RANGE == par["flat_range"].default == 6 and par["flat_div"].default == 8


def test_numpy_restatement_on_random_pels_of_the_whole_int16_range(pkg):
    """Quads nobody constructed: Pels over all of int16 (casts, clips) and low-amplitude content (many quads near every edge of the rule)."""
    rng = np.random.default_rng(20)
    for lo, hi, base in ((-32768, 32768, 0), (-4, 5, 0), (0, 8, 1018), (-3, 4, 500)):
        org = (base + rng.integers(lo, hi, (3, 16, 16))).astype(np.int16)
        pred = (base + rng.integers(lo, hi, (3, 16, 16))).astype(np.int16)
        near, exact, flagged = pkg.synth.flat_guard_flags(org, pred)
        frac_near, frac_exact = pkg.synth.flat_quad_fraction(org, pred, return_exact=True)
        for i in range(3):
            want = ff.scalar_counts(org[i], pred[i])
            assert (int(near[i]), int(exact[i])) == want, (lo, hi, base, i)
            assert bool(flagged[i]) == ff.scalar_flag(*want, 16, 8)
            assert (frac_near[i] * 64, frac_exact[i] * 64) == want              # flat_quad_fraction is the same statistic as a fraction
        if base:
            assert near.max() > 0


@pytest.mark.parametrize("div", (8, 16))
@pytest.mark.parametrize("size", SIZES)
def test_families_carry_their_counts_and_the_numpy_form_agrees(pkg, size, div):
    """Building the families asserts, per CU and with the scalar reference: the background counts nothing, the CU has exactly its intended
    two counts, the T and the T - 1 CUs of every layout cover every quad position, and synth.flat_guard_flags returns the same integers
    and flags.  Restated here on what comes back: counts on the thresholds, flags as intended, both classes present in every family."""
    fam = ff.family(pkg, size, div)
    q, t, h = ff.thresholds(size, div)
    near, exact, flagged = pkg.synth.flat_guard_flags(fam.org, fam.pred, flat_div=div)
    assert np.array_equal(near, fam.near) and np.array_equal(exact, fam.exact) and np.array_equal(flagged, fam.flagged)
    for f in ("E", "N", "C"):
        for layout in (ff.LAYOUTS if f != "C" else ("perm",)):
            sel = np.array([l.startswith(f"{f}/{layout}/") for l in fam.label])
            if f == "N":
                assert set(near[sel].tolist()) == {h - 1, h} and (exact[sel] == (t - 1) // 2).all() and (t - 1) // 2 < t
            else:
                assert set(exact[sel].tolist()) == {t - 1, t} and np.array_equal(near[sel], exact[sel]) and t < h
            assert flagged[sel].any() and not flagged[sel].all()
            hit = (exact >= t) | (near >= h)
            assert np.array_equal(hit, flagged)
    # E: per layout `div` CUs of T and the covering number of T - 1 CUs (div + 1 wherever (div + 1)(T - 1) >= Q); N: 2 + 3; C: 2 + 2
    per_layout = div + max(div + 1, -(-q // (t - 1))) + 5
    assert len(fam) == 3 * per_layout + 4
    if t > div:
        assert len(fam) == 3 * (2 * div + 6) + 4


def test_default_background_counts_nothing(pkg):
    """The families' background -- 10-bit uniform Pels in both planes -- has no counted quad (64 CUs per size)."""
    for size in SIZES:
        rng = np.random.default_rng([77, size])
        org = rng.integers(0, 1024, (64, size, size)).astype(np.int16)
        pred = rng.integers(0, 1024, (64, size, size)).astype(np.int16)
        near, exact, flagged = pkg.synth.flat_guard_flags(org, pred)
        assert near.sum() == 0 and exact.sum() == 0 and not flagged.any()
    for i in range(4):
        assert ff.scalar_counts(org[i], pred[i]) == (0, 0)


def test_batches_are_reproducible_and_mixed(pkg):
    b1 = ff.batch(pkg, 16, 8, 200)
    b2 = ff.batch(pkg, 16, 8, 200)
    assert np.array_equal(b1.org, b2.org) and np.array_equal(b1.pred, b2.pred) and b1.label == b2.label and len(b1) == 200
    assert 0 < b1.flagged.sum() < 200
    near, exact, flagged = pkg.synth.flat_guard_flags(b1.org, b1.pred)
    assert np.array_equal(flagged, b1.flagged) and np.array_equal(near, b1.near) and np.array_equal(exact, b1.exact)
