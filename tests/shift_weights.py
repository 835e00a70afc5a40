"""Shift weights: a weight family for which NO arithmetic tier rounds, beside the tracer weights (tests/tracer_weights.py), whose network (Net64), preprocessing,
impulse families and adjoint it reuses.

The tracer weights hold a kernel to rho_fast ~ 1e-3 relative whatever it mixes: an impulse's error is made at the first fp16 rounding sites.  Here every
activation of an impulse CU is a short sum of equal powers of two, so rounding to fp16 is the identity at every site: the single pass, hi+lo weights, the exact
and the exact-lite arithmetic and every mixture of them land on the same float64 value to ~1e-7, and the tolerance is RHO_SHIFT ~ 1e-6.

  shift_state_dict(size, tapset)
      BatchNorm   weight 1, bias 0, mean 0, running_var = float32(1) - float32(1e-5): the fold scale in double is 1 + 6.8e-9
      channels    channel c of a tensor carries a . 2^g(c), g(c) in {0, 1} seeded per tensor (the residual stream of a stage shares one g: the identity
                  shortcut adds equal channels).  A (cout, cin) entry of a non-zero tap is 2^(g_out(cout) - g_in(cin)) / cin_used: the sum over the input channels
                  is a . 2^g_out(cout) exactly, and a kernel that permutes channels meets unequal gains (two swapped channels of unequal g: 0.5 / cin relative)
      cin_used    cin, but 64 for the small models' 96-channel inputs (input channels 64 .. 95 get zero weights): the factor stays a power of two
      stride 1    ONE non-zero tap (ty, tx) per 3 x 3 conv, seeded per conv and per tap set; the centre tap where the output map is <= 2 x 2.  conv2 of the
                  identity block takes the MIRROR of its conv1's tap: the block doubles a pixel in place (not at a border the shift leaves through), and the
                  number of paths that meet in a pixel stays a short sum of powers of two.  With free taps there it grows like a binomial coefficient, and
                  37 m leaves fp16's eleven bits at some of the 512 subset positions (64 x 64, measured: 4e-4 .. 8e-4 for five seeds of six)
      stride 2    conv1 of each stage: a 2 x 2 group of taps at a seeded offset in {0, 1}^2; every input pixel reaches at most one output pixel (none: the
                  last row / column under a group that looks up / left); the centre tap alone where the input map is 1 x 1.  The group is NOT scaled by 2^-2:
                  with it a path through the group and one through the shortcut rejoin as a (1 + 1/4), and 37 . 5^k leaves fp16's eleven bits (measured: 4e-4).
                  The all-ones CU grows by 5 x 2 per stage instead, which the stem's gain STEM[size] (2^-2 / 2^-5) takes back: condition (b)
      shortcut    1 x 1, every entry 2^(g_out - g_in) / cin_used
      stem        one tap per input plane, STEM[size] . 1023 . 2^-10 . 2^g(cout)
      heads       feature column c of class k: 2^-k . 2^-g(c) / C_used; poc / qp columns and biases 0
  TAPSETS         tap sets 0 and 1 give conv c the taps base_c and (base_c + 3) mod 9 of its seeded base tap (a stride-2 group: two of the four offsets); tap set 2
                  is the CENTRE set: every stride-1 tap and both stem taps in the centre, every stride-2 group at offset (1, 1) -- every pixel of every map has a
                  path to every head there (no expectation is 0), which is what lets a mutation at a map's corner be seen.  Two to three of the nine taps of
                  every conv are used; all nine would take nine sets, and each costs the CPU test a minute at 128 x 128

Nothing is negative and there is no bias: logit_k = G[k] . (org plane, residual plane) as with the tracer weights -- tw.adjoint gives G, tw.expected the
reference for any content.  G is exactly 0 where every path of a pixel leaves the map (a shifted impulse at a border, an odd row under a stride-2 group that
looks the other way): such a logit's expectation is 0, and the device must return exactly 0.0.

Amplitudes: 512, 37 and 1 (1023 is NOT rounding-free: 1023 . 2^-10 has ten mantissa bits).  Amplitude 1 runs on the set with the stem 2^10 larger (STEM_LOW),
as the tracer's amplitude family does: its activations would otherwise lie in fp16's subnormal range (condition (c)).

Sizes: 128 and 64 -- the sizes the GPU test's configurations name.  32 and 16 are left out: under this construction their deep heads see 2 x 2 and 1 x 1 maps,
where every conv is pinned to the centre tap and most impulses have no path to them.

Tolerance: RHO_SHIFT[size] = 8 x max(the largest relative deviation of Net64("fp16") / Net64("hilo") from float64 on the family, SHIFT_ORACLE_MEASURED[size],
2^-24) -- tests/test_shift_cpu.py recomputes it and holds the table to within 5 %.  No figure here comes from a device run."""
import numpy as np

import tracer_weights as tw

SEED = {128: 2029, 64: 2032}         # per size: the first seeds whose two seeded tap sets meet condition (d) (64 x 64 with 2029: 23 % in tap set 1)
CENTRE = 2                            # the tap set with every tap in the centre
SIZES = (128, 64)
TAPSETS = (0, 1, 2)
AMPLITUDES = (512, 37, 1)
STEM = {128: 2.0 ** -2, 64: 2.0 ** -5}  # the stem's gain: the all-ones CU grows by 5 x 2 per stage (four taps + the shortcut, then the identity block)
STEM_LOW = 1024.0                     # ... times this in the sets that amplitude 1 runs on
MIRROR = True
S2_SCALE = 1.0                        # the stride-2 group's scale
BN_VAR = np.float32(1) - np.float32(1e-5)

# |expected - C oracle| / expected on the family's impulse CUs as measured by tests/test_shift_cpu.py (36 CUs per tap set), rounded up.  (The oracle's own fp32
# accumulation on DENSE content -- 8 further CUs per size, 3.7e-6 / 4.8e-6 -- is held to the tracer test's bound and is no property of `expected` on the family.)
SHIFT_ORACLE_MEASURED = {128: 1.0e-7, 64: 1.02e-7}
# the largest relative deviation of the fp16 / hilo emulations from float64 over the family (test_shift_cpu.py: condition (a)), rounded up
SHIFT_EMULATED = {128: 0.9e-7, 64: 1.02e-7}
RHO_SHIFT = {128: 8.0e-7, 64: 8.2e-7}


def stem_gain(size, amplitude):
    return STEM[size] * (STEM_LOW if amplitude == 1 else 1.0)


def conv_names(arch):
    """The 3 x 3 convs in forward order: [(key, stage, block, which)], the stem excluded."""
    n = len(tw.STAGE_PLANES[arch])
    return [(f"layer{s}.{b}.conv{w}", s, b, w) for s in range(n) for b in range(2) for w in (1, 2)]


def map_of(size, s):
    """Output map side of stage s."""
    return max(size >> (s + 1), 1)


def taps(size, tapset=0, seed=None):
    """{conv key: [(ty, tx), ...]} -- the non-zero taps of every 3 x 3 conv (the stem: one per input plane).  Stride-1 convs: one tap; stride-2 convs: the 2 x 2
    group.  The base assignment is seeded per (size, conv); tap set j moves every free tap by 3 j positions of the nine (a stride-2 group: its offset to the
    j-th next of the four)."""
    arch = tw.arch_of(size)
    g = np.random.default_rng([SEED[size] if seed is None else seed, size])
    out = {}
    base = g.integers(0, 9, size=2)
    out["conv1"] = [(1, 1) if tapset == CENTRE else divmod(int((b + 3 * tapset) % 9), 3) for b in base]
    for key, s, b, w in conv_names(arch):
        h_out = map_of(size, s)
        h_in = map_of(size, s - 1) if s > 0 else size
        t9, o4 = int(g.integers(0, 9)), int(g.integers(0, 4))
        if b == 0 and w == 1:                                   # the stride-2 conv of the stage
            if h_in == 1:
                out[key] = [(1, 1)]
            else:
                oy, ox = (1, 1) if tapset == CENTRE else divmod((o4 + tapset) % 4, 2)
                out[key] = [(oy + i, ox + j) for i in (0, 1) for j in (0, 1)]
        elif b == 1 and w == 2 and MIRROR:                      # the identity block's conv2 undoes its conv1's shift: the block doubles a pixel in place
            (ty, tx), = out[key[:-1] + "1"]
            out[key] = [(2 - ty, 2 - tx)]
        else:
            out[key] = [(1, 1)] if h_out <= 2 or tapset == CENTRE else [divmod((t9 + 3 * tapset) % 9, 3)]
    return out


def _gains(g, c):
    return np.exp2(g.integers(0, 2, size=c).astype(np.float64))


def shift_state_dict(size, tapset=0, stem=None, seed=None, tap_override=None):
    """The state dict of (size, tap set).  stem: the stem's gain (a power of two).  tap_override: {conv key: [(ty, tx), ...]} replaces the taps of those convs (the
    tap mutations of tests/test_shift_cpu.py)."""
    arch = tw.arch_of(size)
    stem = STEM[size] if stem is None else stem
    pkg = tw._pkg()
    sd = {k: np.array(v, copy=True) for k, v in pkg.synth.make_state_dict(arch, 1).items()}
    tp = taps(size, tapset, seed)
    if tap_override:
        tp.update(tap_override)
    g = np.random.default_rng([SEED[size] if seed is None else seed, size, 7])
    planes = tw.STAGE_PLANES[arch]
    used = lambda c: 64 if c == 96 else c
    for key, v in sd.items():
        if key.endswith("num_batches_tracked"):
            continue
        if key.endswith(".running_mean") or key.endswith(".bias"):
            v[...] = 0.0
        elif key.endswith(".running_var"):
            v[...] = BN_VAR
        elif v.ndim == 1 and key.endswith(".weight"):
            v[...] = 1.0
        elif v.ndim in (2, 4):
            v[...] = 0.0
        else:
            raise KeyError(key)
    g_stem = _gains(g, 32)
    for p in range(2):
        ty, tx = tp["conv1"][p]
        sd["conv1.weight"][:, p, ty, tx] = (stem * 1023.0 * 2.0 ** -10 * g_stem).astype(np.float32)
    g_in = g_stem
    for s, c in enumerate(planes):
        g_res, g_t0, g_t1 = _gains(g, c), _gains(g, c), _gains(g, c)      # the stage's residual stream, the conv1 activations of its two blocks
        cin = len(g_in)
        cu = used(cin)
        w_in = np.where(np.arange(cin) < cu, 1.0 / (g_in * cu), 0.0)     # [cin]: 2^-g_in / cin_used on the used input channels
        p = f"layer{s}"
        for ty, tx in tp[f"{p}.0.conv1"]:
            sd[f"{p}.0.conv1.weight"][:, :, ty, tx] = np.outer(g_t0, w_in) * (S2_SCALE if len(tp[f"{p}.0.conv1"]) == 4 else 1.0)
        sd[f"{p}.0.shortcut.0.weight"][:, :, 0, 0] = np.outer(g_res, w_in)
        cu = used(c)
        inv = lambda gg: np.where(np.arange(c) < cu, 1.0 / (gg * cu), 0.0)
        for key, go, gi in ((f"{p}.0.conv2", g_res, g_t0), (f"{p}.1.conv1", g_t1, g_res), (f"{p}.1.conv2", g_res, g_t1)):
            (ty, tx), = tp[key]
            sd[key + ".weight"][:, :, ty, tx] = np.outer(go, inv(gi))
        if s >= 1:
            K = sd[f"branch{s}.weight"].shape[0]
            sd[f"branch{s}.weight"][:, :c] = np.outer(2.0 ** -np.arange(K), inv(g_res))
        g_in = g_res
    for k, v in sd.items():
        assert v.dtype == np.float32 or k.endswith("num_batches_tracked"), k
    return sd


def shift_blob(size, tapset=0, stem=None):
    return tw._pkg().weights.pack_blob(tw.arch_of(size), shift_state_dict(size, tapset, stem))


def expected_impulse(G, plane, pos, amplitude):
    return tw.expected_impulse(G, plane, pos, amplitude)


def adjoint(sd, size, mutation=None, check=True):
    """tw.adjoint without its `G . x > 0` assertion (G has exact zeros here): linearity on random non-negative content to 1e-12, the zero CU exactly 0."""
    import torch
    G = tw.adjoint(sd, size, mutation=mutation, check=False)
    if check:
        net = tw.Net64(sd)
        rng = np.random.default_rng([size, 5])
        xs = rng.random((3, 2, size, size))
        xs[1] *= rng.random((2, size, size)) < 0.02
        xs[2, 0] = 0.0
        with torch.no_grad():
            got = net.forward(torch.from_numpy(xs), mutation=mutation).numpy()
            z = net.forward(torch.zeros((1, 2, size, size), dtype=torch.float64)).numpy()
        want = np.einsum("kpyx,npyx->nk", G, xs)
        assert (G >= 0).all() and np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), "the shift network is not linear on non-negative input"
        assert (z == 0.0).all(), "the zero CU must give logits exactly 0"
    return G


def family(size, positions=None):
    """The CUs conditions (a) and (c) are stated on: impulses of every amplitude in each plane at `positions` (default tw.sample_positions(size, 24, 40)).
    -> [(amplitude, plane, org, pred)]"""
    pos = tw.sample_positions(size, 24, 40) if positions is None else positions
    return [(a, p) + tw.impulses(size, p, pos, a) for a in AMPLITUDES for p in (0, 1)]


def odd_amplitude_positions(size, tapset):
    """Where the GPU test runs the one amplitude that is no power of two, beyond the family's sample: the 512-position subset, on tap set 0 (the mixed
    configurations' second amplitude).  37 m must fit fp16's eleven bits for the number m of paths that meet in a pixel; for 512 and 1 that holds of any m < 2048."""
    return np.setdiff1d(tw.subset_positions(size), tw.sample_positions(size, 24, 40)) if tapset == 0 else np.zeros(0, np.int64)


def emulated_deviation(size, tapset, positions=None):
    """Condition (a): {rounding: the largest |Net64(rounding) - Net64(None)| / Net64(None) over the family's non-zero logits}; a logit that is exactly 0 in float64
    must be exactly 0 under either rounding.  Amplitude 37 is held on every further position the GPU test uses it at as well (there: the fp16 rounding alone -- where
    it is the identity, so is the (hi, lo) pair)."""
    worst = {"fp16": 0.0, "hilo": 0.0}
    for stem in sorted({stem_gain(size, a) for a in AMPLITUDES}):
        sd = shift_state_dict(size, tapset, stem)
        ref, emu = tw.Net64(sd), {r: tw.Net64(sd, r) for r in worst}
        fam = [f + (tuple(worst),) for f in family(size, positions)]
        extra = odd_amplitude_positions(size, tapset)
        if positions is None and len(extra):
            fam += [(37, p) + tw.impulses(size, p, extra, 37) + (("fp16",),) for p in (0, 1)]
        for a, p, org, pred, roundings in fam:
            if stem_gain(size, a) != stem:
                continue
            x = tw.preprocess(org, pred)
            want = tw.forward64(ref, x)
            for r in roundings:
                got = tw.forward64(emu[r], x)
                assert (got[want == 0.0] == 0.0).all(), (size, tapset, a, p, r)
                nz = want > 0
                if nz.any():
                    worst[r] = max(worst[r], float((np.abs(got[nz] - want[nz]) / want[nz]).max()))
    return worst


def rho_shift(size):
    return RHO_SHIFT[size]


# ---- the mixed configurations of the 128 model (tests/test_shift_gpu.py runs them, tests/test_shift_cpu.py holds their coverage of run_network's lo offsets) -----
# (name, tuning switches around the constructor, w2_units, x_units the context must report, full sweep as well).  MLT_W2_MASK is kept outright by the tier search;
# MLT_X_MASK / MLT_X_UNITS are reached once the single pass and the fifteen hi+lo-weights subsets have admitted nothing: those contexts are built with a tolerance no
# fp16 tier can meet.  0xFA = every chain unit alone (0xAA) plus the stride-2 units of layer2 / layer3, which may not stay on the single pass in front of a
# two-plane chain (illegal_w2_unit_drop).  MLT_X_UNITS = 0x0A (layer0.1 and layer1's chain exact behind hi+lo-weights units) is the one state of layer0 the issue's
# list leaves out: conv1 of layer0.1 reading a single-plane b0 (x_lo = 0) and its conv2 adding it (res_lo = 0).
MIXED_128 = [
    ("w2 layer0", {"MLT_W2_MASK": "1"}, 0x03, 0, False),
    ("w2 layer1", {"MLT_W2_MASK": "2"}, 0x0C, 0, False),
    ("w2 layer2", {"MLT_W2_MASK": "4"}, 0x30, 0, False),
    ("w2 layer3", {"MLT_W2_MASK": "8"}, 0xC0, 0, False),
    ("w2 stride-2 units", {"MLT_W2_MASK": "15", "MLT_W2_UNITS": "0x55"}, 0x55, 0, False),
    ("w2 chain units", {"MLT_W2_MASK": "15", "MLT_W2_UNITS": "0xFA"}, 0xFA, 0, False),
    ("x layer2", {"MLT_X_MASK": "4"}, 0xCF, 0x30, True),
    ("x layer1+2", {"MLT_X_MASK": "6"}, 0xC3, 0x3C, False),
    ("x layer0", {"MLT_X_MASK": "1"}, 0xFC, 0x03, False),
    ("x layer3", {"MLT_X_MASK": "8"}, 0x3F, 0xC0, False),
    ("x units 0xF8 behind w2 0x07", {"MLT_X_UNITS": "0xF8", "MLT_W2_UNITS": "0x07"}, 0x07, 0xF8, True),
    ("x units 0x54", {"MLT_X_UNITS": "0x54"}, 0xAB, 0x54, False),
    ("x units 0x0A", {"MLT_X_UNITS": "0x0A"}, 0xF5, 0x0A, False),
]
STALE_N = (96, 600)                   # the two batch classes of the stale-plane runs


def needs_tolerance(env):
    """A configuration the search reaches only when nothing cheaper is admitted."""
    return "MLT_X_MASK" in env or "MLT_X_UNITS" in env


def plan_lines(pkg, blob, size, n, tier=0, w2_units=0, x_units=0, detail=False):
    import ctypes as C
    lib = pkg.capi.load_library()
    lib.mlt_plan_describe.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    k = lib.mlt_plan_describe(blob, len(blob), size, n, tier, w2_units, x_units, 3 if detail else 1, buf, 1 << 16)
    lines = buf.value.decode().splitlines()
    assert k == len(lines) and k > 0, (k, len(lines))
    return lines


def units_of_line(line):
    """The launch units (bit indices of w2_units / x_units) of a plan line of the 128 model; () for the heads and the guard statistic.  (A 32 -> 32 stride-1 conv is
    counted to layer0.1; behind stem5x5 the first of them is layer0.0's conv2 -- there both units run the same arithmetic.)"""
    import re
    name = line.split(" [")[0].split(" {")[0]
    planes = tw.STAGE_PLANES[0]
    if name.startswith(("heads", "guard_flat_stat")):
        return ()
    if name.startswith("layer0_stream"):
        return (0, 1, 2) if "layer1.0.conv1" in name else (0, 1)
    if name.startswith(("stem+block_s2", "stem5x5")):
        return (0,)
    if name.startswith("block_s1_32"):
        return (1,)
    if name.startswith("layer1_stream"):
        return (3,)
    m = re.match(r"stage_(\d+)_h", name)
    if m:
        st = planes.index(int(m.group(1)))
        return (2 * st, 2 * st + 1)
    m = re.match(r"chain3_s1_(\d+)_h", name)
    if m:
        return (2 * planes.index(int(m.group(1))) + 1,)
    m = re.match(r"conv3x3_s(\d)_\d+to(\d+)_h", name)
    assert m, line
    st = planes.index(int(m.group(2)))
    return (2 * st,) if m.group(1) == "2" else (2 * st + 1,)


def check_plan_arithmetic(lines, w2_units, x_units):
    """Every launch of a plan runs the arithmetic its units' masks say: "[exact" for x_units, "hi+lo weights" for w2_units, "single pass" (or a fused streaming
    kernel without a tag) otherwise."""
    seen = set()
    for l in lines:
        us = units_of_line(l)
        if not us:
            continue
        want = {"exact" if (x_units >> u) & 1 else "hi+lo weights" if (w2_units >> u) & 1 else "single pass" for u in us}
        assert len(want) == 1, (l, want)
        want = want.pop()
        head = l.split(" {")[0]
        tag = head.split("[", 1)[1] if "[" in head else ""
        if any(t in tag for t in ("exact", "hi+lo weights", "single pass")):
            assert want in tag and sum(t in tag for t in ("exact", "hi+lo weights", "single pass")) == 1, (l, want)
        else:
            assert want == "single pass", (l, want)
        seen.update(us)
    assert seen == set(range(8)), (sorted(seen), lines)


def lo_states(lines):
    """The (role, x_lo != 0, res_lo != 0) of every [exact] per-conv launch of a detailed plan: role S2 (stride-2 conv + shortcut), B0C2 (conv2 of block 0: the s1 conv
    with a residual that does not follow a conv1), B1C1 (the s1 conv without residual), B1C2 (the s1 conv with a residual behind a B1C1)."""
    import re
    out, prev = [], None
    for l in lines:
        role = None
        if l.startswith("conv3x3_s2"):
            role = "S2"
        elif l.startswith("conv3x3_s1"):
            role = "B1C1" if " res=" not in l else "B1C2" if prev == "B1C1" else "B0C2"
        prev = role
        if role and "[exact" in l.split(" {")[0]:
            f = dict(kv.split("=") for kv in re.search(r"\{(.*)\}", l).group(1).split())
            out.append((role, l.split("_h")[0], int(f["x_lo"]) != 0, int(f["res_lo"]) != 0))
    return out


# ---- tap mutations ------------------------------------------------------------------------------------------------------------------------------------------
def tap_mutations(size, tapset=0):
    """[(name, {conv key: taps})]: ONE tap of one conv zeroed (a stride-2 group: one of its four) or moved to a neighbouring tap -- what turns some expected logit
    of the sweep from non-zero to zero or the reverse."""
    tp = taps(size, tapset)
    out = []
    for key in ("layer0.0.conv1", "layer1.0.conv1", "layer2.0.conv1"):
        gone = [t for t in tp[key] if t != (1, 1)][0]          # (the centre tap reads the pixel the shortcut reads as well: zeroing it alone leaves a path)
        out.append((f"{key}: tap {gone} zeroed", {key: [t for t in tp[key] if t != gone]}))
    for key in ("layer0.1.conv1", "layer1.0.conv2", "layer1.1.conv2", "layer2.1.conv1"):
        (ty, tx), = tp[key]
        moved = (ty, tx + 1) if tx < 2 else (ty, tx - 1)
        out.append((f"{key}: tap {(ty, tx)} moved to {moved}", {key: [moved]}))
    (ty, tx) = tp["conv1"][1]
    out.append((f"stem, residual plane: tap {(ty, tx)} moved", {"conv1": [tp["conv1"][0], ((ty + 1) % 3, tx)]}))
    return out


if __name__ == "__main__":
    import time
    for size in SIZES[::-1]:
        for ts in TAPSETS:
            t0 = time.time()
            sd = shift_state_dict(size, ts)
            G = adjoint(sd, size)
            plane, pos = tw.sweep(size)
            e = tw.expected_impulse(G, plane, pos, 512)
            hk = tw.head_of_logit(tw.arch_of(size))
            print(size, ts, "all logits > 0: %.0f %%" % (100 * (e > 0).all(axis=1).mean()), "per head non-zero:",
                  [f"{100 * (e[:, hk == h] > 0).all(axis=1).mean():.0f} %" for h in range(hk.max() + 1)],
                  "all-ones top %.4g" % tw.activation_report(sd, np.ones((1, 2, size, size))), emulated_deviation(size, ts, tw.sample_positions(size, 8, 12)), f"{time.time() - t0:.1f} s", flush=True)
