"""Tracer weights: a positive, ReLU-free weight set whose logits are LINEAR in the two input planes, and the float64 adjoint of that map.

Three designed weight families hold the convolution kernels to float64 per pixel, in front of the pooling (everything else sees pooled logits of seeded random
weights at |dlogit| <= 1e-3: global average pooling divides a wrong pixel by the map area, and the seeded BN shifts put an O(1) baseline under it).  This one
covers the MFMA sums, the taps, strides, padding and tile seams of every path at every pixel position, with every epilogue a no-op; tests/shift_weights.py
covers every arithmetic tier and every hand-off between them at ~1e-6, on weights for which no tier rounds; tests/gated_weights.py covers what both switch off on
purpose -- the folded bias and the shortcut's, the order of add and ReLU, the clamp at zero and the BatchNorm fold of negative and far-from-1 scales.  With the
weights of this module nothing hides a pixel:

  tracer_state_dict   the seeded state dict with identity BatchNorm (weight 1, bias 0, mean 0, var 1), every conv weight g (0.5 + u) / (cin kh kw) with u from
                      synth.uniform -- g = GAINS["stride2"] on the stride-2 conv1 of each stage, GAINS["other"] elsewhere --, head feature columns
                      (0.5 + u) / C, head poc / qp columns and biases 0.  All weights > 0, no bias anywhere: no ReLU ever clips on the non-negative planes the
                      preprocessing produces, the zero CU gives logits exactly 0, and logit_k = sum_{plane, y, x} G[k, plane, y, x] * plane[y, x].
  forward64           the network in float64 on torch.nn.functional, BN folded in double; rounding = "fp16" rounds the folded conv weights, the stem output and
                      every block activation (the conv1 activation inside the block and the block's output) to fp16, "hilo" to h + half(a - h)
  adjoint             G[K, 2, S, S]: one forward and K backward passes at the all-0.5 input (torch's ReLU gradient at 0 is 0: the adjoint at a zero input
                      would be identically zero), linearity asserted on random non-negative content
  expected            the preprocessing restated (uint16 cast, absdiff, * float32(1 / 1023), clip) and the dot product with G in float64: the reference for ANY
                      content
  mutations / adjoint(..., mutation=)
                      eight single-pixel perturbations (ONE output pixel of ONE layer scaled by 8/9): what the tolerance must be able to see

Nothing of oracle/ and nothing of the kernels' emulator is imported; of the package only synth and weights.pack_blob.

Tolerance (tests/test_tracer_cpu.py derives it, tests/test_tracer_gpu.py uses it): RHO_FAST[size][head] = 8 x the largest relative error of
forward64(rounding="fp16") against float64 over `sample_positions` (four corners, 64 border and 256 interior positions per plane, impulses of 1023),
RHO_EXACT the same with "hilo" and not below 8 x the measured error of `expected` against the C oracle.  The tables below are the CPU emulation's figures
(`python tests/tracer_weights.py` prints them); the CPU test recomputes them and fails when the committed table is not what the emulation gives.  No
figure here comes from a device run.

rho as measured by the emulation (seed 77, GAINS as below; per head, first to last; docs/NUMERICS.md "Tracer weights" has the device's figures beside them):
  size   rho_fast                               rho_exact
  128    8.4e-4  9.7e-4  1.12e-3                1.2e-5  4.6e-5  5.6e-4
   64    8.4e-4  1.01e-3 1.00e-3 1.18e-3        1.2e-5  6.8e-5  4.6e-4  7.4e-4
   32    8.4e-4  1.07e-3 1.13e-3 1.66e-3        1.2e-5  2.4e-5  4.7e-5  2.1e-4
   16    8.5e-4  9.0e-4  1.34e-3 1.71e-3        1.2e-5  1.2e-5  2.9e-5  3.3e-5
(1.2e-5 is the floor 8 x ORACLE_MEASURED; the emulation alone gives 5.6e-6 .. 1.0e-5 there.  The worst case 3 L 2^-11 is 1.3e-2 .. 3.1e-2 for L = 9 .. 21.)"""
import numpy as np

SEED = 77
GAINS = {"stem": 1.0, "stride2": 2.0, "other": 1.0}
# the amplitude family (impulses of 1, 37 and 700): the stem 2^10 larger, so that an impulse of ONE ten-bit step keeps its activations out of fp16's subnormal
# range (the underflow condition of tests/test_tracer_cpu.py; a power of two: G is exactly 1024 x the base set's).  Dense content would overflow with it.
GAINS_LOW = {"stem": 1024.0, "stride2": 2.0, "other": 1.0}
STAGE_PLANES = {0: (32, 64, 128, 256), 1: (32, 64, 96, 128, 256)}
HEAD_CLASSES = {0: (2, 3, 4), 1: (2, 3, 4, 6)}
BN_EPS = 1e-5
AMPLITUDE = 1023
SCALE = np.float32(1.0 / 1023)


def _pkg():
    import mltcnn_pkg
    return mltcnn_pkg.load()


def arch_of(size):
    return 0 if size == 128 else 1


def n_convs_before_head(arch, head):
    """L of the worst-case bound 3 L 2^-11: convs on the longest path from the input to head `head` (stem + two per block; the shortcut runs beside conv1 / conv2)."""
    return 1 + 4 * (head + 2)


# ---- weights ------------------------------------------------------------------------------------------------------------------------------------------
def tracer_state_dict(arch, seed=SEED, gains=None):
    gains = GAINS if gains is None else gains
    pkg = _pkg()
    sd = {k: np.array(v, copy=True) for k, v in pkg.synth.make_state_dict(arch, seed).items()}
    for key, v in sd.items():
        if key.endswith("num_batches_tracked"):
            continue
        if key.endswith(".running_mean") or (v.ndim == 1 and key.endswith(".bias") and not key.startswith("branch")):
            v[...] = 0.0
        elif key.endswith(".running_var") or (v.ndim == 1 and key.endswith(".weight")):
            v[...] = 1.0
        elif v.ndim == 4:
            cout, cin, kh, kw = v.shape
            g = gains["stem"] if key == "conv1.weight" else gains["stride2"] if key.endswith(".0.conv1.weight") else gains["other"]
            u = pkg.synth.uniform(seed, "tracer/" + key, v.size).reshape(v.shape)
            v[...] = (g * (0.5 + u) / (cin * kh * kw)).astype(np.float32)
        elif key.startswith("branch") and key.endswith(".weight"):
            K, c2 = v.shape
            C = c2 - 2
            u = pkg.synth.uniform(seed, "tracer/" + key, K * C).reshape(K, C)
            v[:, :C] = ((0.5 + u) / C).astype(np.float32)
            v[:, C:] = 0.0
        elif key.startswith("branch") and key.endswith(".bias"):
            v[...] = 0.0
        else:
            raise KeyError(key)
    return sd


def tracer_blob(arch, seed=SEED, gains=None):
    return _pkg().weights.pack_blob(arch, tracer_state_dict(arch, seed, gains))


# ---- the network in float64 ----------------------------------------------------------------------------------------------------------------------------
def _half(t):
    import torch
    return t.to(torch.float16).to(torch.float64)


def _rnd(t, rounding):
    if rounding is None:
        return t
    h = _half(t)
    if rounding == "fp16":
        return h
    assert rounding == "hilo", rounding
    return h + _half(t - h)


class Net64:
    """The folded network of one state dict; sites (in forward order): "stem", then per block "layerL.B.conv1" (after its ReLU) and "layerL.B.out"."""

    def __init__(self, sd, rounding=None):
        import torch
        self.rounding = rounding
        self.n_stages = 1 + max(int(k[5]) for k in sd if k.startswith("layer"))
        t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64).copy())

        def fold(conv, bn):
            w = t64(sd[conv + ".weight"])
            if bn is None:
                return _rnd(w, rounding), None
            s = t64(sd[bn + ".weight"]) / torch.sqrt(t64(sd[bn + ".running_var"]) + BN_EPS)
            return _rnd(w * s[:, None, None, None], rounding), t64(sd[bn + ".bias"]) - t64(sd[bn + ".running_mean"]) * s

        self.stem = fold("conv1", None)[0]
        self.blocks = []
        for s in range(self.n_stages):
            for b in range(2):
                p = f"layer{s}.{b}"
                self.blocks.append((p, 2 if b == 0 else 1, fold(p + ".conv1", p + ".bn1"), fold(p + ".conv2", p + ".bn2"),
                                    fold(p + ".shortcut.0", p + ".shortcut.1") if b == 0 else None))
        self.heads = [(t64(sd[f"branch{s}.weight"]), t64(sd[f"branch{s}.bias"])) for s in range(1, self.n_stages)]
        self.sites = ["stem"] + [f"{p}.{w}" for p, *_ in self.blocks for w in ("conv1", "out")]

    def forward(self, x, poc=None, qp=None, mutation=None, keep=None):
        """x: float64 [n, 2, S, S] -> logits [n, K].  mutation = (site, y, x, factor): that output pixel (every channel) of that site is scaled.
        keep: a dict that receives every site's activation tensor."""
        import torch
        import torch.nn.functional as F
        n = x.shape[0]

        def site(name, t):
            if mutation is not None and mutation[0] == name:
                m = torch.ones(t.shape[2:], dtype=t.dtype)
                m[mutation[1], mutation[2]] = mutation[3]
                t = t * m
            t = _rnd(t, self.rounding)
            if keep is not None:
                keep[name] = t
            return t

        cur = site("stem", F.conv2d(x, self.stem, padding=1))
        extra = torch.zeros((n, 2), dtype=torch.float64)
        if poc is not None:
            extra = torch.stack([torch.as_tensor(np.asarray(poc, np.float64)), torch.as_tensor(np.asarray(qp, np.float64))], dim=1)
        outs = []
        for i, (p, stride, (w1, b1), (w2, b2), sc) in enumerate(self.blocks):
            t = site(p + ".conv1", F.relu(F.conv2d(cur, w1, b1, stride=stride, padding=1)))
            u = F.conv2d(t, w2, b2, padding=1)
            if sc is not None:
                cur = F.conv2d(cur, sc[0], sc[1], stride=stride)
            cur = site(p + ".out", F.relu(u + cur))
            if i % 2 == 1 and i >= 3:
                w, b = self.heads[i // 2 - 1]
                outs.append(F.linear(torch.cat([cur.mean(dim=(2, 3)), extra], dim=1), w, b))
        return torch.cat(outs, dim=1)


def forward64(sd, x, rounding=None, mutation=None, chunk=64):
    """x: float64 [n, 2, S, S] (numpy) -> logits float64 [n, K] (numpy)."""
    import torch
    net = sd if isinstance(sd, Net64) else Net64(sd, rounding)
    x = np.asarray(x, np.float64)
    with torch.no_grad():
        return np.concatenate([net.forward(torch.from_numpy(x[i:i + chunk]), mutation=mutation).numpy() for i in range(0, len(x), chunk)])


def preprocess(org, pred):
    """int16 [n, S, S] x 2 -> the two input planes, float64 [n, 2, S, S], every value a float32 (EncCu.cpp: uint16 cast, absdiff, * (float)(1 / 1023), clip)."""
    o = np.ascontiguousarray(org, np.int16).view(np.uint16).astype(np.float32)
    p = np.ascontiguousarray(pred, np.int16).view(np.uint16).astype(np.float32)
    a = np.clip(o * SCALE, np.float32(0), np.float32(1))
    r = np.clip(np.abs(o - p) * SCALE, np.float32(0), np.float32(1))
    assert a.dtype == np.float32 and r.dtype == np.float32
    return np.stack([a, r], axis=1).astype(np.float64)


def adjoint(sd, size, mutation=None, check=True):
    """G[K, 2, S, S] float64: dlogit_k / dplane[y, x] at the all-0.5 input.  check: forward64 on random non-negative content equals G . x to 1e-12 relative."""
    import torch
    net = Net64(sd)
    x = torch.full((1, 2, size, size), 0.5, dtype=torch.float64, requires_grad=True)
    y = net.forward(x, mutation=mutation)[0]
    K = y.shape[0]
    G = np.empty((K, 2, size, size), np.float64)
    for k in range(K):
        g, = torch.autograd.grad(y[k], x, retain_graph=k + 1 < K)
        G[k] = g[0].numpy()
    if check:
        rng = np.random.default_rng([size, 5])
        xs = rng.random((3, 2, size, size))
        xs[1] *= rng.random((2, size, size)) < 0.02           # sparse content: most of the planes exactly zero
        xs[2, 0] = 0.0
        with torch.no_grad():
            got = net.forward(torch.from_numpy(xs), mutation=mutation).numpy()
        want = np.einsum("kpyx,npyx->nk", G, xs)
        assert (want > 0).all() and np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), "the tracer network is not linear on non-negative input"
        z = net.forward(torch.zeros((1, 2, size, size), dtype=torch.float64)).detach().numpy()
        assert (z == 0.0).all(), "the zero CU must give logits exactly 0"
    return G


def expected(G, org, pred):
    """float64 [n, K]: G . preprocess(org, pred) -- the reference for any content."""
    x = preprocess(org, pred)
    n = x.shape[0]
    return x.reshape(n, -1) @ G.reshape(G.shape[0], -1).T


# ---- content families ------------------------------------------------------------------------------------------------------------------------------------
def impulses(size, plane, pos, amplitude=AMPLITUDE):
    """CUs with ONE non-zero pixel of ONE input plane.  plane 0 (org): org = pred = v at the pixel; plane 1 (resi): org = 0, pred = v; plane 2: both planes
    at once (org = v, pred = 0).  pos: [m] flat pixel indices y * S + x.  -> org, pred int16 [m, S, S]."""
    pos = np.asarray(pos, np.int64)
    m = len(pos)
    org = np.zeros((m, size * size), np.int16)
    pred = np.zeros((m, size * size), np.int16)
    r = np.arange(m)
    if plane in (0, 2):
        org[r, pos] = amplitude
    if plane in (0, 1):
        pred[r, pos] = amplitude
    return org.reshape(m, size, size), pred.reshape(m, size, size)


def sweep(size, seed=1):
    """The full impulse sweep in a seeded shuffled order: (plane[m], pos[m]) with m = 2 S^2, every (plane, pixel) exactly once."""
    m = 2 * size * size
    order = np.random.default_rng([size, seed]).permutation(m)
    assert np.array_equal(np.sort(order), np.arange(m))
    return (order // (size * size)).astype(np.int64), (order % (size * size)).astype(np.int64)


def sweep_chunk(size, plane, pos):
    """org, pred of sweep entries (mixed planes)."""
    m = len(pos)
    org = np.zeros((m, size * size), np.int16)
    pred = np.zeros((m, size * size), np.int16)
    r = np.arange(m)
    pred[r, pos] = AMPLITUDE
    o = plane == 0
    org[r[o], pos[o]] = AMPLITUDE
    return org.reshape(m, size, size), pred.reshape(m, size, size)


def expected_impulse(G, plane, pos, amplitude=AMPLITUDE):
    """float64 [m, K] of impulse CUs, by gather (equal to expected() on the same CUs: one non-zero term)."""
    v = float(np.clip(np.float32(amplitude) * SCALE, np.float32(0), np.float32(1)))
    K = G.shape[0]
    Gf = G.reshape(K, 2, -1)
    plane, pos = np.asarray(plane), np.asarray(pos)
    if np.ndim(plane) == 0:
        plane = np.full(len(pos), int(plane))
    out = np.where((plane == 0)[:, None], Gf[:, 0, pos].T, 0.0) + np.where((plane == 1)[:, None], Gf[:, 1, pos].T, 0.0)
    both = plane == 2
    if both.any():
        out[both] = (Gf[:, 0, pos[both]] + Gf[:, 1, pos[both]]).T
    return out * v


def subset_positions(size, count=512, seed=2):
    """A seeded subset of `count` flat positions (all of them when the CU has no more), the four corners always among them."""
    S2 = size * size
    if S2 <= count:
        return np.arange(S2)
    corners = np.array([0, size - 1, S2 - size, S2 - 1])
    rest = np.setdiff1d(np.random.default_rng([size, seed]).permutation(S2), corners, assume_unique=True)[:count - 4]
    return np.sort(np.concatenate([corners, rest]))


def sample_positions(size, n_border=64, n_interior=256, seed=3):
    """The tolerance sample: the four corners, n_border further positions of the outermost ring and n_interior interior positions (all there are when fewer)."""
    yy, xx = np.mgrid[0:size, 0:size]
    ring = ((yy == 0) | (xx == 0) | (yy == size - 1) | (xx == size - 1)).reshape(-1)
    corners = np.array([0, size - 1, size * size - size, size * size - 1])
    g = np.random.default_rng([size, seed])
    border = np.setdiff1d(np.flatnonzero(ring), corners)
    interior = np.flatnonzero(~ring)
    border = np.sort(g.permutation(border)[:n_border])
    interior = np.sort(g.permutation(interior)[:n_interior])
    return np.concatenate([corners, border, interior])


def ring_families(size):
    """Non-zero surroundings, all-1023 in BOTH input planes (org = 1023, pred = 0) on a mask: the outermost ring alone, everything but the ring, single full
    rows and single full columns (every one for sizes <= 32, every 2nd for 64, every 4th plus 0, 1, S - 2, S - 1 for 128).  -> labels, org, pred."""
    step = 1 if size <= 32 else 2 if size == 64 else 4
    lines = sorted(set(range(0, size, step)) | ({0, 1, size - 2, size - 1} if size == 128 else set()))
    masks, labels = [], []
    ring = np.zeros((size, size), bool)
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = True
    masks += [ring, ~ring]
    labels += ["ring", "all but the ring"]
    for i in lines:
        m = np.zeros((size, size), bool); m[i, :] = True
        masks.append(m); labels.append(f"row {i}")
    for i in lines:
        m = np.zeros((size, size), bool); m[:, i] = True
        masks.append(m); labels.append(f"column {i}")
    org = (np.stack(masks) * AMPLITUDE).astype(np.int16)
    return labels, org, np.zeros_like(org)


def leakage_family(size, n=600, n_zero=40, seed=4):
    """n CUs all-1023 in both planes (org = 1023, pred = 0) except zero CUs at n_zero seeded batch indices plus the first and the last.  -> org, pred, is_zero."""
    g = np.random.default_rng([size, seed])
    zero = np.zeros(n, bool)
    zero[g.permutation(np.arange(1, n - 1))[:n_zero]] = True
    zero[0] = zero[-1] = True
    org = np.full((n, size, size), AMPLITUDE, np.int16)
    org[zero] = 0
    return org, np.zeros_like(org), zero


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------------------------
FACTOR = 8.0 / 9.0
# (site, map divisor, (y, x) on the 128 model's maps); the small models take the same fractions of their own map sizes
_MUT_128 = [("layer0.0.conv1", 2, (0, 63)), ("layer1.0.conv1", 4, (31, 0)), ("layer2.1.out", 8, (15, 15)), ("layer1.1.out", 4, (16, 16)),
            ("layer0.1.out", 2, (33, 17)), ("layer3.1.out", 16, (3, 4)), ("stem", 1, (0, 127)), ("layer2.1.conv1", 8, (5, 5))]


def mutations(size):
    """[(name, (site, y, x, 8/9))]: the eight single-pixel perturbations, on this size's own maps (position = the same fraction of the map, inside it)."""
    out = []
    for site, div, (y, x) in _MUT_128:
        M128, M = 128 // div, max(size // div, 1)
        yy, xx = min((y * M + M128 // 2) // M128, M - 1), min((x * M + M128 // 2) // M128, M - 1)
        if y == M128 - 1:
            yy = M - 1
        if x == M128 - 1:
            xx = M - 1
        out.append((f"{site} pixel ({yy},{xx})", (site, yy, xx, FACTOR)))
    return out


# ---- conditions -------------------------------------------------------------------------------------------------------------------------------------------
def activation_report(sd, x):
    """Largest float64 activation over every site for the content x [n, 2, S, S]."""
    import torch
    net = Net64(sd)
    worst = 0.0
    with torch.no_grad():
        for i in range(0, len(x), 16):
            keep = {}
            net.forward(torch.from_numpy(np.asarray(x[i:i + 16], np.float64)), keep=keep)
            worst = max(worst, max(float(t.max()) for t in keep.values()))
    return worst


def underflow_terms(sd, size, x):
    """First-order fp16 underflow term per CU and logit: 2^-25 x sum over the sites of sum_{0 < a < 2^-14} |dlogit_k / da| (an activation in fp16's
    subnormal range is rounded with an ABSOLUTE error of up to 2^-25; zeros and normal numbers are not).  x: float64 [n, 2, S, S] -> [n, K]."""
    import torch
    net = Net64(sd)
    x0 = torch.full((1, 2, size, size), 0.5, dtype=torch.float64, requires_grad=True)
    keep = {}
    y = net.forward(x0, keep=keep)[0]
    K = y.shape[0]
    names = list(keep)
    grads = {nm: [] for nm in names}
    for k in range(K):
        gs = torch.autograd.grad(y[k], [keep[nm] for nm in names], retain_graph=k + 1 < K, allow_unused=True)
        for nm, g in zip(names, gs):
            grads[nm].append(torch.zeros_like(keep[nm][0]) if g is None else g[0].abs())
    grads = {nm: torch.stack(v).reshape(K, -1) for nm, v in grads.items()}
    out = np.zeros((len(x), K))
    with torch.no_grad():
        for i in range(0, len(x), 16):
            act = {}
            net.forward(torch.from_numpy(np.asarray(x[i:i + 16], np.float64)), keep=act)
            for nm in names:
                a = act[nm].reshape(act[nm].shape[0], -1)
                sub = ((a > 0) & (a < 2.0 ** -14)).to(torch.float64)
                out[i:i + 16] += (sub @ grads[nm].T).numpy()
    return out * 2.0 ** -25


# ---- the tolerance ----------------------------------------------------------------------------------------------------------------------------------------
def head_of_logit(arch):
    return np.concatenate([np.full(c, h) for h, c in enumerate(HEAD_CLASSES[arch])])


def emulated_errors(sd, size, roundings=("fp16", "hilo"), positions=None):
    """{rounding: [n_heads]}: the largest relative error per head of forward64(rounding) against float64 on amplitude-1023 impulses at `positions` (default:
    sample_positions) of each input plane."""
    pos = sample_positions(size) if positions is None else positions
    arch = arch_of(size)
    ref, emu = Net64(sd), {r: Net64(sd, r) for r in roundings}
    hk = head_of_logit(arch)
    worst = {r: np.zeros(len(HEAD_CLASSES[arch])) for r in roundings}
    for plane in (0, 1):
        for i in range(0, len(pos), 64):
            x = preprocess(*impulses(size, plane, pos[i:i + 64]))
            a = forward64(ref, x)
            for r in roundings:
                rel = np.abs(forward64(emu[r], x) - a) / a
                for h in range(len(worst[r])):
                    worst[r][h] = max(worst[r][h], rel[:, hk == h].max())
    return worst


# |expected - C oracle| / expected as measured by tests/test_tracer_cpu.py (44 CUs per size), rounded up: the floor under RHO_EXACT is 8 x this
ORACLE_MEASURED = {128: 1.5e-6, 64: 1.5e-6, 32: 1.5e-6, 16: 1.5e-6}
# 8 x the emulation's largest relative error per head (tests/test_tracer_cpu.py recomputes them and holds the table to within 2 %)
RHO_FAST = {128: (8.359e-4, 9.662e-4, 1.1234e-3), 64: (8.359e-4, 1.0067e-3, 9.954e-4, 1.1752e-3),
            32: (8.359e-4, 1.0746e-3, 1.1295e-3, 1.6554e-3), 16: (8.457e-4, 9.019e-4, 1.3430e-3, 1.7075e-3)}
# (the deep heads' figures are the lo halves' underflow: an impulse's activations there are ~1e-4, their lo parts fp16 subnormals)
RHO_EXACT = {128: (1.2e-5, 4.649e-5, 5.597e-4), 64: (1.2e-5, 6.784e-5, 4.624e-4, 7.423e-4),
             32: (1.2e-5, 2.380e-5, 4.716e-5, 2.0806e-4), 16: (1.2e-5, 1.2e-5, 2.907e-5, 3.265e-5)}


def rho(size, exact):
    """Per-logit tolerance [K] of a size."""
    t = (RHO_EXACT if exact else RHO_FAST)[size]
    return np.asarray(t, np.float64)[head_of_logit(arch_of(size))]


if __name__ == "__main__":
    import time
    for size in (16, 32, 64, 128):
        t0 = time.time()
        e = emulated_errors(tracer_state_dict(arch_of(size)), size)
        print(size, "8 x fp16", [float(f"{8 * v:.3e}") for v in e["fp16"]], "8 x hilo", [float(f"{8 * v:.3e}") for v in e["hilo"]], f"{time.time() - t0:.1f} s", flush=True)
