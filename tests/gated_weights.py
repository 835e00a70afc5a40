"""Gated weights: the tracer weights (tests/tracer_weights.py) with a bias, a clipping ReLU and a non-trivial BatchNorm fold at every site where pooling dilutes.

The tracer and the shift weights make the network linear on purpose: BatchNorm is the identity, there is no bias, every weight is positive and no ReLU clips.  On
them the three things every kernel epilogue does besides the MFMA sum -- add the folded bias (and the shortcut's), add conv2 and the shortcut BEFORE the ReLU,
clamp at zero -- are no-ops.  This family makes each of them matter per pixel:

  gated_state_dict(arch, size)
      A site is a ReLU output, "layerL.B.conv1" or "layerL.B.out"; it is GATED when its map is at least 8 x 8 (all four stages of the 128 model, stages 0-2 of 64,
      0-1 of 32, stage 0 of 16 -- the state dict depends on the size, not on the architecture alone).  Ungated sites, the stem and the heads are the tracer's.
      At a gated site, per output channel c:
        scale     s = gamma / sqrt(var + eps) = sigma 2^e / sqrt(1 + eps), e seeded in {-2 .. 2}; var + eps = 4^v (1 + eps) with v seeded in {-1, 1} (pinned where e + v = 0),
                  gamma = sigma 2^(e + v): neither is 1.  The conv weight row is divided by 2^e (exactly): the folded |weight| is the tracer's to fp32 rounding.
        sign      sigma = -1 on a seeded quarter of the channels.  ".0" blocks: bn2 and the shortcut BN on the same channels (the channel is strongly negative in
                  front of the ReLU and comes out exactly 0); ".1" blocks: bn2 alone (the site sees -conv2 + identity).  conv1 sites: bn1.
        bias      folded bias t = beta - mean s with mean = -2 t / s and beta = -t (the `mean x scale` term is twice the result).  conv1 sites: t = -b;
                  ".0.out": bn2 +b and the shortcut -2 b (a dropped shortcut bias shows on every CU); ".1.out": -b.
        b         B[size][site], a committed constant: theta x the median positive pre-activation (without the bias) over the calibration impulses
                  (tw.sample_positions(size, 16, 32), both planes), found site by site in forward order by `calibrate` (`python tests/gated_weights.py`).
      The zero CU has every gated pre-activation equal to -b: its logits are exactly 0.0, and an impulse lights only its own cone.
  GatedNet / forward64
      tw.Net64 (BN folded in double) with the pre-activation spelled out, and three single-pixel mutation kinds beside the tracer's scale mutation:
      ("norelu", site, y, x) the ReLU skipped, ("nobias", site, y, x) the site's folded bias (conv2's and the shortcut's) skipped, ("relu_before_add", site, y, x)
      relu(conv2 + b2) + shortcut at an ".out" site.
  magnitude   M[cu, k] = the logit of the same CU under the tracer network (tw.expected with the tracer adjoint).  fp16 error is relative to what flows, not to
              what survives the gates: the metric is |device - forward64| <= rho_k M for every CU and logit.
  content     per size: the zero CU first and last, impulses of 1023 in each plane alone (16, 32: every pixel; 64: tw.subset_positions; 128: a 160-position set
              with the four corners, 48 ring positions and the input pixel under every mutated place), tw.ring_families, 32 dense CUs, tw.leakage_family cut to 136.

Tolerance: RHO_GATED_FAST / RHO_GATED_EXACT[size][head] = 8 x the largest |forward64(rounding) - forward64| / M over the impulse content ("fp16" / "hilo"), the
exact table not below 8 x GATED_ORACLE_MEASURED.  tests/test_gated_cpu.py recomputes both and holds the committed figures to 2 %.  No figure here comes from a
device run.  Of the package only synth and weights.pack_blob are used."""
import numpy as np

import tracer_weights as tw

SEED = 91
MIN_MAP = 8
NEG_SHARE = 4            # one channel in four gets gamma < 0
SIZES = (128, 64, 32, 16)
N_IMPULSE_128 = 160


def map_of(size, stage):
    return size >> (stage + 1)


def sites(arch):
    return [f"layer{s}.{b}.{w}" for s in range(len(tw.STAGE_PLANES[arch])) for b in range(2) for w in ("conv1", "out")]


def gated_sites(size):
    """The gated sites of a size in forward order."""
    return [s for s in sites(tw.arch_of(size)) if map_of(size, int(s[5])) >= MIN_MAP]


CAL = (16, 32)            # border and interior positions of the calibration sample (tw.sample_positions; the four corners come with it)
# theta per kind of site, (stages 0 and 1, stages 2 and 3): the 128 model's, and the small models'
THETA = {128: {"first": (0.7, 0.7), "0.conv1": (0.3, 0.12), "0.out": (0.3, 0.15), "1.conv1": (0.4, 0.15), "1.out": (0.75, 0.3)},
         64: {"first": (1.0, 1.0), "0.conv1": (0.5, 0.5), "0.out": (0.5, 0.5), "1.conv1": (0.5, 0.5), "1.out": (1.5, 1.5)}}
THETA[32] = THETA[16] = THETA[64]


def theta(site, size):
    """The share of the median positive pre-activation that the bias takes (THETA): 0.5, but 1 at the first site (the stem's cone is nine pixels of one level) and
    1.5 at the identity blocks' outputs (the identity shortcut keeps the median-based b small against what flows).  The 128 model takes about half of that, and a
    quarter from stage 2 on: its impulse set is one third border positions, an impulse's cone is the whole map there, and a median over all impulses puts out the
    weak ones -- those in the last rows and columns, which every stride-2 conv reads through one tap -- altogether (the cap on empty comparisons of
    tests/test_gated_cpu.py; with the small models' thetas 12 % of the 128 model's comparisons are empty)."""
    return THETA[size]["first" if site == "layer0.0.conv1" else site[7:]][int(site[5]) >= 2]


# b per (size, site): `python tests/gated_weights.py` prints this table (calibrate); tests/test_gated_cpu.py holds the conditions it was chosen for
B = {
    128: {'layer0.0.conv1': 0.02506, 'layer0.0.out': 0.00117, 'layer0.1.conv1': 0.0005228, 'layer0.1.out': 0.0009285, 'layer1.0.conv1': 0.0005308, 'layer1.0.out': 0.0003977, 'layer1.1.conv1': 0.0002627, 'layer1.1.out': 0.000343, 'layer2.0.conv1': 0.0001361, 'layer2.0.out': 8.334e-05, 'layer2.1.conv1': 4.685e-05, 'layer2.1.out': 6.186e-05, 'layer3.0.conv1': 5.155e-05, 'layer3.0.out': 4.412e-05, 'layer3.1.conv1': 3.536e-05, 'layer3.1.out': 5.888e-05},
    64: {'layer0.0.conv1': 0.02633, 'layer0.0.out': 0.001988, 'layer0.1.conv1': 0.0005787, 'layer0.1.out': 0.002023, 'layer1.0.conv1': 0.0007233, 'layer1.0.out': 0.000932, 'layer1.1.conv1': 0.00023, 'layer1.1.out': 0.0005119, 'layer2.0.conv1': 0.0004475, 'layer2.0.out': 0.0002791, 'layer2.1.conv1': 0.0001316, 'layer2.1.out': 0.0003024},
    32: {'layer0.0.conv1': 0.03504, 'layer0.0.out': 0.001552, 'layer0.1.conv1': 0.0005404, 'layer0.1.out': 0.002019, 'layer1.0.conv1': 0.0007908, 'layer1.0.out': 0.0009007, 'layer1.1.conv1': 0.0002248, 'layer1.1.out': 0.0006281},
    16: {'layer0.0.conv1': 0.0367, 'layer0.0.out': 0.001469, 'layer0.1.conv1': 0.00197, 'layer0.1.out': 0.002401},
}


def _channel_draws(size, site, c, salt=0):
    """(e, v, sigma) per output channel of a gated site (salt 1: the shortcut BN's own e and v)."""
    g = np.random.default_rng([SEED, size, sites(tw.arch_of(size)).index(site), salt])
    e = g.integers(-2, 3, size=c)
    v = np.where(g.integers(0, 2, size=c) == 0, -1, 1)
    v = np.where(e == 1, 1, np.where(e == -1, -1, v))              # e + v != 0: gamma is never 1
    neg = np.zeros(c, bool)
    neg[g.permutation(c)[:c // NEG_SHARE]] = True
    return e, v, np.where(neg, -1.0, 1.0)


def _set_bn(sd, bn, e, v, sigma, t):
    """BatchNorm `bn` with scale sigma 2^e and folded bias t (a scalar), from a gamma, a var, a mean and a beta that are all non-trivial."""
    var = (4.0 ** v * (1.0 + tw.BN_EPS) - tw.BN_EPS).astype(np.float32)          # sqrt(var + eps) = 2^v sqrt(1 + eps): the tracer's identity BN scales by 1 / sqrt(1 + eps) too
    gamma = (sigma * 2.0 ** (e + v)).astype(np.float32)
    s = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + tw.BN_EPS)
    sd[bn + ".running_var"][...] = var
    sd[bn + ".weight"][...] = gamma
    sd[bn + ".running_mean"][...] = (-2.0 * t / s).astype(np.float32)
    sd[bn + ".bias"][...] = np.float32(-t)


def gated_state_dict(arch, size=None, b=None):
    """b: {site: b} (default: the committed B[size]); a gated site missing from it gets b = 0 (calibrate)."""
    size = (128 if arch == 0 else 64) if size is None else size
    assert tw.arch_of(size) == arch
    b = B[size] if b is None else b
    sd = tw.tracer_state_dict(arch)
    for site in gated_sites(size):
        p, which = site.rsplit(".", 1)
        bs = float(b.get(site, 0.0))
        c = sd[p + ".conv1.weight"].shape[0]
        e, v, sigma = _channel_draws(size, site, c)
        row = (2.0 ** -e).astype(np.float32)[:, None, None, None]
        if which == "conv1":
            sd[p + ".conv1.weight"] *= row
            _set_bn(sd, p + ".bn1", e, v, sigma, -bs)
        else:
            sd[p + ".conv2.weight"] *= row
            if p.endswith(".0"):
                _set_bn(sd, p + ".bn2", e, v, sigma, +bs)
                e2, v2, _ = _channel_draws(size, site, c, 1)          # the shortcut BN: its own scale and var, bn2's sign
                sd[p + ".shortcut.0.weight"] *= (2.0 ** -e2).astype(np.float32)[:, None, None, None]
                _set_bn(sd, p + ".shortcut.1", e2, v2, sigma, -2.0 * bs)
            else:
                _set_bn(sd, p + ".bn2", e, v, sigma, -bs)
    return sd


def gated_blob(size):
    arch = tw.arch_of(size)
    return tw._pkg().weights.pack_blob(arch, gated_state_dict(arch, size))


# ---- the network in float64 ----------------------------------------------------------------------------------------------------------------------------
KINDS = ("norelu", "nobias", "relu_before_add")


class GatedNet(tw.Net64):
    """tw.Net64 with every site's pre-activation spelled out.  mutation: (site, y, x, factor) as in tw.Net64, or (kind, site, y, x) with kind in KINDS."""

    def forward(self, x, poc=None, qp=None, mutation=None, keep=None, pre=None):
        """keep: receives every site's activation; pre: receives per site (pre-activation without any bias, the site's total bias [C])."""
        import torch
        import torch.nn.functional as F
        n = x.shape[0]
        kind = mutation[0] if mutation is not None and mutation[0] in KINDS else None
        scale = mutation if mutation is not None and kind is None else None

        def site(name, lin, bias, before=None):
            """lin: the sum of the convs without bias; bias [C]: the site's folded bias; before = (u, b2, shortcut with its bias) at an ".out" site."""
            hit = torch.zeros(lin.shape[2:], dtype=torch.bool)
            if kind is not None and mutation[1] == name:
                hit[mutation[2], mutation[3]] = True
            if pre is not None:
                pre[name] = (lin, bias)
            bmap = bias[None, :, None, None] * (~(hit & (kind == "nobias"))).to(lin.dtype)
            z = lin + bmap
            t = F.relu(z)
            if kind == "norelu":
                t = torch.where(hit, z, t)
            elif kind == "relu_before_add" and mutation[1] == name:
                assert before is not None, "relu_before_add is a mutation of an .out site"
                u, b2, sc = before
                t = torch.where(hit, F.relu(u + b2[None, :, None, None]) + sc, t)
            if scale is not None and scale[0] == name:
                m = torch.ones(t.shape[2:], dtype=t.dtype)
                m[scale[1], scale[2]] = scale[3]
                t = t * m
            t = tw._rnd(t, self.rounding)
            if keep is not None:
                keep[name] = t
            return t

        cur = F.conv2d(x, self.stem, padding=1)
        if scale is not None and scale[0] == "stem":
            m = torch.ones(cur.shape[2:], dtype=cur.dtype)
            m[scale[1], scale[2]] = scale[3]
            cur = cur * m
        cur = tw._rnd(cur, self.rounding)
        if keep is not None:
            keep["stem"] = cur
        extra = torch.zeros((n, 2), dtype=torch.float64)
        if poc is not None:
            extra = torch.stack([torch.as_tensor(np.asarray(poc, np.float64)), torch.as_tensor(np.asarray(qp, np.float64))], dim=1)
        outs = []
        for i, (p, stride, (w1, b1), (w2, b2), sc) in enumerate(self.blocks):
            t = site(p + ".conv1", F.conv2d(cur, w1, None, stride=stride, padding=1), b1)
            u = F.conv2d(t, w2, None, padding=1)
            if sc is not None:
                short, bsc = F.conv2d(cur, sc[0], None, stride=stride), sc[1]
            else:
                short, bsc = cur, torch.zeros_like(b2)
            cur = site(p + ".out", u + short, b2 + bsc, before=(u, b2, short + bsc[None, :, None, None]))
            if i % 2 == 1 and i >= 3:
                w, b = self.heads[i // 2 - 1]
                outs.append(F.linear(torch.cat([cur.mean(dim=(2, 3)), extra], dim=1), w, b))
        return torch.cat(outs, dim=1)


def forward64(sd, x, rounding=None, mutation=None, chunk=32):
    """x: float64 [n, 2, S, S] (numpy) -> logits float64 [n, K] (numpy)."""
    import torch
    net = sd if isinstance(sd, GatedNet) else GatedNet(sd, rounding)
    x = np.asarray(x, np.float64)
    with torch.no_grad():
        return np.concatenate([net.forward(torch.from_numpy(x[i:i + chunk]), mutation=mutation).numpy() for i in range(0, len(x), chunk)])


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------------------------
# tw._MUT_128 has no ".0.out" site -- the one place where conv2's bias (+b) and the shortcut's (-2 b) meet: two more places, mapped to the size like the others
EXTRA_128 = [("layer0.0.out", 2, (40, 7)), ("layer1.0.out", 4, (9, 21))]


def places(size):
    """[(site, y, x)]: the places of tw._MUT_128 that are gated sites of this size, on its own maps, and the two ".0.out" places of EXTRA_128."""
    gs = set(gated_sites(size))
    out = [(m[0], m[1], m[2]) for _, m in tw.mutations(size) if m[0] in gs]
    for site, div, (y, x) in EXTRA_128:
        if site in gs:
            m = size // div
            out.append((site, y * m // (128 // div), x * m // (128 // div)))
    return out


def mutations(size):
    """[(name, (kind, site, y, x))]: three kinds x the gated places (relu_before_add at ".out" sites only)."""
    return [(f"{kind} at {site} pixel ({y},{x})", (kind, site, y, x)) for site, y, x in places(size) for kind in KINDS
            if kind != "relu_before_add" or site.endswith(".out")]


# (kind, site) pairs whose float64 mutated network stays within 2 x rho_fast x M of the float64 network at every CU that is looked at, with the largest multiple
# that tests/test_gated_cpu.py measures (it holds this table: a pair listed here does not reach 2, every other pair does).  docs/NUMERICS.md says why.
UNSEEN = {128: {("nobias", "layer2.1.out"): 1.95, ("relu_before_add", "layer2.1.out"): 1.40, ("norelu", "layer1.1.out"): 1.39, ("nobias", "layer1.1.out"): 1.24,
                ("relu_before_add", "layer1.1.out"): 1.93, ("nobias", "layer0.1.out"): 1.91, ("norelu", "layer3.1.out"): 0.37, ("nobias", "layer3.1.out"): 0.18,
                ("relu_before_add", "layer3.1.out"): 1.23, ("norelu", "layer2.1.conv1"): 1.33, ("nobias", "layer2.1.conv1"): 0.06, ("nobias", "layer0.0.out"): 1.99,
                ("nobias", "layer1.0.out"): 1.72},
          64: {("nobias", "layer2.1.conv1"): 0.33}, 32: {}, 16: {}}


def seen_mutations(size):
    """mutations(size) without the pairs of UNSEEN: what tests/test_gated_gpu.py asks the device's results to tell from the network."""
    return [(n, m) for n, m in mutations(size) if (m[0], m[1]) not in UNSEEN[size]]


def anchor(size, site, y, x):
    """Flat input position under the centre of output pixel (y, x) of `site`."""
    f = size // map_of(size, int(site[5]))
    return min(y * f + f // 2, size - 1) * size + min(x * f + f // 2, size - 1)


# ---- content -------------------------------------------------------------------------------------------------------------------------------------------------
def impulse_positions(size):
    if size <= 32:
        return np.arange(size * size)
    if size == 64:
        return np.union1d(tw.subset_positions(64), [anchor(64, *p) for p in places(64)])
    fixed = np.unique(np.concatenate([tw.sample_positions(128, 48, 0)[:52], [anchor(128, *p) for p in places(128)]]))
    rest = np.setdiff1d(np.random.default_rng([128, SEED]).permutation(128 * 128), fixed, assume_unique=True)[:N_IMPULSE_128 - len(fixed)]
    return np.sort(np.concatenate([fixed, rest]))


def impulse_content(size):
    """-> labels, org, pred of the impulse CUs alone (what the tolerance is derived on)."""
    pos = impulse_positions(size)
    parts = [tw.impulses(size, plane, pos) for plane in (0, 1)]
    labels = [f"impulse plane {plane} ({q // size},{q % size})" for plane in (0, 1) for q in pos]
    return labels, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def content(size):
    """-> labels [n], org, pred int16 [n, S, S], is_zero [n], is_impulse [n]."""
    il, io, ip = impulse_content(size)
    rl, ro, rp = tw.ring_families(size)
    do, dp = tw._pkg().synth.make_patches_bulk(size, 32, 32)
    lo, lp, lz = tw.leakage_family(size, 136, 8)
    z = np.zeros((1, size, size), np.int16)
    labels = ["zero CU (first)"] + il + rl + [f"dense {i}" for i in range(32)] + [f"leakage {i} ({'zero' if q else 'bright'})" for i, q in enumerate(lz)] + ["zero CU (last)"]
    org = np.concatenate([z, io, ro, do, lo, z])
    pred = np.concatenate([z, ip, rp, dp, lp, z])
    is_zero = np.concatenate([[True], np.zeros(len(il) + len(rl) + 32, bool), lz, [True]])
    is_imp = np.zeros(len(org), bool)
    is_imp[1:1 + len(il)] = True
    assert len(labels) == len(org) == len(is_zero) and int(is_zero.sum()) == 12
    return labels, org, pred, is_zero, is_imp


def unique_rows(org, pred):
    """(first, inverse): the CUs at `first` are the distinct ones, row i equals row first[inverse[i]] (the leakage family repeats one CU 126 times)."""
    seen, first, inv = {}, [], np.empty(len(org), np.int64)
    for i in range(len(org)):
        k = (org[i].tobytes(), pred[i].tobytes())
        if k not in seen:
            seen[k] = len(first)
            first.append(i)
        inv[i] = seen[k]
    return np.asarray(first), inv


def reference(size, org, pred, rounding=None, mutation=None, sd=None):
    """forward64 of the gated set on the distinct CUs of (org, pred), spread back.  float64 [n, K]."""
    sd = gated_state_dict(tw.arch_of(size), size) if sd is None else sd
    first, inv = unique_rows(org, pred)
    return forward64(sd, tw.preprocess(org[first], pred[first]), rounding, mutation)[inv]


_G = {}


def magnitude(size, org, pred):
    """M [n, K]: the tracer network's logits of the same CUs."""
    if size not in _G:
        _G[size] = tw.adjoint(tw.tracer_state_dict(tw.arch_of(size)), size)
    return tw.expected(_G[size], org, pred)


def mutation_cus(size, mut, labels, org, is_zero, is_imp):
    """Indices into the content that a mutation is looked for at: the impulses nearest to the input pixel under the mutated place (all of them for 16; 96 CUs
    for 32 and 64, 32 for 128), the ring and its complement, the full rows and columns within 8 pixels of that input pixel, four dense CUs and the first zero CU."""
    idx = np.flatnonzero(is_imp)
    a = anchor(size, *mut[1:])
    ay, ax = a // size, a % size
    if size > 16:
        at = np.array([tuple(int(t) for t in labels[i].split("(")[1].rstrip(")").split(",")) for i in idx])
        d = np.abs(at[:, 0] - ay) + np.abs(at[:, 1] - ax)
        idx = idx[np.argsort(d, kind="stable")[:32 if size == 128 else 96]]
    near = lambda l: abs(int(l.split()[1]) - (ay if l.startswith("row") else ax)) <= 8
    fam = [i for i, l in enumerate(labels) if l.startswith(("ring", "all but")) or l.startswith(("row", "column")) and near(l)]
    dense = [i for i, l in enumerate(labels) if l.startswith("dense")][:4]
    return np.concatenate([[0], idx, fam, dense]).astype(np.int64)


# ---- conditions -------------------------------------------------------------------------------------------------------------------------------------------
def site_statistics(sd, x, names, chunk=16):
    """Per site of `names` over the content x: (median positive pre-activation without the bias, share of the light cone -- entries positive without the bias --
    that the bias clips)."""
    import torch
    net = GatedNet(sd)
    pos = {nm: [] for nm in names}
    cone = {nm: 0 for nm in names}
    clipped = {nm: 0 for nm in names}
    with torch.no_grad():
        for i in range(0, len(x), chunk):
            pre = {}
            net.forward(torch.from_numpy(np.asarray(x[i:i + chunk], np.float64)), pre=pre)
            for nm in names:
                lin, bias = pre[nm]
                lit = lin > 0
                pos[nm].append(lin[lit].numpy())
                cone[nm] += int(lit.sum())
                clipped[nm] += int((lit & (lin + bias[None, :, None, None] <= 0)).sum())
    return {nm: (float(np.median(np.concatenate(pos[nm]))) if cone[nm] else 0.0, clipped[nm] / max(cone[nm], 1)) for nm in names}


def calibration_input(size):
    pos = tw.sample_positions(size, *CAL)
    return np.concatenate([tw.preprocess(*tw.impulses(size, plane, pos)) for plane in (0, 1)])


def calibrate(size):
    """{site: b}: site by site in forward order, theta x the median positive pre-activation over the calibration impulses with every earlier b in place."""
    arch = tw.arch_of(size)
    x = calibration_input(size)
    b = {}
    for site in gated_sites(size):
        med, _ = site_statistics(gated_state_dict(arch, size, b), x, [site])[site]
        b[site] = float(f"{theta(site, size) * med:.4g}")
    return b


def head_errors(err, M, size):
    """Largest |err| / M per head over the CUs."""
    hk = tw.head_of_logit(tw.arch_of(size))
    rel = np.abs(err) / M
    return np.array([rel[:, hk == h].max() for h in range(hk.max() + 1)])


def emulated_errors(size, roundings=("fp16", "hilo")):
    """{rounding: [n_heads]}: the largest |forward64(rounding) - forward64| / M per head over the impulse content."""
    _, org, pred = impulse_content(size)
    M = magnitude(size, org, pred)
    ref = reference(size, org, pred)
    return {r: head_errors(reference(size, org, pred, r) - ref, M, size) for r in roundings}


# |forward64 - C oracle| / M as measured by tests/test_gated_cpu.py (44 CUs per size), rounded up: the floor under RHO_GATED_EXACT is 8 x this
GATED_ORACLE_MEASURED = {128: 1.0e-7, 64: 1.0e-7, 32: 2.0e-7, 16: 3.0e-7}
RHO_GATED_FAST = {128: (0.0002455, 0.0002244, 0.0001507), 64: (0.0001649, 0.0001565, 0.0001778, 0.0001955), 32: (0.000171, 0.0002364, 0.0003066, 0.0002751), 16: (0.0003981, 0.0005402, 0.0003964, 0.0004958)}
RHO_GATED_EXACT = {128: (1.583e-05, 1.368e-06, 1.839e-06), 64: (1.06e-06, 2.393e-06, 1.267e-05, 5.991e-05), 32: (1.6e-06, 2.857e-05, 0.0002988, 0.0005973), 16: (5.826e-06, 9.671e-06, 2.487e-05, 3.78e-05)}


def rho(size, exact):
    t = (RHO_GATED_EXACT if exact else RHO_GATED_FAST)[size]
    return np.asarray(t, np.float64)[tw.head_of_logit(tw.arch_of(size))]


if __name__ == "__main__":
    import sys
    import time
    for size in [int(a) for a in sys.argv[1:]] or SIZES[::-1]:
        t0 = time.time()
        if size not in B:
            B[size] = calibrate(size)
        print(f"    {size}: {B[size]},", f"# {time.time() - t0:.1f} s", flush=True)
        e = emulated_errors(size)
        print(size, "8 x fp16", [float(f"{8 * v:.3e}") for v in e["fp16"]], "8 x hilo", [float(f"{8 * v:.3e}") for v in e["hilo"]], f"{time.time() - t0:.1f} s", flush=True)
