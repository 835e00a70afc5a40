"""Designed decision heads: weight blobs whose head logits are known bit for bit, and the selection rules restated on one CU.

The head is logits_k = W_k . [feat, poc, qp] + b_k in fp32 (include/mltcnn.h; csrc/mlt_tail_kernels.inc), poc and qp per-CU integers.  A head whose FEATURE
columns are +0.0 gives logits that depend on (poc, qp, bias) alone: fl32(fl32(a_k * f32(poc)) + fl32(c_k * f32(qp))) + b_k.  With dyadic coefficients every
step is exact, so the fast and the exact arithmetic, the CPU oracle and this module agree on every bit (`designed_logits` asserts the exactness against
float64; the one exception are the deliberate |poc|, |qp| >= 2^24 cases, where int -> float rounds and the expected operand is np.float32(poc)).

  designed_blob     the seeded state dict with one head (or several: designed_blob_multi) replaced by (a, c, b); the other heads keep their seeded weights, so
                    an exact re-run of a CU stays visible in THEIR bytes
  designed_logits   the prediction
  arrangements      one (poc, qp) per weak order (ranking with ties) of the K logits that a grid of integer points reaches
  decide / candidates / guard_flags
                    the records and the three float-valued guard rules on ONE CU's decision-head logits in np.float32 scalars, written from the text of
                    include/mltcnn.h (mlt_decision, mlt_candidates, mlt_set_confidence_gate, mlt_set_candidate_policy, mlt_config.flags) -- nothing of the
                    package and nothing of the kernel is called.  A NaN flags in every rule.

Threshold families for the guards (`margin_family`, `gap_family`): logits in which the decision head's top-2 margin, or the gap between the last kept and the
first dropped class, is EXACTLY T, T (1 - 2^-24) (one fp32 step below), T + 2^-20, 0 or large, chosen per CU by small (poc, qp) -- small, so that the OTHER
heads' logits stay of order 1 .. 500 and the fast and the exact arithmetic remain distinguishable in their bytes."""
import numpy as np

F = np.float32
STAGE_PLANES = {0: (32, 64, 128, 256), 1: (32, 64, 96, 128, 256)}
HEAD_CLASSES = {0: (2, 3, 4), 1: (2, 3, 4, 6)}
CONF_BAND_FRAC = F(0.75)     # mltcnn.h: "within 0.75 x tolerance of the threshold" (gate guard, candidate guard (a))
FAR = F(-200.0)              # expf(-200) is 0 in fp32 and adding it leaves a float64 sum >= 1 unchanged as well


def _pkg():
    import mltcnn_pkg
    return mltcnn_pkg.load()


def feature_width(arch, head):
    return STAGE_PLANES[arch][head + 1]


def arch_of(size):
    return 0 if size == 128 else 1


def head_offset(arch, head):
    return sum(HEAD_CLASSES[arch][:head])


# ---- blobs ---------------------------------------------------------------------------------------------------------------------------------------------
def designed_blob_multi(arch, seed, designs, keep_other_heads=True):
    """designs: {head: (a, c, b)}, each of length K(head).  keep_other_heads=False: every head not designed gets all-zero weights and bias."""
    pkg = _pkg()
    sd = {k: np.array(v, copy=True) for k, v in pkg.synth.make_state_dict(arch, seed).items()}
    for head, K in enumerate(HEAD_CLASSES[arch]):
        w, bias = sd[f"branch{head + 1}.weight"], sd[f"branch{head + 1}.bias"]
        C = feature_width(arch, head)
        assert w.shape == (K, C + 2) and bias.shape == (K,)
        if head in designs:
            a, c, b = (np.asarray(v, F) for v in designs[head])
            assert a.shape == c.shape == b.shape == (K,), (head, a.shape, K)
            w[:, :C] = F(0.0)
            w[:, C], w[:, C + 1], bias[:] = a, c, b
        elif not keep_other_heads:
            w[:], bias[:] = F(0.0), F(0.0)
    return pkg.weights.pack_blob(arch, sd)


def designed_blob(arch, seed, head, a, c, b, keep_other_heads=True):
    return designed_blob_multi(arch, seed, {head: (a, c, b)}, keep_other_heads)


def designed_logits(a, c, b, poc, qp):
    """[n, K] float32: fl32(fl32(a * f32(poc)) + fl32(c * f32(qp))) + b, every intermediate asserted exact against float64 (NaN / inf coefficients pass through;
    |poc|, |qp| >= 2^24 may round in the int -> float conversion and nowhere else)."""
    a, c, b = (np.asarray(v, F) for v in (a, c, b))
    poc, qp = np.atleast_1d(np.asarray(poc, np.int64)), np.atleast_1d(np.asarray(qp, np.int64))
    assert poc.shape == qp.shape and poc.ndim == 1 and np.abs(poc).max() < 2 ** 31 and np.abs(qp).max() < 2 ** 31
    fp, fq = poc.astype(np.int32).astype(F), qp.astype(np.int32).astype(F)
    for v, f in ((poc, fp), (qp, fq)):
        small = np.abs(v) < 2 ** 24
        assert (f[small].astype(np.int64) == v[small]).all()
    with np.errstate(invalid="ignore", over="ignore"):
        zero = F(0.0)
        p = fp[:, None] * a[None, :] + zero          # (the kernel's fmaf(w, f, +0): a product of -0 becomes +0)
        q = fq[:, None] * c[None, :] + zero
        s = p + q
        out = s + b[None, :]
        p64 = fp[:, None].astype(np.float64) * a[None, :].astype(np.float64)
        q64 = fq[:, None].astype(np.float64) * c[None, :].astype(np.float64)
        s64 = p64 + q64
        o64 = s64 + b[None, :].astype(np.float64)
    fin = np.isfinite(o64)
    for got, want in ((p, p64), (q, q64), (s, s64), (out, o64)):
        assert (got.astype(np.float64)[fin] == want[fin]).all(), "a designed logit is not exact in fp32"
    assert out.dtype == F
    return out


# ---- designs for the byte checks (oracle, device) --------------------------------------------------------------------------------------------------
BIG = 2 ** 24
# (poc, qp): small, negative, zero, and the cases in which int -> float rounds (2^24 + 1 -> 2^24, -(2^24 + 3) -> -(2^24 + 4))
SCALARS = [(0, 0), (1, 0), (0, 1), (-1, -1), (37, -22), (-48, 48), (600, 47), (-600, 17), (BIG + 1, 3), (5, -(BIG + 3)), (BIG + 1, -(BIG + 3)), (-(BIG + 1), BIG + 2)]


def sixteenths(K, seed):
    g = np.random.default_rng([99, K, seed])
    return tuple((g.integers(-128, 129, K) / 16.0).astype(F) for _ in range(3))


def one_sided(K, seed):
    """A design that stays exact at |poc|, |qp| ~ 2^24: per class ONE of the two slopes, +-2^e with e in -3 .. 0, and an even bias."""
    g = np.random.default_rng([98, K, seed])
    slope = (np.ldexp(1.0, g.integers(-3, 1, K)) * g.choice([-1.0, 1.0], K)).astype(F)
    on_poc = (np.arange(K) + seed) % 2 == 0
    return np.where(on_poc, slope, 0).astype(F), np.where(on_poc, 0, slope).astype(F), (2 * g.integers(-20, 21, K)).astype(F)


# ---- weak orders -----------------------------------------------------------------------------------------------------------------------------------------
def signature(l):
    """Weak order of K logits: per class the number of classes with a larger logit (ties share a rank); [..., K] -> tuple(s) of ints."""
    l = np.asarray(l)
    r = (l[..., None, :] > l[..., :, None]).sum(-1)
    return tuple(int(v) for v in r) if r.ndim == 1 else r


def is_strict(sig):
    return len(set(sig)) == len(sig)


def arrangements(a, c, b, grid=48, limit=64.0):
    """{weak-order signature: (poc, qp)} over the integer points |poc|, |qp| <= grid whose K logits all have |logit| <= limit; per signature the point nearest
    the origin (then the smallest poc, qp)."""
    g = np.arange(-grid, grid + 1)
    poc, qp = (v.reshape(-1) for v in np.meshgrid(g, g, indexing="ij"))
    order = np.lexsort((qp, poc, np.abs(poc) + np.abs(qp)))
    poc, qp = poc[order], qp[order]
    l = designed_logits(a, c, b, poc, qp)
    ok = (np.abs(l) <= limit).all(axis=1)
    poc, qp, l = poc[ok], qp[ok], l[ok]
    K = l.shape[1]
    sig = signature(l)
    code = (sig * (K ** np.arange(K))[None, :]).sum(axis=1)
    _, first = np.unique(code, return_index=True)
    return {tuple(int(v) for v in sig[i]): (int(poc[i]), int(qp[i])) for i in sorted(first)}


def random_design(K, seed, coef=8, bias=40, step=16):
    """Coefficients: multiples of 1 / step in [-coef, coef]; bias: integers in [-bias, bias] (so that ties fall on grid points often)."""
    g = np.random.default_rng([K, seed])
    a = g.integers(-coef * step, coef * step + 1, K).astype(F) / F(step)
    c = g.integers(-coef * step, coef * step + 1, K).astype(F) / F(step)
    b = g.integers(-bias, bias + 1, K).astype(F)
    return a, c, b


# (seed, coef, bias, step) of random_design per K, at most 8 per K; tests/test_designed_heads_cpu.py asserts the orders they reach together.
# Unit-size slopes let the whole grid in under the |logit| <= 64 limit; integer and half-integer coefficients put grid points ON the tie lines and their crossings.
DESIGNS = {
    2: [(0, 1, 4, 1), (1, 1, 4, 1)],
    3: [(1, 1, 4, 1), (0, 1, 4, 1)],
    4: [(25, 1, 24, 1), (32, 1, 10, 2), (15, 1, 4, 1), (5, 1, 4, 1)],
    6: [(37, 1, 10, 2), (39, 1, 24, 2), (35, 1, 24, 1), (26, 1, 10, 2), (22, 1, 10, 2), (18, 1, 24, 2), (17, 1, 10, 4), (28, 1, 4, 2)],
}
_CASES = {}


def case_set(K):
    """The case set of a K-class head: per design of DESIGNS[K] its coefficients and arrangement representatives -> [((a, c, b), [(signature, poc, qp)])]."""
    if K not in _CASES:
        out = []
        for seed, coef, bias, step in DESIGNS[K]:
            a, c, b = random_design(K, seed, coef=coef, bias=bias, step=step)
            out.append(((a, c, b), [(s, p, q) for s, (p, q) in arrangements(a, c, b).items()]))
        _CASES[K] = out
    return _CASES[K]


# ---- the records and the guards on one CU, np.float32 scalars, from the header's text ---------------------------------------------------------------------
def _f(l):
    return [F(v) for v in l]


def decide(l, min_conf=0.0):
    """mlt_decision of one head: raw_mode = first maximal index; confidence = softmax probability of raw_mode (fp32, max-subtracted, summed in class order);
    margin = top-1 minus top-2 logit; split_mode = confidence >= min_conf ? raw_mode : -1 (a NaN confidence gates).  A row with a NaN has a NaN confidence and a
    NaN margin; its raw_mode is left to the scan (mltcnn.h defines the argmax for comparable logits) and is None here."""
    l = _f(l)
    K = len(l)
    if any(v != v for v in l):
        return {"raw_mode": None, "confidence": F(np.nan), "margin": F(np.nan), "split_mode": None if not min_conf > 0 else -1}
    best = 0
    for k in range(1, K):
        if l[k] > l[best]:
            best = k
    s = F(0.0)
    with np.errstate(under="ignore"):
        for k in range(K):
            s = F(s + np.exp(F(l[k] - l[best]), dtype=F))
    conf = F(F(1.0) / s)
    srt = sorted(l, reverse=True)
    margin = F(srt[0] - srt[1])
    split = best if not (min_conf > 0) or conf >= F(min_conf) else -1
    return {"raw_mode": best, "confidence": conf, "margin": margin, "split_mode": split}


def candidates(l, coverage=0.0, max_modes=0, prob=None):
    """mlt_candidates of one head, steps 1 .. 7 of the header.  prob: the record's probabilities (class order) in place of the restated softmax -- the prefix
    sums are then the device's own to the bit (fp32 additions in rank order).  -> order, prob, cum, n, count, mask, gap (last kept minus first dropped logit;
    None when nothing is dropped), nan."""
    l = _f(l)
    K = len(l)
    nan = any(v != v for v in l)
    order = list(range(K)) if nan else sorted(range(K), key=lambda k: (-float(l[k]), k))     # stable, descending, equal logits in class order
    if prob is None:
        with np.errstate(under="ignore", invalid="ignore"):
            e = [np.exp(F(l[k] - l[order[0]]), dtype=F) for k in range(K)]
            s = F(0.0)
            for k in range(K):
                s = F(s + e[k])
            prob = [F(e[k] / s) for k in range(K)]
    else:
        prob = _f(prob[:K])
    cum, run, n = [], F(0.0), K
    found = False
    with np.errstate(invalid="ignore"):
        for r in range(K):
            run = F(run + prob[order[r]])
            cum.append(run)
            if not found and run >= F(coverage):
                n, found = r + 1, True
    count = K if nan or (max_modes > 0 and n > max_modes) else n
    mask = 0
    for r in range(count):
        mask |= 1 << order[r]
    gap = F(l[order[count - 1]] - l[order[count]]) if count < K else None
    return {"order": order, "prob": prob, "cum": cum, "n": n, "count": count, "mask": mask, "gap": gap, "nan": nan}


def guard_flags(l, guard_margin, tolerance, min_conf=0.0, coverage=0.0, max_modes=0, confidence=None, prob=None):
    """Which of the float-valued guards select the CU for the exact re-run (a size that runs a non-exact tier with the decision guard on):
      decision   not (top1 - top2 >= guard_margin)
      gate       a gate is set and not (|confidence - min_conf| >= 0.75 x tolerance); confidence: the record's (default: the restated one)
      cand_a     a policy other than (0, 0) is set and a proper prefix sum is not at least 0.75 x tolerance away from the coverage
      cand_b     ... and classes are dropped over a logit gap that is not >= guard_margin
    Every comparison is written so that a NaN flags.  -> dict of bools + "any"."""
    d = decide(l)
    T, band = F(guard_margin), F(CONF_BAND_FRAC * F(tolerance))
    out = {"decision": not (d["margin"] >= T), "gate": False, "cand_a": False, "cand_b": False}
    if min_conf > 0:
        conf = d["confidence"] if confidence is None else F(confidence)
        out["gate"] = not (np.abs(F(conf - F(min_conf))) >= band)
    if coverage > 0 or max_modes > 0:
        c = candidates(l, coverage, max_modes, prob)
        K = len(c["order"])
        with np.errstate(invalid="ignore"):
            out["cand_a"] = any(not (np.abs(F(c["cum"][r] - F(coverage))) >= band) for r in range(K - 1))
        out["cand_b"] = c["gap"] is not None and not (c["gap"] >= T)
    out["any"] = any(out.values())
    return out


# ---- threshold families -------------------------------------------------------------------------------------------------------------------------------------
def _place(K, classes, rows):
    a, c, b = np.zeros(K, F), np.zeros(K, F), np.full(K, FAR, F)
    for k, (ak, ck, bk) in zip(classes, rows):
        a[k], c[k], b[k] = ak, ck, bk
    return a, c, b


def margin_family(K, T, p, q):
    """l_p = T * qp - 2^-32 * poc, l_q = 0, the other classes 200 below.  -> ((a, c, b), {name: (poc, qp, top-2 margin)})."""
    T = F(T)
    eps = F(2.0 ** -32)
    assert T == F(2.0 ** -8), "the cases below are worked out for T = 2^-8: T (1 - 2^-24) = T - 2^-32, T + 2^-20 = T + 4096 x 2^-32"
    design = _place(K, (p, q), ((-eps, T, 0.0), (0.0, 0.0, 0.0)))
    cases = {
        "T": (0, 1, T),                                  # the margin IS the threshold: kept
        "T-": (1, 1, F(T - eps)),                        # one fp32 step below: re-run
        "T+": (-4096, 1, F(T + F(2.0 ** -20))),
        "zero": (0, 0, F(0.0)),                          # a tie
        "large": (0, 1024, F(4.0)),
        "T other way": (0, -1, T),                       # class q on top
        "T- other way": (-1, -1, F(T - eps)),
        "sure": (0, 51200, F(200.0)),                    # confidence exactly 1
        "one": (0, 256, F(1.0)),                         # confidence 1 / (1 + e^-1): no special value
    }
    return design, cases


def gap_family(K, T, p, q, r):
    """K >= 3: l_p = 1, l_q = 0, l_r = -(T * qp - 2^-32 * poc), the others 200 below; under a policy that keeps two classes the dropped-class gap is |l_q - l_r|.
    -> ((a, c, b), {name: (poc, qp, gap)})."""
    T = F(T)
    eps = F(2.0 ** -32)
    assert K >= 3 and T == F(2.0 ** -8)
    design = _place(K, (p, q, r), ((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), (eps, -T, 0.0)))
    cases = {
        "T": (0, 1, T),
        "T-": (1, 1, F(T - eps)),
        "T+": (-4096, 1, F(T + F(2.0 ** -20))),
        "zero": (0, 0, F(0.0)),
        "large": (0, 64, F(0.25)),
        "T other way": (0, -1, T),                       # class r second, class q dropped
        "T- other way": (-1, -1, F(T - eps)),
    }
    return design, cases
