"""Host restatement of the device's decision records (include/mltcnn.h: mlt_decision), in float64.

`from_logits` turns an [n, num_logits] array of head logits (lvl1..lvlN concatenated, as every entry point returns them) into the records
heads_kernel writes: per head the first-max argmax (torch.argmax) and its softmax probability, the decision head's top-2 margin, and the
confidence gate.  It is what the tests compare the device against, the way synth.flat_quad_fraction restates the flat statistic, and what
tools/confidence_sweep.py evaluates on a call dump.

`candidates_from_logits` restates the candidate records (include/mltcnn.h: mlt_candidates) the same way: rank, softmax, prefix sums, kept count, cap, mask,
with the device's tie and NaN rules; tools/candidate_sweep.py evaluates it on a call dump."""
from __future__ import annotations

import numpy as np

HEAD_CLASSES = {128: (2, 3, 4), 64: (2, 3, 4, 6), 32: (2, 3, 4, 6), 16: (2, 3, 4, 6)}
# float64 twin of capi.DECISION_DTYPE (same field names and shapes)
DTYPE = np.dtype([("split_mode", "<i4"), ("raw_mode", "<i4"), ("confidence", "<f8"), ("margin", "<f8"),
                  ("level_mode", "<i4", (4,)), ("level_conf", "<f8", (4,))])


def default_head(size: int) -> int:
    """The reference's decision head: element [2] for the 128 model, [0] otherwise (EncCu.cpp:913-919)."""
    return 2 if size == 128 else 0


def from_logits(size: int, logits, head_index: int | None = None, min_confidence: float = 0.0) -> np.ndarray:
    classes = HEAD_CLASSES[size]
    lg = np.asarray(logits, np.float64)
    if lg.ndim == 1:
        lg = lg[None, :]
    assert lg.ndim == 2 and lg.shape[1] == sum(classes), (lg.shape, classes)
    dh = default_head(size) if head_index is None or head_index < 0 else head_index
    assert 0 <= dh < len(classes)
    out = np.zeros((lg.shape[0],), DTYPE)
    out["level_mode"] = -1
    rows = np.arange(lg.shape[0])
    lo = 0
    for h, k in enumerate(classes):
        l = lg[:, lo:lo + k]
        lo += k
        best = np.argmax(l, axis=1)   # first maximal index
        e = np.exp(l - l[rows, best][:, None])
        s = np.zeros(lg.shape[0])
        for c in range(k):            # class order, like the device
            s = s + e[:, c]
        out["level_mode"][:, h] = best
        out["level_conf"][:, h] = 1.0 / s
        if h == dh:
            top = np.sort(l, axis=1)
            out["raw_mode"] = best
            out["confidence"] = 1.0 / s
            out["margin"] = top[:, -1] - top[:, -2]
    passed = out["confidence"] >= min_confidence if min_confidence > 0.0 else np.ones(lg.shape[0], bool)   # (a NaN confidence gates)
    out["split_mode"] = np.where(passed, out["raw_mode"], -1)
    return out


# float64 twin of capi.CANDIDATES_DTYPE (same leading fields), followed by what the record is derived from: the prefix sums in rank order (0 beyond K), the
# kept count before the cap, and the logit gap between the last kept and the first dropped class (inf when nothing is dropped)
CAND_DTYPE = np.dtype([("mask", "<u4"), ("count", "<i4"), ("order", "i1", (8,)), ("prob", "<f8", (6,)),
                       ("cum", "<f8", (6,)), ("n", "<i4"), ("gap", "<f8")])


def candidates_from_logits(size: int, logits, head_index: int | None = None, coverage: float = 0.0, max_modes: int = 0) -> np.ndarray:
    """Candidate set of the decision head per CU: classes ranked by logit (descending, equal logits in class order), softmax summed in class order, prefix
    sums in rank order, the shortest prefix with cum >= coverage (all K if none reaches it), all K when that prefix is longer than max_modes > 0 or a logit
    of the head is NaN (order then lists the classes in class order)."""
    classes = HEAD_CLASSES[size]
    lg = np.asarray(logits, np.float64)
    if lg.ndim == 1:
        lg = lg[None, :]
    assert lg.ndim == 2 and lg.shape[1] == sum(classes), (lg.shape, classes)
    dh = default_head(size) if head_index is None or head_index < 0 else head_index
    assert 0 <= dh < len(classes)
    K = classes[dh]
    assert 0.0 <= coverage < 1.0 and 0 <= max_modes <= K, (coverage, max_modes)
    lo = sum(classes[:dh])
    l = lg[:, lo:lo + K]
    n_cu = l.shape[0]
    rows = np.arange(n_cu)
    nan = np.isnan(l).any(axis=1)
    order = np.argsort(-np.where(np.isnan(l), -np.inf, l), axis=1, kind="stable")   # descending, equal logits keep class order
    order[nan] = np.arange(K)
    best = np.zeros(n_cu, np.int64)     # first-max argmax the way the device finds it (a NaN never wins a comparison)
    for k in range(1, K):
        best = np.where(l[:, k] > l[rows, best], k, best)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(l - l[rows, best][:, None])
        s = np.zeros(n_cu)
        for c in range(K):              # class order, like the device
            s = s + e[:, c]
        prob = e / s[:, None]
    out = np.zeros((n_cu,), CAND_DTYPE)
    out["order"] = -1
    out["order"][:, :K] = order
    out["prob"][:, :K] = prob
    cum = np.zeros(n_cu)
    kept = np.full(n_cu, K, np.int32)
    found = np.zeros(n_cu, bool)
    for r in range(K):                  # rank order
        cum = cum + prob[rows, order[:, r]]
        out["cum"][:, r] = cum
        hit = ~found & (cum >= coverage)
        kept[hit] = r + 1
        found |= hit
    out["n"] = kept
    full = nan | ((kept > max_modes) if max_modes > 0 else np.zeros(n_cu, bool))
    count = np.where(full, K, kept)
    mask = np.zeros(n_cu, np.uint32)
    for r in range(K):
        mask |= np.where(r < count, np.uint32(1) << order[:, r].astype(np.uint32), np.uint32(0)).astype(np.uint32)
    out["mask"] = mask
    out["count"] = count
    srt = l[rows[:, None], order]
    gap = np.full(n_cu, np.inf)
    drop = count < K
    with np.errstate(invalid="ignore"):
        gap[drop] = srt[drop, count[drop] - 1] - srt[drop, np.minimum(count[drop], K - 1)]
    out["gap"] = gap
    return out
