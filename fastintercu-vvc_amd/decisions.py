"""Host restatement of the device's decision records (include/mltcnn.h: mlt_decision), in float64.

`from_logits` turns an [n, num_logits] array of head logits (lvl1..lvlN concatenated, as every entry point returns them) into the records
heads_kernel writes: per head the first-max argmax (torch.argmax) and its softmax probability, the decision head's top-2 margin, and the
confidence gate.  It is what the tests compare the device against, the way synth.flat_quad_fraction restates the flat statistic, and what
tools/confidence_sweep.py evaluates on a call dump."""
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
