"""Prediction pictures: numpy restatement of the device's block motion search and quarter-sample compensation (include/mltcnn.h, "Prediction pictures on the
device"; csrc/mlt_motion_kernels.inc).  Everything is integer arithmetic with one stated rule, so the device must return these arrays byte for byte -- this module is
what tests/test_motion_*.py compare it against, in the way decisions.build_tree restates the descent.

  blocks      block (i, j) of a W x H picture covers x in [i B, min((i + 1) B, W)), likewise y: border blocks are clipped
  field       [by][bx][2] int16 {mvx, mvy}, quarter luma samples
  R(x, y)     ref[clip(y, 0, H - 1)][clip(x, 0, W - 1)]
  compensate  ix = mvx >> 2, fx = mvx & 3 (likewise y); t_j = sum_k C[fx][k] R(x + ix + k - 3, y + iy + j - 3); v = sum_j C[fy][j] t_j;
              dst = clip((v + 2048) >> 12, 0, 1023) -- int32 throughout.  Its own rounding: not the encoder's interpolation
  search      over (dx, dy) in [-range, range]^2: SAD = sum |cur(x, y) - R(x + dx, y + dy)| over the block, cost = SAD + lam (|dx| + |dy|); the winner has the
              smallest (cost, |dx| + |dy|, dy, dx); mv = (4 dx, 4 dy)

Quarter-sample refinement and per-block reference choice (include/mltcnn.h: mlt_picture_predict_refs, mlt_picture_compensate_refs) -- P_mv^r is `compensate` of
refs[r], 1 <= n_refs <= MAX_REFS, the same picture may be listed more than once:
  step 1      the integer search above, per reference r, unchanged -> (dx_r, dy_r)
  step 2      refine, per reference: candidates mv = (4 dx_r + qx, 4 dy_r + qy), qx, qy in WINDOWS[subpel] = {0} / {-2, 0, 2} / {-3 .. 3}, all of them;
              SADP = sum |cur(x, y) - P_mv^r(x, y)| over the block's clipped samples (cur: the int16 values as they are),
              cost_q = 4 SADP + lam (|mvx| + |mvy|) in uint32
  step 3      the winner over all (r, mv) has the smallest (cost_q, |mvx| + |mvy|, r, mvy, mvx), mvy and mvx signed -- as one unsigned 64-bit key
              cost_q << 32 | l1 << 22 | r << 20 | (mvy + 512) << 10 | (mvx + 512); outputs: the block's vector, reference index and cost_q
  step 4      dst is, block by block, P_mv^r of the winner (compensate_refs)
cost_q is in quarter units and on CLIPPED samples: it is 4 x the integer search's cost only while every reference sample the block touches lies in 0 .. 1023.
With subpel = 0 and one reference the field and the plane are `predict`'s.
"""
from __future__ import annotations

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

BLOCKS = (8, 16, 32, 64)
MAX_RANGE = 64
MAX_LAMBDA = 65535
MAX_REFS = 4
WINDOWS = ((0,), (-2, 0, 2), (-3, -2, -1, 0, 1, 2, 3))   # the refinement's offsets a side, by subpel
# the quarter-sample luma taps, by fraction
TAPS = np.array([[0, 0, 0, 64, 0, 0, 0, 0],
                 [-1, 4, -10, 58, 17, -5, 1, 0],
                 [-1, 4, -11, 40, 40, -11, 4, -1],
                 [0, 1, -5, 17, 58, -10, 4, -1]], np.int32)


def blocks(width: int, height: int, block: int):
    """-> (bx, by) = (ceil(width / block), ceil(height / block))."""
    assert block in BLOCKS and width >= 1 and height >= 1
    return -(-width // block), -(-height // block)


def _per_sample(field2d: np.ndarray, block: int, height: int, width: int) -> np.ndarray:
    """[by, bx] -> [height, width]: every sample takes its block's value."""
    return np.repeat(np.repeat(field2d, block, axis=0), block, axis=1)[:height, :width]


def compensate(ref: np.ndarray, mv: np.ndarray, block: int = 16) -> np.ndarray:
    """ref: int16 [H, W]; mv: int16 [by, bx, 2] -> the prediction plane, int16 [H, W]."""
    ref = np.asarray(ref)
    assert ref.dtype == np.int16 and ref.ndim == 2
    H, W = ref.shape
    bx, by = blocks(W, H, block)
    mv = np.asarray(mv)
    assert mv.dtype == np.int16 and mv.shape == (by, bx, 2)
    mvx = _per_sample(mv[:, :, 0].astype(np.int32), block, H, W)
    mvy = _per_sample(mv[:, :, 1].astype(np.int32), block, H, W)
    ix, fx, iy, fy = mvx >> 2, mvx & 3, mvy >> 2, mvy & 3
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int32)
    r32 = ref.astype(np.int32)
    cols = [np.clip(xs + ix + (k - 3), 0, W - 1) for k in range(8)]
    cxs = [TAPS[fx, k] for k in range(8)]
    v = np.zeros((H, W), np.int32)
    for j in range(8):
        row = np.clip(ys + iy + (j - 3), 0, H - 1)
        t = np.zeros((H, W), np.int32)
        for k in range(8):
            t += cxs[k] * r32[row, cols[k]]
        v += TAPS[fy, j] * t
    return np.clip((v + 2048) >> 12, 0, 1023).astype(np.int16)


def sad_volume(cur: np.ndarray, ref: np.ndarray, block: int, search_range: int) -> np.ndarray:
    """-> uint32 [by, bx, 2 R + 1 (dy), 2 R + 1 (dx)]: every block's SAD under every candidate.  One pass per dy over an edge-padded reference: the 2 R + 1
    horizontal shifts are a sliding window, the block sums two reduceat calls."""
    cur, ref = np.asarray(cur), np.asarray(ref)
    assert cur.dtype == np.int16 and ref.dtype == np.int16 and cur.ndim == 2 and cur.shape == ref.shape
    R = int(search_range)
    assert 0 <= R <= MAX_RANGE
    H, W = cur.shape
    bx, by = blocks(W, H, block)
    nC = 2 * R + 1
    pad = np.pad(ref.astype(np.int32), R, mode="edge")   # pad[y + R, x + R] = R(x, y) for -R <= x < W + R
    c32 = cur.astype(np.int32)[:, None, :]
    y_edges, x_edges = np.arange(0, H, block), np.arange(0, W, block)
    out = np.zeros((by, bx, nC, nC), np.uint32)
    for dyi in range(nC):
        win = sliding_window_view(pad[dyi:dyi + H, :], W, axis=1)   # [H, nC (dx), W]: win[y, dxi, x] = R(x + dxi - R, y + dyi - R)
        d = np.abs(win - c32)
        d = np.add.reduceat(d, y_edges, axis=0)
        d = np.add.reduceat(d, x_edges, axis=2)                     # [by, nC, bx]
        out[:, :, dyi, :] = d.transpose(0, 2, 1)
    return out


def pick(sad: np.ndarray, lam: int = 0):
    """sad_volume's array -> (mv int16 [by, bx, 2], cost uint32 [by, bx]): per block the candidate with the smallest (cost, |dx| + |dy|, dy, dx)."""
    by, bx, nC, _ = sad.shape
    R = (nC - 1) // 2
    assert 0 <= lam <= MAX_LAMBDA
    d = np.arange(-R, R + 1, dtype=np.int64)
    dy, dx = d[:, None], d[None, :]
    l1 = np.abs(dy) + np.abs(dx)
    cost = sad.astype(np.int64) + int(lam) * l1
    key = (cost << 24) | (l1 << 16) | ((dy + 64) << 8) | (dx + 64)   # the lexicographic order as one integer (cost < 2^32, the rest a byte each)
    best = key.reshape(by, bx, nC * nC).min(axis=2)
    mv = np.stack([4 * ((best & 0xff) - 64), 4 * (((best >> 8) & 0xff) - 64)], axis=2).astype(np.int16)
    return mv, (best >> 24).astype(np.uint32)


def search(cur: np.ndarray, ref: np.ndarray, block: int = 16, search_range: int = 16, lam: int = 0):
    """-> (mv int16 [by, bx, 2] = {4 dx, 4 dy}, cost uint32 [by, bx])."""
    return pick(sad_volume(cur, ref, block, search_range), lam)


def predict(cur: np.ndarray, ref: np.ndarray, block: int = 16, search_range: int = 16, lam: int = 0):
    """search, then compensate with the found field -> (plane, mv, cost): what MltCnn.predict_picture leaves in dst and returns."""
    mv, cost = search(cur, ref, block, search_range, lam)
    return compensate(ref, mv, block), mv, cost


def _fraction_planes(ref: np.ndarray, pad: int, fractions):
    """{(fx, fy): int32 [H + 2 pad - 7, W + 2 pad - 7]}: v of the compensation rule at every integer position of the edge-padded reference (edge padding IS the
    clamp of R), before the rounding -- plane[Y, X] is v for the sample whose tap (0, 0) reads padded (Y, X), i.e. for position (X + 3 - pad, Y + 3 - pad)."""
    padded = np.pad(ref.astype(np.int32), pad, mode="edge")
    hor = {}
    for fx in sorted({f[0] for f in fractions}):
        win = sliding_window_view(padded, 8, axis=1)           # [.., X, k] = padded[.., X + k]
        hor[fx] = win @ TAPS[fx]
    out = {}
    for fx, fy in fractions:
        win = sliding_window_view(hor[fx], 8, axis=0)          # [Y, X, j] = hor[Y + j, X]
        out[(fx, fy)] = win @ TAPS[fy]
    return out


def refine(cur: np.ndarray, refs, mv_int: np.ndarray, block: int = 16, lam: int = 0, subpel: int = 2):
    """Steps 2 and 3.  refs: the n_refs int16 [H, W] references; mv_int: int16 [n_refs, by, bx, 2], every reference's integer winners {4 dx, 4 dy} (`search`)
    -> (mv int16 [by, bx, 2], ref uint8 [by, bx], cost_q uint32 [by, bx]).  Per reference the 16 fractions' filtered planes are computed ONCE over the padded
    picture; a candidate is then a gather at its per-block integer offset, a rounding, and block sums by two reduceat calls."""
    cur = np.asarray(cur)
    refs = [np.asarray(r) for r in refs]
    assert cur.dtype == np.int16 and cur.ndim == 2 and 1 <= len(refs) <= MAX_REFS and all(r.dtype == np.int16 and r.shape == cur.shape for r in refs)
    assert subpel in (0, 1, 2) and 0 <= lam <= MAX_LAMBDA
    H, W = cur.shape
    bx, by = blocks(W, H, block)
    mv_int = np.asarray(mv_int)
    assert mv_int.dtype == np.int16 and mv_int.shape == (len(refs), by, bx, 2) and not (mv_int & 3).any() and np.abs(mv_int).max(initial=0) <= 4 * MAX_RANGE
    qs = WINDOWS[subpel]
    pad = MAX_RANGE + 8
    c32 = cur.astype(np.int32)
    ys, xs = np.mgrid[0:H, 0:W]
    y_edges, x_edges = np.arange(0, H, block), np.arange(0, W, block)
    best = np.full((by, bx), (1 << 64) - 1, np.uint64)
    for r, ref in enumerate(refs):
        planes = _fraction_planes(ref, pad, sorted({(qx & 3, qy & 3) for qx in qs for qy in qs}))
        for qy in qs:
            for qx in qs:
                mvx, mvy = mv_int[r, :, :, 0].astype(np.int64) + qx, mv_int[r, :, :, 1].astype(np.int64) + qy
                col = xs + _per_sample(mvx >> 2, block, H, W) + (pad - 3)
                row = ys + _per_sample(mvy >> 2, block, H, W) + (pad - 3)
                p = np.clip((planes[(qx & 3, qy & 3)][row, col] + 2048) >> 12, 0, 1023)
                d = np.add.reduceat(np.add.reduceat(np.abs(c32 - p), y_edges, axis=0), x_edges, axis=1).astype(np.uint64)
                l1 = (np.abs(mvx) + np.abs(mvy)).astype(np.uint64)
                cost = np.uint64(4) * d + np.uint64(lam) * l1
                assert int(cost.max()) < 1 << 32
                key = (cost << np.uint64(32)) | (l1 << np.uint64(22)) | np.uint64(r << 20) | ((mvy + 512).astype(np.uint64) << np.uint64(10)) | (mvx + 512).astype(np.uint64)
                best = np.minimum(best, key)
    mv = np.stack([(best & np.uint64(0x3ff)).astype(np.int64) - 512, ((best >> np.uint64(10)) & np.uint64(0x3ff)).astype(np.int64) - 512], axis=2).astype(np.int16)
    return mv, ((best >> np.uint64(20)) & np.uint64(3)).astype(np.uint8), (best >> np.uint64(32)).astype(np.uint32)


def compensate_refs(refs, mv: np.ndarray, ref_idx=None, block: int = 16) -> np.ndarray:
    """Step 4: block by block `compensate` of refs[ref_idx[block]] with the field mv; ref_idx: uint8 [by, bx], None = reference 0 everywhere."""
    refs = [np.asarray(r) for r in refs]
    assert 1 <= len(refs) <= MAX_REFS
    H, W = refs[0].shape
    bx, by = blocks(W, H, block)
    if ref_idx is None:
        return compensate(refs[0], mv, block)
    ref_idx = np.asarray(ref_idx)
    assert ref_idx.dtype == np.uint8 and ref_idx.shape == (by, bx) and int(ref_idx.max()) < len(refs)
    which = _per_sample(ref_idx, block, H, W)
    out = np.zeros((H, W), np.int16)
    for r in np.unique(ref_idx):
        out = np.where(which == r, compensate(refs[int(r)], mv, block), out)
    return out


def predict_refs(cur: np.ndarray, refs, block: int = 16, search_range: int = 16, lam: int = 0, subpel: int = 2):
    """Steps 1 - 4 -> (plane, mv, ref, cost_q): what MltCnn.predict_picture_refs leaves in dst and returns."""
    mv_int = np.stack([search(cur, r, block, search_range, lam)[0] for r in refs])
    mv, ref_idx, cost = refine(cur, refs, mv_int, block, lam, subpel)
    return compensate_refs(refs, mv, ref_idx, block), mv, ref_idx, cost
