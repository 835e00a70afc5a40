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
"""
from __future__ import annotations

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

BLOCKS = (8, 16, 32, 64)
MAX_RANGE = 64
MAX_LAMBDA = 65535
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
