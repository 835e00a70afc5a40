#!/usr/bin/env python3
"""Split-prior maps of a whole picture: every complete CU of the size-aligned grid, every loaded CU size, from two device-resident planes.

Reads the original and the prediction luma of one frame -- `.npy` int16 [height, width], or raw 16-bit little-endian luma (e.g. the first plane of a
10-bit 4:0:0 / 4:2:0 .yuv) with --width / --height -- uploads each ONCE (MltCnn.picture), runs grid_positions + predict_at for every requested size
and writes per size `<out>_<S>_split.npy` (int32, -1 where the confidence gate withholds), `<out>_<S>_confidence.npy` (float32) and
`<out>_<S>_mask.npy` (uint32 candidate mask), each shaped [height // S, width // S]; prints the class histogram of the decision head.

  python tools/picture_map.py org.npy pred.npy --weights-dir DIR --sizes 128,64 --poc 8 --qp 32 --out maps/frame8
  python tools/picture_map.py org.yuv pred.yuv --width 1920 --height 1080 --synthetic 10 --coverage 0.9 --out /tmp/f
  python tools/picture_map.py org.npy pred.npy --weights-dir DIR --tree --min-size 32 --out maps/frame8

--tree [--min-size S]: the PARTITION TREE instead of the per-size maps (MltCnn.predict_tree): the CTUs, and only where the network says "quad split" their
children, down to S (default 16); loads every size 128 .. S, writes `<out>_tree_nodes.npy` (capi.TREE_NODE_DTYPE, the contract's order) and `<out>_leafmap.npy`
(uint8 [height // 16, width // 16]) and prints the nodes per level.
--tree --frames N: the inputs hold N frames -- `.npy` int16 [N, height, width], or N consecutive raw planes -- and ALL N trees come from ONE call
(MltCnn.predict_trees: one network pass per level over the nodes of all frames); --poc is the first frame's POC, frame f takes --poc + f.  Writes
`<out>_f<f>_tree_nodes.npy` and `<out>_f<f>_leafmap.npy` per frame.

--tree --tree-qps 22,27,32,37: the trees of ONE frame under several QPs from ONE call (MltCnn.predict_tree_sweep: one descent over the union of the trees, the
network once per union node, the heads once per QP); --qp is not consulted and --frames does not go with it.  Writes `<out>_qp<QP>_tree_nodes.npy` and
`<out>_qp<QP>_leafmap.npy` per QP and prints the nodes per level per QP and of the union.

--tree --frames N --gop-qps 22,27,32,37 [--qp-offsets 0,3,4,3,...]: the trees of N frames under several base QPs each from ONE call (MltCnn.predict_trees_sweep:
one descent over the unions of all frames, the network once per union node); frame f under base QP b runs at QP b + offset f (--qp-offsets: one integer per
frame, default 0 for all; an RA GOP does not code every frame at the base QP); --qp is not consulted.  Writes `<out>_f<f>_qp<QP>_tree_nodes.npy` and
`<out>_f<f>_qp<QP>_leafmap.npy` per (frame, QP), <QP> the frame's QP b + offset, and prints the nodes per level per (frame, QP) and of every frame's union.
(--tree --frames N --tree-qps stays refused: --tree-qps is the one-frame form.)

--qps 22,27,32,37 (without --tree): one map set PER QP from ONE sweep call per size (MltCnn.predict_at_sweep: the network runs once, the heads once per QP),
written as `<out>_<S>_qp<QP>_split.npy` etc.; --qp is not consulted.  Combined with --tree it is refused: trees under several QPs are --tree-qps.

--motion BLOCK,RANGE[,LAMBDA] (with any of the above): the second file is not a prediction but the REFERENCE frame, another original, and the prediction is built
on the device before the maps or trees (MltCnn.predict_picture: integer-sample block search of the original in the reference over [-RANGE, RANGE]^2 on BLOCK x
BLOCK blocks, cost SAD + LAMBDA (|dx| + |dy|), then quarter-sample compensation; fastintercu_vvc_amd/motion.py is the rule) -- no prediction plane crosses PCIe.
With --frames N the second file holds N frames like the first and frame f's reference is its frame f - 1, frame 0's its frame 0 (pass the originals' file twice
for a GOP of originals: every frame is then predicted from its predecessor and frame 0 from itself).  Without --motion nothing changes.

--motion-refine SUBPEL[,NREFS] (with --motion only): the prediction comes from MltCnn.predict_picture_refs instead -- the integer winner refined over the half
(SUBPEL 1) or quarter (SUBPEL 2) sample window (0: none), each block choosing among NREFS (1 .. 4, default 1) references: with --frames N frame f's references
are frames f - 1, f - 2, ... of the second file, clipped at frame 0; a single frame is listed NREFS times.

  python tools/picture_map.py cur.npy ref.npy --motion 16,16 --synthetic 10 --tree --out maps/frame8

File reading and grid logic (read_picture, grid, to_map, histogram) need neither a device nor the library; run_maps needs the MI355X."""
import argparse
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (128, 64, 32, 16)


def read_picture(path: str, width: int | None = None, height: int | None = None) -> np.ndarray:
    """-> int16 [height, width], C-contiguous.  `.npy`: a 2-D int16 array (width / height, if given, must match).  Anything else: raw 16-bit little-endian
    samples, the first width x height of the file (the luma plane of its first frame)."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.ndim != 2 or a.dtype != np.int16:
            raise ValueError(f"{path}: want a 2-D int16 array, got {a.dtype} {a.shape}")
        if (width and a.shape[1] != width) or (height and a.shape[0] != height):
            raise ValueError(f"{path}: {a.shape[1]}x{a.shape[0]}, not the {width}x{height} asked for")
        return np.ascontiguousarray(a)
    if not width or not height:
        raise ValueError(f"{path}: a raw file needs --width and --height")
    count = width * height
    a = np.fromfile(path, dtype="<u2", count=count)
    if a.size != count:
        raise ValueError(f"{path}: a {width}x{height} plane needs {count} samples of 16 bits, the file holds {a.size}")
    if a.max(initial=0) > 0x7FFF:
        raise ValueError(f"{path}: samples above 32767 do not fit a Pel (int16)")
    return a.astype(np.int16).reshape(height, width)


def read_frames(path: str, frames: int, width: int | None = None, height: int | None = None) -> np.ndarray:
    """-> int16 [frames, height, width], C-contiguous.  `.npy`: a 3-D int16 array of exactly `frames` frames (a 2-D array is one frame).  Anything else: raw 16-bit
    little-endian samples, `frames` consecutive width x height planes from the start of the file."""
    if frames < 1:
        raise ValueError(f"--frames {frames}: want at least 1")
    if path.endswith(".npy"):
        a = np.load(path)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.dtype != np.int16:
            raise ValueError(f"{path}: want an int16 array [frames, height, width], got {a.dtype} {a.shape}")
        if a.shape[0] != frames:
            raise ValueError(f"{path}: holds {a.shape[0]} frames, --frames says {frames}")
        if (width and a.shape[2] != width) or (height and a.shape[1] != height):
            raise ValueError(f"{path}: {a.shape[2]}x{a.shape[1]}, not the {width}x{height} asked for")
        return np.ascontiguousarray(a)
    if not width or not height:
        raise ValueError(f"{path}: a raw file needs --width and --height")
    count = frames * width * height
    a = np.fromfile(path, dtype="<u2", count=count)
    if a.size != count:
        raise ValueError(f"{path}: {frames} planes of {width}x{height} need {count} samples of 16 bits, the file holds {a.size}")
    if a.max(initial=0) > 0x7FFF:
        raise ValueError(f"{path}: samples above 32767 do not fit a Pel (int16)")
    return a.astype(np.int16).reshape(frames, height, width)


def grid(width: int, height: int, size: int) -> np.ndarray:
    """[count, 2] int32 {x, y}: the complete CUs of the size-aligned grid, raster order -- what capi.grid_positions returns, in numpy (partial CUs at
    the right and bottom border are left out: VTM splits them implicitly)."""
    if size not in SIZES or width < size or height < size:
        return np.zeros((0, 2), np.int32)
    ys, xs = np.meshgrid(np.arange(height // size, dtype=np.int32) * size, np.arange(width // size, dtype=np.int32) * size, indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32)


def to_map(values: np.ndarray, width: int, height: int, size: int) -> np.ndarray:
    """Per-CU values in grid (raster) order -> [height // size, width // size]."""
    return np.asarray(values).reshape(height // size, width // size)


def histogram(split: np.ndarray, classes: int) -> dict:
    """{class: count} of the split map, -1 (withheld by the confidence gate) included when present."""
    h = {k: int((split == k).sum()) for k in range(classes)}
    if (split < 0).any():
        h[-1] = int((split < 0).sum())
    return h


def run_maps(m, org: np.ndarray, pred: np.ndarray, sizes, poc: int, qp: int, motion=None) -> dict:
    """m: an MltCnn with `sizes` loaded.  -> {size: {"xy", "split", "confidence", "mask"}} with the three maps shaped [height // size, width // size].
    motion: see uploaded()."""
    from fastintercu_vvc_amd import capi
    assert org.shape == pred.shape
    height, width = org.shape
    out = {}
    with uploaded(m, org, pred, motion) as pics:
        p_org, p_pred = pics[0]
        for size in sizes:
            xy = capi.grid_positions(width, height, size)
            if not len(xy):
                continue
            n = len(xy)
            r = m.predict_at(size, p_org, p_pred, xy, np.full(n, poc, np.int32), np.full(n, qp, np.int32), want=("decisions", "candidates"))
            out[size] = {"xy": xy, "split": to_map(r["decisions"]["split_mode"], width, height, size),
                         "confidence": to_map(r["decisions"]["confidence"], width, height, size), "mask": to_map(r["candidates"]["mask"], width, height, size)}
    return out


def run_maps_sweep(m, org: np.ndarray, pred: np.ndarray, sizes, poc: int, qps, motion=None) -> dict:
    """run_maps under every QP of `qps` from one sweep call per size -> {size: {qp: {"xy", "split", "confidence", "mask"}}} (a duplicate QP keeps one entry)."""
    from fastintercu_vvc_amd import capi
    assert org.shape == pred.shape
    height, width = org.shape
    out = {}
    with uploaded(m, org, pred, motion) as pics:
        p_org, p_pred = pics[0]
        for size in sizes:
            xy = capi.grid_positions(width, height, size)
            if not len(xy):
                continue
            r = m.predict_at_sweep(size, p_org, p_pred, xy, np.full(len(xy), poc, np.int32), qps, want=("decisions", "candidates"))
            out[size] = {int(qp): {"xy": xy, "split": to_map(r["decisions"]["split_mode"][q], width, height, size),
                                   "confidence": to_map(r["decisions"]["confidence"][q], width, height, size),
                                   "mask": to_map(r["candidates"]["mask"][q], width, height, size)} for q, qp in enumerate(qps)}
    return out


def parse_qps(text: str) -> tuple:
    """"22,27,32,37" -> (22, 27, 32, 37); 1 .. 32 integers (capi.SWEEP_MAX_QPS)."""
    try:
        qps = tuple(int(v) for v in text.split(",") if v.strip())
    except ValueError:
        raise ValueError(f"--qps {text}: want comma-separated integers") from None
    if not 1 <= len(qps) <= 32:
        raise ValueError(f"--qps {text}: want 1 .. 32 values")
    return qps


def tree_sizes(min_size: int) -> tuple:
    """The CU sizes a tree from 128 down to min_size evaluates (what --tree loads instead of --sizes)."""
    if min_size not in SIZES:
        raise ValueError(f"--min-size {min_size}: want one of {SIZES}")
    return tuple(s for s in SIZES if s >= min_size)


def tree_summary(nodes: np.ndarray) -> list:
    """[(size, nodes, of them descending)] per level of a node array."""
    return [(int(s), int((nodes["size"] == s).sum()), int(((nodes["size"] == s) & (nodes["first_child"] >= 0)).sum())) for s in SIZES if (nodes["size"] == s).any()]


def motion_references(second: np.ndarray) -> list:
    """--motion: the reference frame of every frame out of the second file's array -- [height, width]: that frame; [frames, height, width]: frame f - 1 for
    frame f, frame 0 for frame 0."""
    if second.ndim == 2:
        return [second]
    return [second[max(f - 1, 0)] for f in range(second.shape[0])]


def motion_reference_lists(second: np.ndarray, n_refs: int) -> list:
    """--motion-refine: the n_refs reference frames of every frame -- [frames, height, width]: frames f - 1, f - 2, ..., clipped at frame 0; [height, width]:
    that frame n_refs times."""
    if second.ndim == 2:
        return [[second] * n_refs]
    return [[second[max(f - 1 - k, 0)] for k in range(n_refs)] for f in range(second.shape[0])]


@contextlib.contextmanager
def uploaded(m, org: np.ndarray, pred: np.ndarray, motion=None):
    """The frames of org / pred ([height, width] or [frames, height, width]) as resident picture pairs [(org_pic, pred_pic), ...], closed on exit.
    motion = (block, range, lambda): `pred` holds REFERENCE frames instead (motion_references) and every pred_pic is built on the device from the frame's original
    and its reference (MltCnn.predict_picture, enqueued only: the calls that follow see it in stream order); motion = (block, range, lambda, subpel, n_refs):
    from its n_refs references (motion_reference_lists) with refinement (MltCnn.predict_picture_refs)."""
    assert org.shape == pred.shape
    height, width = org.shape[-2:]
    held, pics = [], []
    try:
        if motion is None:
            for o, p in zip(org.reshape(-1, height, width), pred.reshape(-1, height, width)):
                held += [m.picture(width, height).upload(o), m.picture(width, height).upload(p)]
                pics.append((held[-2], held[-1]))
        elif len(motion) == 5:
            block, search_range, lam, subpel, n_refs = motion
            for o, refs in zip(org.reshape(-1, height, width), motion_reference_lists(pred, n_refs)):
                first = len(held)
                held += [m.picture(width, height).upload(o)] + [m.picture(width, height).upload(r) for r in refs] + [m.picture(width, height)]
                m.predict_picture_refs(held[first], held[first + 1:-1], held[-1], block=block, search_range=search_range, lam=lam, subpel=subpel, want_field=False)
                pics.append((held[first], held[-1]))
        else:
            block, search_range, lam = motion
            for o, r in zip(org.reshape(-1, height, width), motion_references(pred)):
                held += [m.picture(width, height).upload(o), m.picture(width, height).upload(r), m.picture(width, height)]
                m.predict_picture(held[-3], held[-2], held[-1], block=block, search_range=search_range, lam=lam, want_field=False)
                pics.append((held[-3], held[-1]))
        yield pics
    finally:
        m.synchronize()   # (a prediction may still be in flight when an error unwinds)
        for p in held:
            p.close()


def parse_motion(text: str) -> tuple:
    """"16,16" or "16,16,4" -> (block, range, lambda): block 8 / 16 / 32 / 64, 0 <= range <= 64, 0 <= lambda <= 65535 (default 0)."""
    try:
        v = tuple(int(t) for t in text.split(","))
    except ValueError:
        raise ValueError(f"--motion {text}: want BLOCK,RANGE[,LAMBDA] as integers") from None
    if len(v) not in (2, 3) or v[0] not in (8, 16, 32, 64) or not 0 <= v[1] <= 64 or (len(v) == 3 and not 0 <= v[2] <= 65535):
        raise ValueError(f"--motion {text}: want BLOCK,RANGE[,LAMBDA] with BLOCK of 8,16,32,64, 0 <= RANGE <= 64, 0 <= LAMBDA <= 65535")
    return (v[0], v[1], v[2] if len(v) == 3 else 0)


def parse_motion_refine(text: str) -> tuple:
    """"2" or "2,3" -> (subpel, n_refs): subpel 0 / 1 / 2, 1 <= n_refs <= 4 (default 1)."""
    try:
        v = tuple(int(t) for t in text.split(","))
    except ValueError:
        raise ValueError(f"--motion-refine {text}: want SUBPEL[,NREFS] as integers") from None
    if len(v) not in (1, 2) or v[0] not in (0, 1, 2) or (len(v) == 2 and not 1 <= v[1] <= 4):
        raise ValueError(f"--motion-refine {text}: want SUBPEL[,NREFS] with SUBPEL of 0,1,2 and 1 <= NREFS <= 4")
    return (v[0], v[1] if len(v) == 2 else 1)


def run_tree(m, org: np.ndarray, pred: np.ndarray, poc: int, qp: int, min_size: int = 16, motion=None) -> dict:
    """m: an MltCnn with tree_sizes(min_size) loaded -> {"nodes", "leaf_map"} (MltCnn.predict_tree)."""
    assert org.ndim == 2
    with uploaded(m, org, pred, motion) as pics:
        return m.predict_tree(pics[0][0], pics[0][1], poc, qp, top=128, min_size=min_size, want=("leaf_map",))


def run_trees(m, org: np.ndarray, pred: np.ndarray, poc: int, qp: int, min_size: int = 16, motion=None) -> list:
    """org / pred: [frames, height, width]; m: an MltCnn with tree_sizes(min_size) loaded -> one {"nodes", "leaf_map", "first_node"} per frame, all from ONE
    call (MltCnn.predict_trees); frame f takes poc + f."""
    assert org.ndim == 3
    with uploaded(m, org, pred, motion) as pics:
        return m.predict_trees(pics, [poc + f for f in range(len(pics))], qp, top=128, min_size=min_size, want=("leaf_map",))


def run_tree_sweep(m, org: np.ndarray, pred: np.ndarray, poc: int, qps, min_size: int = 16, motion=None) -> list:
    """m: an MltCnn with tree_sizes(min_size) loaded -> one {"nodes", "leaf_map", "first_node", "union_nodes"} per QP of `qps`, all from ONE call
    (MltCnn.predict_tree_sweep)."""
    assert org.ndim == 2
    with uploaded(m, org, pred, motion) as pics:
        return m.predict_tree_sweep(pics[0][0], pics[0][1], poc, qps, top=128, min_size=min_size, want=("leaf_map",))


def run_trees_sweep(m, org: np.ndarray, pred: np.ndarray, poc: int, qp_offsets, qps, min_size: int = 16, motion=None) -> list:
    """org / pred: [frames, height, width]; m: an MltCnn with tree_sizes(min_size) loaded -> result[frame][point], each {"nodes", "leaf_map", "first_node",
    "union_nodes"}, all from ONE call (MltCnn.predict_trees_sweep); frame f takes poc + f and, under point q, QP qp_offsets[f] + qps[q]."""
    assert org.ndim == 3
    with uploaded(m, org, pred, motion) as pics:
        return m.predict_trees_sweep(pics, [poc + f for f in range(len(pics))], list(qp_offsets), qps, top=128, min_size=min_size, want=("leaf_map",))


def parse_offsets(text: str, frames: int) -> tuple:
    """"0,3,4,3" -> (0, 3, 4, 3): one integer per frame."""
    try:
        off = tuple(int(v) for v in text.split(",") if v.strip())
    except ValueError:
        raise ValueError(f"--qp-offsets {text}: want comma-separated integers") from None
    if len(off) != frames:
        raise ValueError(f"--qp-offsets {text}: want one value per frame ({frames}), got {len(off)}")
    return off


def save_tree(prefix: str, t: dict) -> None:
    np.save(f"{prefix}_tree_nodes.npy", t["nodes"])
    np.save(f"{prefix}_leafmap.npy", t["leaf_map"])


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("org")
    ap.add_argument("pred")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--sizes", default="128", help="comma-separated CU sizes")
    ap.add_argument("--weights-dir", help="directory with MLTORPQ_splitMode_<S>.mltw (tools/convert_weights.py)")
    ap.add_argument("--synthetic", type=int, help="seeded synthetic weights instead of --weights-dir")
    ap.add_argument("--poc", type=int, default=0)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--qps", default=None, help="comma-separated QPs: one map set per QP from one sweep call per size (not with --tree)")
    ap.add_argument("--min-conf", type=float, default=0.0, help="confidence gate")
    ap.add_argument("--coverage", type=float, default=0.0, help="candidate policy: coverage")
    ap.add_argument("--max-modes", type=int, default=0, help="candidate policy: cap")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", required=True, help="prefix of the .npy maps")
    ap.add_argument("--tree", action="store_true", help="the partition tree (quadtree descent on the device) instead of the per-size maps")
    ap.add_argument("--min-size", type=int, default=None, help="with --tree: the smallest CU size of the descent (default 16)")
    ap.add_argument("--frames", type=int, default=None, help="with --tree: the inputs hold this many frames; all trees from one call, --poc is the first frame's")
    ap.add_argument("--tree-qps", default=None, help="with --tree: comma-separated QPs, one tree per QP from one call (not with --frames)")
    ap.add_argument("--gop-qps", default=None, help="with --tree --frames N: comma-separated base QPs, one tree per (frame, QP) from one call")
    ap.add_argument("--qp-offsets", default=None, help="with --gop-qps: one QP offset per frame, comma-separated (default 0)")
    ap.add_argument("--motion", default=None, help="BLOCK,RANGE[,LAMBDA]: the second file is the REFERENCE frame; the prediction is built on the device")
    ap.add_argument("--motion-refine", default=None, help="with --motion: SUBPEL[,NREFS] -- half (1) / quarter (2) sample refinement, per-block choice among NREFS references")
    args = ap.parse_args(argv)
    sizes = tuple(int(s) for s in args.sizes.split(",") if s)
    if not sizes or any(s not in SIZES for s in sizes) or (args.weights_dir is None) == (args.synthetic is None):
        ap.error("--sizes from 128,64,32,16 and exactly one of --weights-dir / --synthetic")
    if args.min_size is not None and not args.tree:
        ap.error("--min-size goes with --tree")
    if args.frames is not None and (not args.tree or not 1 <= args.frames <= 256):
        ap.error("--frames goes with --tree, 1 .. 256")
    args.motion_cfg = None
    if args.motion is not None:
        try:
            args.motion_cfg = parse_motion(args.motion)
        except ValueError as e:
            ap.error(str(e))
    if args.motion_refine is not None:
        if args.motion_cfg is None:
            ap.error("--motion-refine goes with --motion")
        try:
            args.motion_cfg += parse_motion_refine(args.motion_refine)
        except ValueError as e:
            ap.error(str(e))
    args.qp_list = None
    if args.qps is not None:
        if args.tree:
            ap.error("--qps does not go with --tree: the descents of a tree diverge per QP and there is no tree sweep; run one --tree call per QP")
        try:
            args.qp_list = parse_qps(args.qps)
        except ValueError as e:
            ap.error(str(e))
    args.tree_qp_list = None
    if args.tree_qps is not None:
        if not args.tree or args.frames is not None:
            ap.error("--tree-qps goes with --tree and not with --frames")
        try:
            args.tree_qp_list = parse_qps(args.tree_qps)
        except ValueError as e:
            ap.error(str(e).replace("--qps", "--tree-qps"))
    args.gop_qp_list, args.qp_offset_list = None, None
    if args.gop_qps is not None:
        if not args.tree or args.frames is None:
            ap.error("--gop-qps goes with --tree --frames N")
        try:
            args.gop_qp_list = parse_qps(args.gop_qps)
            args.qp_offset_list = parse_offsets(args.qp_offsets, args.frames) if args.qp_offsets is not None else (0,) * args.frames
        except ValueError as e:
            ap.error(str(e).replace("--qps", "--gop-qps"))
        if any(not -2 ** 31 <= o + q < 2 ** 31 for o in args.qp_offset_list for q in args.gop_qp_list):
            ap.error("--gop-qps / --qp-offsets: an offset + QP does not fit 32 bits")
    elif args.qp_offsets is not None:
        ap.error("--qp-offsets goes with --gop-qps")
    if args.tree:
        if args.min_size is None:
            args.min_size = 16
        if args.min_size not in SIZES:
            ap.error("--min-size from 128,64,32,16")
        sizes = tree_sizes(args.min_size)   # every level of the descent (--sizes is not consulted)
    args.size_list = sizes
    return args


def main(argv=None):
    args = parse_args(argv)
    sizes = args.size_list
    if args.frames is not None:
        org = read_frames(args.org, args.frames, args.width, args.height)
        pred = read_frames(args.pred, args.frames, org.shape[2], org.shape[1])
    else:
        org = read_picture(args.org, args.width, args.height)
        pred = read_picture(args.pred, org.shape[1], org.shape[0])
    import mltcnn_pkg
    pkg = mltcnn_pkg.load()
    blobs = None
    if args.synthetic is not None:
        blobs = {s: pkg.weights.synthetic_blob(pkg.synth.ARCH_CTU if s == 128 else pkg.synth.ARCH_CU, args.synthetic) for s in sizes}
    m = pkg.MltCnn(device=args.device, sizes=sizes, weights_dir=args.weights_dir, blobs=blobs)
    for s in sizes:
        if args.min_conf > 0:
            m.set_confidence_gate(s, args.min_conf)
        if args.coverage > 0 or args.max_modes > 0:
            m.set_candidate_policy(s, args.coverage, args.max_modes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.tree and args.gop_qp_list is not None:
        res = run_trees_sweep(m, org, pred, args.poc, args.qp_offset_list, args.gop_qp_list, args.min_size, args.motion_cfg)
        for f, (off, row) in enumerate(zip(args.qp_offset_list, res)):
            for qp, t in zip(args.gop_qp_list, row):
                save_tree(f"{args.out}_f{f}_qp{qp + off}", t)
                print(f"frame {f} (poc {args.poc + f}) qp {qp + off}: {len(t['nodes'])} nodes from node {t['first_node']}  " +
                      "  ".join(f"{size}: {count} ({desc} descend)" for size, count, desc in tree_summary(t["nodes"])))
            union = [int(v) for v in row[0]["union_nodes"]]
            print(f"frame {f} union: {sum(union)} nodes evaluated for {sum(len(t['nodes']) for t in row)} nodes of {len(row)} trees  " +
                  "  ".join(f"{size}: {count}" for size, count in zip(SIZES, union) if size >= args.min_size))
        m.close()
        return 0
    if args.tree and args.frames is not None:
        for f, t in enumerate(run_trees(m, org, pred, args.poc, args.qp, args.min_size, args.motion_cfg)):
            save_tree(f"{args.out}_f{f}", t)
            print(f"frame {f} (poc {args.poc + f}): {len(t['nodes'])} nodes from node {t['first_node']}  " +
                  "  ".join(f"{size}: {count} ({desc} descend)" for size, count, desc in tree_summary(t["nodes"])))
        m.close()
        return 0
    if args.tree and args.tree_qp_list is not None:
        trees = run_tree_sweep(m, org, pred, args.poc, args.tree_qp_list, args.min_size, args.motion_cfg)
        for qp, t in zip(args.tree_qp_list, trees):
            save_tree(f"{args.out}_qp{qp}", t)
            print(f"qp {qp}: {len(t['nodes'])} nodes  " + "  ".join(f"{size}: {count} ({desc} descend)" for size, count, desc in tree_summary(t["nodes"])))
        union = [int(v) for v in trees[0]["union_nodes"]]
        print(f"union: {sum(union)} nodes evaluated for {sum(len(t['nodes']) for t in trees)} nodes of {len(trees)} trees  " +
              "  ".join(f"{size}: {count}" for size, count in zip(SIZES, union) if size >= args.min_size))
        m.close()
        return 0
    if args.tree:
        t = run_tree(m, org, pred, args.poc, args.qp, args.min_size, args.motion_cfg)
        save_tree(args.out, t)
        for size, count, desc in tree_summary(t["nodes"]):
            print(f"size {size}: {count} nodes, {desc} descend")
        print(f"tree: {len(t['nodes'])} nodes of at most {pkg.capi.tree_max_nodes(org.shape[1], org.shape[0], 128, args.min_size)}, "
              f"{int((t['leaf_map'] == 0xFF).sum())} of {t['leaf_map'].size} 16x16 blocks uncovered")
        m.close()
        return 0
    if args.qp_list is not None:
        sweeps = run_maps_sweep(m, org, pred, sizes, args.poc, args.qp_list, args.motion_cfg)
        maps = {(s, f"_qp{qp}"): r for s, per_qp in sweeps.items() for qp, r in per_qp.items()}
    else:
        maps = {(s, ""): r for s, r in run_maps(m, org, pred, sizes, args.poc, args.qp, args.motion_cfg).items()}
    for (s, tag), r in maps.items():
        for name in ("split", "confidence", "mask"):
            np.save(f"{args.out}_{s}{tag}_{name}.npy", r[name])
        classes = pkg.decisions.HEAD_CLASSES[s][pkg.decisions.default_head(s)]
        hist = " ".join(f"{k}:{v}" for k, v in sorted(histogram(r["split"], classes).items()))
        print(f"size {s}{tag.replace('_qp', ' qp ')}: {r['split'].size} CUs ({r['split'].shape[1]} x {r['split'].shape[0]})  split histogram  {hist}  "
              f"mean confidence {float(r['confidence'].mean()):.4f}")
    m.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
