"""ctypes binding of libmltcnn_hip.so (include/mltcnn.h) + the host-side mirror of the reference call site.

`MltCnn.predict(org, pred, poc, qp)` takes exactly what EncCu.cpp:806-830 reads at the call site
(two Pel planes with their strides, the slice POC and the CU QP) and returns what :921 produces
(`predictedSplitMode`).  There is NO fallback: a missing library raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

MLT_OK = 0
ERR_NAMES = {1: "MLT_ERR_ARG", 2: "MLT_ERR_NO_DEVICE", 3: "MLT_ERR_WEIGHTS", 4: "MLT_ERR_SIZE_DISABLED",
             5: "MLT_ERR_HIP", 6: "MLT_ERR_NOMEM"}
SIZE_BITS = {128: 1, 64: 2, 32: 4, 16: 8}
FLAG_EXACT_128 = 0x1   # 128x128 in exact (fp16 hi+lo, 3-pass) arithmetic instead of fast
FLAG_FAST_SMALL = 0x2  # 64/32/16 in fast arithmetic instead of exact
FLAG_DECISION_GUARD = 0x4  # ABI <= 3 opt-in; since ABI 4 the decision guard is the default (accepted, no effect)
FLAG_NO_FLAT_GUARD = 0x8   # fast arithmetic without the flat-content guard (measurement only)
FLAG_NO_CALIBRATION = 0x10  # keep the fast arithmetic whatever the weight set (measurement only)
FLAG_EXACT_LITE = 0x40  # round 5 (measurement): exact-configured sizes run the exact-lite arithmetic (FP8 cross terms)
FLAG_NO_MAGNITUDE_GUARD = 0x80  # round 6 (measurement): never admit a tier behind the magnitude guard
FLAG_NO_DECISION_GUARD = 0x20  # ABI 4: no exact re-evaluation of CUs with a near-tie on the decision head (measurement only)
EXPORTS = ["mlt_abi_version", "mlt_build_signature", "mlt_init", "mlt_num_devices", "mlt_device_ctx", "mlt_load_weights", "mlt_calibrate", "mlt_arithmetic", "mlt_predict", "mlt_predict_batch",
           "mlt_predict_batch_device", "mlt_submit", "mlt_flush", "mlt_wait", "mlt_synchronize", "mlt_set_stream", "mlt_alloc_pinned", "mlt_free_pinned",
           "mlt_num_logits", "mlt_profile_enable", "mlt_profile_read", "mlt_last_error", "mlt_shutdown",
           "mlt_set_confidence_gate", "mlt_get_confidence_gate", "mlt_predict_decision", "mlt_predict_batch_decisions", "mlt_predict_batch_device_decisions",
           "mlt_wait_decision",
           "mlt_set_candidate_policy", "mlt_get_candidate_policy", "mlt_predict_candidates", "mlt_predict_batch_candidates",
           "mlt_predict_batch_device_candidates", "mlt_wait_candidates",
           "mlt_picture_create", "mlt_picture_upload", "mlt_picture_wrap_device", "mlt_picture_destroy", "mlt_predict_at", "mlt_grid_positions",
           "mlt_tree_max_nodes", "mlt_tree_roots", "mlt_predict_tree", "mlt_predict_trees",
           "mlt_predict_batch_device_sweep", "mlt_predict_at_sweep", "mlt_predict_tree_sweep", "mlt_predict_trees_sweep",
           "mlt_motion_blocks", "mlt_picture_download", "mlt_picture_compensate", "mlt_picture_predict",
           "mlt_picture_compensate_refs", "mlt_picture_predict_refs",
           "mlt_debug_conv_table"]
MOTION_MAX_REFS = 4  # MLT_MOTION_MAX_REFS
SWEEP_MAX_QPS = 32  # MLT_SWEEP_MAX_QPS
TREES_MAX_PICTURES = 256  # MLT_TREES_MAX_PICTURES
TREE_BY_CANDIDATES = 0x1  # mlt_tree_config.flags: descend on cand_mask & descend_mask instead of on split_mode


class MltConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("weights_dir", C.c_char_p),
                ("size_mask", C.c_uint32), ("head_index", C.c_int32 * 4), ("max_batch", C.c_int32),
                ("flags", C.c_uint32), ("guard_margin", C.c_float), ("tolerance", C.c_float), ("reserved", C.c_uint32),
                ("n_devices", C.c_int32), ("devices", C.c_int32 * 8)]


class MltArithInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("exact", C.c_int32), ("calibrated", C.c_int32), ("calib_rms", C.c_float), ("calib_max", C.c_float),
                ("flat_guard", C.c_int32), ("decision_guard", C.c_int32), ("guard_reruns", C.c_uint64),
                ("w2_stages", C.c_int32), ("guard_margin", C.c_float), ("x_stages", C.c_int32), ("w2_units", C.c_int32), ("x_units", C.c_int32), ("rounding", C.c_int32),
                ("calib_cus", C.c_int32), ("calib_caller_cus", C.c_int32), ("mag_guard_thr", C.c_float), ("mag_guard_flagged", C.c_float),
                ("mag_guard_kind", C.c_int32)]


class MltDecision(C.Structure):
    """`struct mlt_decision` (include/mltcnn.h): 48 bytes, no padding."""
    _fields_ = [("split_mode", C.c_int32), ("raw_mode", C.c_int32), ("confidence", C.c_float), ("margin", C.c_float),
                ("level_mode", C.c_int32 * 4), ("level_conf", C.c_float * 4)]


# the same layout as a numpy structured dtype (what the batch calls return and decisions.from_logits builds)
DECISION_DTYPE = np.dtype([("split_mode", "<i4"), ("raw_mode", "<i4"), ("confidence", "<f4"), ("margin", "<f4"),
                           ("level_mode", "<i4", (4,)), ("level_conf", "<f4", (4,))])


class MltCandidates(C.Structure):
    """`struct mlt_candidates` (include/mltcnn.h): 40 bytes, no padding."""
    _fields_ = [("mask", C.c_uint32), ("count", C.c_int32), ("order", C.c_int8 * 8), ("prob", C.c_float * 6)]


CANDIDATES_DTYPE = np.dtype([("mask", "<u4"), ("count", "<i4"), ("order", "i1", (8,)), ("prob", "<f4", (6,))])


class MltTreeConfig(C.Structure):
    """`struct mlt_tree_config` (include/mltcnn.h): 40 bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("top_size", C.c_int32), ("min_size", C.c_int32), ("descend_mask", C.c_uint32 * 4), ("flags", C.c_uint32),
                ("poc", C.c_int32), ("qp", C.c_int32)]


class MltTreePicture(C.Structure):
    """`struct mlt_tree_picture` (include/mltcnn.h): 24 bytes -- one entry of mlt_predict_trees."""
    _fields_ = [("org", C.c_void_p), ("pred", C.c_void_p), ("poc", C.c_int32), ("qp", C.c_int32)]


class MltMotionConfig(C.Structure):
    """`struct mlt_motion_config` (include/mltcnn.h): 20 bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("block", C.c_int32), ("range", C.c_int32), ("lambda_", C.c_int32), ("flags", C.c_uint32)]


class MltMotionRefsConfig(C.Structure):
    """`struct mlt_motion_refs_config` (include/mltcnn.h): 24 bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("block", C.c_int32), ("range", C.c_int32), ("lambda_", C.c_int32), ("subpel", C.c_int32), ("flags", C.c_uint32)]


# `struct mlt_tree_node` (include/mltcnn.h): 32 bytes, no padding
TREE_NODE_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("size", "<i2"), ("depth", "i1"), ("flags", "u1"), ("parent", "<i4"), ("first_child", "<i4"),
                            ("split_mode", "<i4"), ("confidence", "<f4"), ("cand_mask", "<u4")])
assert TREE_NODE_DTYPE.itemsize == 32


class MltKernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint32), ("total_ms", C.c_float),
                ("flops", C.c_double), ("bytes", C.c_double)]


class MltError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


_LIB = None


def lib_path() -> str:
    return os.environ.get("MLT_LIB_PATH") or _build.LIB  # MLT_LIB_PATH: tuning variants only (scripts/sweep_cfg.py)


def load_library():
    """Loads the in-tree HIP library; raises if it has not been built (no silent fallback).

    torch is imported FIRST on purpose: in this image the working HIP runtime is the libamdhip64.so.7 bundled
    with PyTorch-ROCm; loading ours first would bind the system copy of the same soname and HIP init fails."""
    import torch  # noqa: F401
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950) first")
    lib = C.CDLL(path)
    vp, i32 = C.c_void_p, C.c_int
    lib.mlt_abi_version.restype = i32
    lib.mlt_build_signature.restype = C.c_char_p
    if "MLT_LIB_PATH" not in os.environ and os.path.isdir(_build.CSRC):
        # the binary travels to the GPU box with the snapshot: one built from other sources than the tree's must not pass for them
        have, want = lib.mlt_build_signature().decode(), _build.source_signature()
        if have != want:
            raise RuntimeError(f"{path} was built from sources {have}, the tree is {want}: rebuild (python __graft_entry__.py)")
    lib.mlt_init.argtypes = [C.POINTER(MltConfig), C.POINTER(vp)]
    lib.mlt_num_devices.argtypes = [vp]
    lib.mlt_device_ctx.argtypes = [vp, i32]
    lib.mlt_device_ctx.restype = vp
    lib.mlt_load_weights.argtypes = [vp, i32, vp, C.c_size_t]
    lib.mlt_arithmetic.argtypes = [vp, i32, C.POINTER(MltArithInfo)]
    lib.mlt_calibrate.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32]
    lib.mlt_predict.argtypes = [vp, vp, i32, vp, i32, i32, C.c_int32, C.c_int32, vp, vp]
    lib.mlt_predict_batch.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.mlt_predict_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.mlt_submit.argtypes = [vp, vp, i32, vp, i32, i32, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]
    lib.mlt_flush.argtypes = [vp, i32]
    lib.mlt_wait.argtypes = [vp, i32, C.c_uint64, vp, vp]
    lib.mlt_set_confidence_gate.argtypes = [vp, i32, C.c_float]
    lib.mlt_get_confidence_gate.argtypes = [vp, i32, C.POINTER(C.c_float)]
    lib.mlt_predict_decision.argtypes = [vp, vp, i32, vp, i32, i32, C.c_int32, C.c_int32, C.POINTER(MltDecision), vp]
    lib.mlt_predict_batch_decisions.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.mlt_predict_batch_device_decisions.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.mlt_wait_decision.argtypes = [vp, i32, C.c_uint64, C.POINTER(MltDecision), vp]
    lib.mlt_set_candidate_policy.argtypes = [vp, i32, C.c_float, i32]
    lib.mlt_get_candidate_policy.argtypes = [vp, i32, C.POINTER(C.c_float), C.POINTER(i32)]
    lib.mlt_predict_candidates.argtypes = [vp, vp, i32, vp, i32, i32, C.c_int32, C.c_int32, C.POINTER(MltCandidates), C.POINTER(MltDecision), vp]
    lib.mlt_predict_batch_candidates.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.mlt_predict_batch_device_candidates.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.mlt_wait_candidates.argtypes = [vp, i32, C.c_uint64, C.POINTER(MltCandidates), C.POINTER(MltDecision), vp]
    lib.mlt_picture_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
    lib.mlt_picture_upload.argtypes = [vp, vp, vp, i32]
    lib.mlt_picture_wrap_device.argtypes = [vp, vp, i32, i32, i32, C.POINTER(vp)]
    lib.mlt_picture_destroy.argtypes = [vp, vp]
    lib.mlt_predict_at.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.mlt_predict_batch_device_sweep.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.mlt_predict_at_sweep.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.mlt_grid_positions.argtypes = [i32, i32, i32, vp, i32]
    lib.mlt_tree_max_nodes.argtypes = [i32, i32, i32, i32]
    lib.mlt_tree_roots.argtypes = [i32, i32, i32, i32, vp, i32]
    lib.mlt_predict_tree.argtypes = [vp, vp, vp, C.POINTER(MltTreeConfig), vp, i32, C.POINTER(i32), vp, vp, i32, vp, vp]
    lib.mlt_predict_trees.argtypes = [vp, i32, C.POINTER(MltTreePicture), C.POINTER(MltTreeConfig), vp, i32, vp, vp, vp, i32, vp, vp]
    lib.mlt_predict_tree_sweep.argtypes = [vp, vp, vp, C.POINTER(MltTreeConfig), vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp]
    lib.mlt_predict_trees_sweep.argtypes = [vp, i32, C.POINTER(MltTreePicture), C.POINTER(MltTreeConfig), vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp]
    lib.mlt_motion_blocks.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.mlt_picture_download.argtypes = [vp, vp, vp, i32]
    lib.mlt_picture_compensate.argtypes = [vp, vp, C.POINTER(MltMotionConfig), vp, vp]
    lib.mlt_picture_predict.argtypes = [vp, vp, vp, C.POINTER(MltMotionConfig), vp, vp, vp]
    lib.mlt_picture_compensate_refs.argtypes = [vp, C.POINTER(vp), i32, C.POINTER(MltMotionRefsConfig), vp, vp, vp]
    lib.mlt_picture_predict_refs.argtypes = [vp, vp, C.POINTER(vp), i32, C.POINTER(MltMotionRefsConfig), vp, vp, vp, vp]
    lib.mlt_synchronize.argtypes = [vp]
    lib.mlt_set_stream.argtypes = [vp, vp]
    lib.mlt_alloc_pinned.restype = vp
    lib.mlt_alloc_pinned.argtypes = [C.c_size_t]
    lib.mlt_free_pinned.argtypes = [vp]
    lib.mlt_num_logits.argtypes = [i32]
    lib.mlt_profile_enable.argtypes = [vp, i32]
    lib.mlt_profile_read.argtypes = [vp, C.POINTER(MltKernelTime), i32]
    lib.mlt_last_error.restype = C.c_char_p
    lib.mlt_last_error.argtypes = [vp]
    lib.mlt_shutdown.argtypes = [vp]
    lib.mlt_shutdown.restype = None
    _LIB = lib
    return lib


def grid_positions(width: int, height: int, size: int) -> np.ndarray:
    """[count, 2] int32 {x, y} of the complete CUs on the size-aligned grid of a width x height picture, raster order (mlt_grid_positions; pure host)."""
    lib = load_library()
    count = lib.mlt_grid_positions(int(width), int(height), int(size), None, 0)
    xy = np.zeros((count, 2), np.int32)
    if count:
        assert lib.mlt_grid_positions(int(width), int(height), int(size), xy.ctypes.data, count) == count
    return xy


def tree_max_nodes(width: int, height: int, top: int = 128, min_size: int = 16) -> int:
    """Node count of a tree that descends everywhere: the capacity mlt_predict_tree asks for (mlt_tree_max_nodes; pure host, 0 on bad arguments)."""
    return load_library().mlt_tree_max_nodes(int(width), int(height), int(top), int(min_size))


def tree_roots(width: int, height: int, top: int, size: int) -> np.ndarray:
    """[count, 2] int32 {x, y}: the roots of level `size` of a tree whose top level is `top`, raster order (mlt_tree_roots; pure host)."""
    lib = load_library()
    count = lib.mlt_tree_roots(int(width), int(height), int(top), int(size), None, 0)
    xy = np.zeros((count, 2), np.int32)
    if count:
        assert lib.mlt_tree_roots(int(width), int(height), int(top), int(size), xy.ctypes.data, count) == count
    return xy


def motion_blocks(width: int, height: int, block: int = 16):
    """(bx, by) = the blocks per row and per column of a width x height picture cut into block x block blocks, border blocks clipped (mlt_motion_blocks; pure
    host); (0, 0) on bad arguments."""
    bx, by = C.c_int(0), C.c_int(0)
    n = load_library().mlt_motion_blocks(int(width), int(height), int(block), C.byref(bx), C.byref(by))
    return (bx.value, by.value) if n else (0, 0)


def motion_config(block: int = 16, search_range: int = 0, lam: int = 0, flags: int = 0) -> MltMotionConfig:
    cfg = MltMotionConfig()
    cfg.struct_size = C.sizeof(MltMotionConfig)
    cfg.block, cfg.range, cfg.lambda_, cfg.flags = int(block), int(search_range), int(lam), int(flags)
    return cfg


def motion_refs_config(block: int = 16, search_range: int = 0, lam: int = 0, subpel: int = 0, flags: int = 0) -> MltMotionRefsConfig:
    cfg = MltMotionRefsConfig()
    cfg.struct_size = C.sizeof(MltMotionRefsConfig)
    cfg.block, cfg.range, cfg.lambda_, cfg.subpel, cfg.flags = int(block), int(search_range), int(lam), int(subpel), int(flags)
    return cfg


def _picture_handles(pics):
    """A list of Pictures as the `const mlt_picture *const *` of the _refs calls."""
    return (C.c_void_p * max(len(pics), 1))(*[p._h for p in pics])


class Picture:
    """`mlt_picture`: one int16 luma plane in device memory, owned by the context it was made on (MltCnn.picture / MltCnn.wrap_picture)."""

    def __init__(self, ctx: "MltCnn", handle, width: int, height: int, keep=None):
        self._ctx, self._h, self.width, self.height = ctx, handle, width, height
        self._keep = keep   # a wrapped plane's owner (e.g. the torch tensor), so that it outlives the handle

    def upload(self, plane: np.ndarray):
        """plane: int16 [height, width] with unit column stride and any row stride (taken from the array): host -> every device of the context."""
        assert plane.dtype == np.int16 and plane.shape == (self.height, self.width) and plane.strides[1] == 2 and plane.strides[0] % 2 == 0
        self._ctx._check(self._ctx._lib.mlt_picture_upload(self._ctx._h, self._h, plane.ctypes.data, plane.strides[0] // 2))
        return self

    def download(self, out: np.ndarray | None = None) -> np.ndarray:
        """devices[0]'s plane -> int16 [height, width] (mlt_picture_download; after the context stream's earlier work, synchronous).  out: an int16 array of that
        shape with unit column stride and any row stride to fill instead of a new one."""
        if out is None:
            out = np.zeros((self.height, self.width), np.int16)
        assert out.dtype == np.int16 and out.shape == (self.height, self.width) and out.strides[1] == 2 and out.strides[0] % 2 == 0
        self._ctx._check(self._ctx._lib.mlt_picture_download(self._ctx._h, self._h, out.ctypes.data, out.strides[0] // 2))
        return out

    def close(self):
        if self._h and self._ctx._h:
            self._ctx._check(self._ctx._lib.mlt_picture_destroy(self._ctx._h, self._h))
        self._h = None


class MltCnn:
    """One context = one HIP device + one stream (one per encoder thread / EncCu instance)."""

    def __init__(self, device: int = 0, sizes=(128,), weights_dir: str | None = None, blobs: dict | None = None,
                 head_index: dict | None = None, max_batch: int = 4096, flags: int = 0, guard_margin: float = 0.0,
                 tolerance: float = 0.0, devices=None):
        """devices: list of HIP ordinals -> ONE context serving several GPUs (mlt_config.n_devices / devices[]); None: `device`."""
        self._lib = load_library()
        cfg = MltConfig()
        cfg.struct_size = C.sizeof(MltConfig)
        cfg.device = device
        if devices:
            cfg.n_devices = len(devices)
            for i, d in enumerate(devices):
                cfg.devices[i] = d
        cfg.weights_dir = weights_dir.encode() if weights_dir else None
        cfg.size_mask = sum(SIZE_BITS[s] for s in sizes)
        for i, s in enumerate((128, 64, 32, 16)):
            cfg.head_index[i] = (head_index or {}).get(s, -1)
        cfg.max_batch = max_batch
        cfg.flags = flags
        cfg.guard_margin = guard_margin
        cfg.tolerance = tolerance
        self._h = C.c_void_p()
        rc = self._lib.mlt_init(C.byref(cfg), C.byref(self._h))
        if rc != MLT_OK:
            raise MltError(rc, self._lib.mlt_last_error(None).decode())
        for s, blob in (blobs or {}).items():
            self.load_weights(s, blob)

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.mlt_shutdown(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != MLT_OK:
            raise MltError(rc, self._lib.mlt_last_error(self._h).decode())

    def load_weights(self, size: int, blob: bytes):
        buf = C.create_string_buffer(blob, len(blob))
        self._check(self._lib.mlt_load_weights(self._h, size, buf, len(blob)))

    def calibrate(self, size: int, org: np.ndarray, pred: np.ndarray, poc, qp, replace: bool = False):
        """Repeat the load-time calibration of `size` with the caller's CUs appended to (or replacing) the synthetic set (mlt_calibrate)."""
        org = np.ascontiguousarray(org, np.int16)
        pred = np.ascontiguousarray(pred, np.int16)
        poc = np.ascontiguousarray(poc, np.int32)
        qp = np.ascontiguousarray(qp, np.int32)
        n = org.shape[0]
        assert org.shape == (n, size, size) and pred.shape == org.shape and poc.shape == (n,) and qp.shape == (n,)
        self._check(self._lib.mlt_calibrate(self._h, size, org.ctypes.data, pred.ctypes.data, poc.ctypes.data, qp.ctypes.data, n, 1 if replace else 0))

    def arithmetic(self, size: int) -> dict:
        """Arithmetic the size runs after loading (fast / exact), what the calibration measured, guard activity."""
        info = MltArithInfo()
        info.struct_size = C.sizeof(MltArithInfo)
        self._check(self._lib.mlt_arithmetic(self._h, size, C.byref(info)))
        return {k: getattr(info, k) for k, _ in MltArithInfo._fields_ if k != "struct_size"}

    def num_devices(self) -> int:
        return self._lib.mlt_num_devices(self._h)

    def arithmetic_of_device(self, index: int, size: int) -> dict:
        info = MltArithInfo()
        info.struct_size = C.sizeof(MltArithInfo)
        h = self._lib.mlt_device_ctx(self._h, index)
        if not h:
            raise MltError(1, "no such device index")
        rc = self._lib.mlt_arithmetic(h, size, C.byref(info))
        if rc != MLT_OK:
            raise MltError(rc, self._lib.mlt_last_error(h).decode())
        return {k: getattr(info, k) for k, _ in MltArithInfo._fields_ if k != "struct_size"}

    def num_logits(self, size: int) -> int:
        return self._lib.mlt_num_logits(size)

    # -- the call site (EncCu.cpp:806-921) ---------------------------------------------------
    def predict(self, org: np.ndarray, pred: np.ndarray, poc: int, qp: int):
        """org / pred: int16 2-D views [S, S] with arbitrary positive row stride (picture buffers)."""
        assert org.dtype == np.int16 and pred.dtype == np.int16 and org.ndim == 2 and org.shape == pred.shape
        S = org.shape[0]
        assert org.shape[1] == S and org.strides[1] == 2 and pred.strides[1] == 2
        split = C.c_int32(-1)  # the reference's "inference failed" value (EncModeCtrl.cpp:147-148)
        logits = np.zeros(self.num_logits(S) or 1, np.float32)
        self._check(self._lib.mlt_predict(self._h, org.ctypes.data, org.strides[0] // 2, pred.ctypes.data,
                                          pred.strides[0] // 2, S, int(poc), int(qp), C.byref(split), logits.ctypes.data))
        return int(split.value), logits

    def predict_batch(self, org: np.ndarray, pred: np.ndarray, poc, qp, want_logits: bool = True):
        org = np.ascontiguousarray(org, np.int16)
        pred = np.ascontiguousarray(pred, np.int16)
        n, S, _ = org.shape
        poc = np.ascontiguousarray(poc, np.int32)
        qp = np.ascontiguousarray(qp, np.int32)
        split = np.full((n,), -1, np.int32)
        logits = np.zeros((n, self.num_logits(S) or 1), np.float32) if want_logits else None
        self._check(self._lib.mlt_predict_batch(self._h, n, S, org.ctypes.data, pred.ctypes.data, poc.ctypes.data,
                                                qp.ctypes.data, split.ctypes.data, logits.ctypes.data if want_logits else None))
        return split, logits

    def submit(self, org: np.ndarray, pred: np.ndarray, poc: int, qp: int) -> int:
        """Deferred single-CU prediction: stage one CU, return a ticket (see mlt_submit in include/mltcnn.h)."""
        assert org.dtype == np.int16 and pred.dtype == np.int16 and org.ndim == 2 and org.shape == pred.shape
        S = org.shape[0]
        assert org.shape[1] == S and org.strides[1] == 2 and pred.strides[1] == 2
        t = C.c_uint64(0)
        self._check(self._lib.mlt_submit(self._h, org.ctypes.data, org.strides[0] // 2, pred.ctypes.data, pred.strides[0] // 2,
                                         S, int(poc), int(qp), C.byref(t)))
        return int(t.value)

    def flush(self, size: int):
        self._check(self._lib.mlt_flush(self._h, size))

    def wait(self, size: int, ticket: int):
        split = C.c_int32(-1)
        logits = np.zeros(self.num_logits(size) or 1, np.float32)
        self._check(self._lib.mlt_wait(self._h, size, C.c_uint64(ticket), C.byref(split), logits.ctypes.data))
        return int(split.value), logits

    def predict_batch_device(self, n: int, size: int, d_org: int, d_pred: int, d_poc: int, d_qp: int, d_split: int | None,
                             d_logits: int | None, d_decisions: int | None = None, d_candidates: int | None = None):
        """Raw device pointers (e.g. torch tensor .data_ptr()); asynchronous on the context's stream.
        d_decisions: n x 48 bytes of device memory -> the decision records instead of the split modes (mlt_predict_batch_device_decisions).
        d_candidates: n x 40 bytes of device memory -> the candidate records, with the decision records beside them when d_decisions is given too
        (mlt_predict_batch_device_candidates)."""
        if d_candidates is not None:
            assert d_split is None, "one call fills either the split modes or the records"
            self._check(self._lib.mlt_predict_batch_device_candidates(self._h, n, size, d_org, d_pred, d_poc, d_qp, d_candidates, d_decisions, d_logits))
            return
        if d_decisions is not None:
            assert d_split is None, "one call fills either the split modes or the decision records"
            self._check(self._lib.mlt_predict_batch_device_decisions(self._h, n, size, d_org, d_pred, d_poc, d_qp, d_decisions, d_logits))
            return
        self._check(self._lib.mlt_predict_batch_device(self._h, n, size, d_org, d_pred, d_poc, d_qp, d_split, d_logits))

    def predict_batch_device_sweep(self, n: int, size: int, d_org: int, d_pred: int, d_poc: int, qps, d_split: int | None = None, d_logits: int | None = None,
                                   d_decisions: int | None = None, d_candidates: int | None = None):
        """QP sweep on raw device pointers (mlt_predict_batch_device_sweep): one trunk pass, the heads under every value of the HOST sequence `qps`.  Every output is
        device memory for len(qps) slabs of n CUs (element (q, i) at q * n + i); at least one of them; asynchronous on the context's stream like its twin."""
        qps = np.ascontiguousarray(qps, np.int32).reshape(-1)
        self._check(self._lib.mlt_predict_batch_device_sweep(self._h, n, size, d_org, d_pred, d_poc, qps.ctypes.data, qps.shape[0], d_split, d_logits, d_decisions, d_candidates))

    # -- per-level decisions with confidence, and the confidence gate ------------------------------
    def set_confidence_gate(self, size: int, min_confidence: float):
        """split = -1 unless the decision head's softmax probability reaches min_confidence (0 = off); every entry point, every device."""
        self._check(self._lib.mlt_set_confidence_gate(self._h, size, float(min_confidence)))

    def confidence_gate(self, size: int, device_index: int = 0) -> float:
        h = self._lib.mlt_device_ctx(self._h, device_index)
        if not h:
            raise MltError(1, "no such device index")
        v = C.c_float(-1.0)
        rc = self._lib.mlt_get_confidence_gate(h, size, C.byref(v))
        if rc != MLT_OK:
            raise MltError(rc, self._lib.mlt_last_error(h).decode())
        return float(v.value)

    @staticmethod
    def _record(d: MltDecision) -> np.ndarray:
        return np.frombuffer(bytes(d), DECISION_DTYPE)[0].copy()

    def predict_decision(self, org: np.ndarray, pred: np.ndarray, poc: int, qp: int):
        """`predict` returning the CU's decision record (a DECISION_DTYPE scalar) and the logits."""
        assert org.dtype == np.int16 and pred.dtype == np.int16 and org.ndim == 2 and org.shape == pred.shape
        S = org.shape[0]
        assert org.shape[1] == S and org.strides[1] == 2 and pred.strides[1] == 2
        d = MltDecision(-1, -1)
        logits = np.zeros(self.num_logits(S) or 1, np.float32)
        self._check(self._lib.mlt_predict_decision(self._h, org.ctypes.data, org.strides[0] // 2, pred.ctypes.data,
                                                   pred.strides[0] // 2, S, int(poc), int(qp), C.byref(d), logits.ctypes.data))
        return self._record(d), logits

    def predict_batch_decisions(self, org: np.ndarray, pred: np.ndarray, poc, qp, want_logits: bool = True):
        org = np.ascontiguousarray(org, np.int16)
        pred = np.ascontiguousarray(pred, np.int16)
        n, S, _ = org.shape
        poc = np.ascontiguousarray(poc, np.int32)
        qp = np.ascontiguousarray(qp, np.int32)
        dec = np.zeros((n,), DECISION_DTYPE)
        dec["split_mode"] = -1
        logits = np.zeros((n, self.num_logits(S) or 1), np.float32) if want_logits else None
        self._check(self._lib.mlt_predict_batch_decisions(self._h, n, S, org.ctypes.data, pred.ctypes.data, poc.ctypes.data,
                                                          qp.ctypes.data, dec.ctypes.data, logits.ctypes.data if want_logits else None))
        return dec, logits

    def wait_decision(self, size: int, ticket: int):
        d = MltDecision(-1, -1)
        logits = np.zeros(self.num_logits(size) or 1, np.float32)
        self._check(self._lib.mlt_wait_decision(self._h, size, C.c_uint64(ticket), C.byref(d), logits.ctypes.data))
        return self._record(d), logits

    # -- candidate split sets ----------------------------------------------------------------------
    def set_candidate_policy(self, size: int, coverage: float, max_modes: int = 0):
        """The candidate record keeps the shortest rank prefix of the decision head that carries `coverage` of the softmax probability, every class when
        that takes more than max_modes > 0 classes ((0, 0) = the argmax alone, the default); every entry point, every device."""
        self._check(self._lib.mlt_set_candidate_policy(self._h, size, float(coverage), int(max_modes)))

    def candidate_policy(self, size: int, device_index: int = 0):
        h = self._lib.mlt_device_ctx(self._h, device_index)
        if not h:
            raise MltError(1, "no such device index")
        cov, mx = C.c_float(-1.0), C.c_int(-1)
        rc = self._lib.mlt_get_candidate_policy(h, size, C.byref(cov), C.byref(mx))
        if rc != MLT_OK:
            raise MltError(rc, self._lib.mlt_last_error(h).decode())
        return float(cov.value), int(mx.value)

    @staticmethod
    def _candidates(c: MltCandidates) -> np.ndarray:
        return np.frombuffer(bytes(c), CANDIDATES_DTYPE)[0].copy()

    def predict_candidates(self, org: np.ndarray, pred: np.ndarray, poc: int, qp: int):
        """`predict` returning the CU's candidate record (a CANDIDATES_DTYPE scalar), its decision record and the logits."""
        assert org.dtype == np.int16 and pred.dtype == np.int16 and org.ndim == 2 and org.shape == pred.shape
        S = org.shape[0]
        assert org.shape[1] == S and org.strides[1] == 2 and pred.strides[1] == 2
        c, d = MltCandidates(), MltDecision(-1, -1)
        logits = np.zeros(self.num_logits(S) or 1, np.float32)
        self._check(self._lib.mlt_predict_candidates(self._h, org.ctypes.data, org.strides[0] // 2, pred.ctypes.data,
                                                     pred.strides[0] // 2, S, int(poc), int(qp), C.byref(c), C.byref(d), logits.ctypes.data))
        return self._candidates(c), self._record(d), logits

    def predict_batch_candidates(self, org: np.ndarray, pred: np.ndarray, poc, qp, want_logits: bool = True, want_decisions: bool = True):
        org = np.ascontiguousarray(org, np.int16)
        pred = np.ascontiguousarray(pred, np.int16)
        n, S, _ = org.shape
        poc = np.ascontiguousarray(poc, np.int32)
        qp = np.ascontiguousarray(qp, np.int32)
        cand = np.zeros((n,), CANDIDATES_DTYPE)
        dec = np.zeros((n,), DECISION_DTYPE) if want_decisions else None
        logits = np.zeros((n, self.num_logits(S) or 1), np.float32) if want_logits else None
        self._check(self._lib.mlt_predict_batch_candidates(self._h, n, S, org.ctypes.data, pred.ctypes.data, poc.ctypes.data, qp.ctypes.data,
                                                           cand.ctypes.data, dec.ctypes.data if want_decisions else None,
                                                           logits.ctypes.data if want_logits else None))
        return cand, dec, logits

    def wait_candidates(self, size: int, ticket: int):
        c, d = MltCandidates(), MltDecision(-1, -1)
        logits = np.zeros(self.num_logits(size) or 1, np.float32)
        self._check(self._lib.mlt_wait_candidates(self._h, size, C.c_uint64(ticket), C.byref(c), C.byref(d), logits.ctypes.data))
        return self._candidates(c), self._record(d), logits

    # -- device-resident pictures ------------------------------------------------------------------
    def picture(self, width: int, height: int) -> Picture:
        """A library-owned plane on every device of the context (mlt_picture_create); fill it with Picture.upload."""
        h = C.c_void_p()
        self._check(self._lib.mlt_picture_create(self._h, int(width), int(height), C.byref(h)))
        return Picture(self, h, int(width), int(height))

    def wrap_picture(self, ptr: int, stride: int, width: int, height: int, keep=None) -> Picture:
        """A plane the caller holds in device memory (e.g. torch tensor .data_ptr()), stride in elements; no copy (mlt_picture_wrap_device)."""
        h = C.c_void_p()
        self._check(self._lib.mlt_picture_wrap_device(self._h, ptr, int(stride), int(width), int(height), C.byref(h)))
        return Picture(self, h, int(width), int(height), keep)

    # -- prediction pictures: block motion search + compensation on the device -------------------------
    def compensate(self, ref_pic: Picture, mv, dst_pic: Picture, block: int = 16):
        """dst_pic <- the quarter-sample compensation of ref_pic with the field mv, int16 [by, bx, 2] {mvx, mvy} (mlt_picture_compensate; motion.compensate is the
        rule).  Returns once mv may be reused."""
        mv = np.ascontiguousarray(mv, np.int16)
        bx, by = motion_blocks(dst_pic.width, dst_pic.height, block or 16)
        assert (bx, by) == (0, 0) or mv.shape == (by, bx, 2), (mv.shape, (by, bx, 2))   # (a bad block: the library's error)
        cfg = motion_config(block)
        self._check(self._lib.mlt_picture_compensate(self._h, ref_pic._h, C.byref(cfg), mv.ctypes.data, dst_pic._h))
        return dst_pic

    def predict_picture(self, cur_pic: Picture, ref_pic: Picture, dst_pic: Picture, block: int = 16, search_range: int = 16, lam: int = 0,
                        want_field: bool = True) -> dict:
        """dst_pic <- the prediction of cur_pic from ref_pic: integer-sample block search, then compensation (mlt_picture_predict; motion.search and
        motion.compensate are the rule).  want_field: -> {"mv": int16 [by, bx, 2], "cost": uint32 [by, bx]} and the call is synchronous; else {} and it returns
        after enqueueing -- later calls on this context see dst_pic in stream order."""
        cfg = motion_config(block, search_range, lam)
        out = {}
        if want_field:
            bx, by = motion_blocks(dst_pic.width, dst_pic.height, block or 16)
            out = {"mv": np.zeros((by, bx, 2), np.int16), "cost": np.zeros((by, bx), np.uint32)}
        self._check(self._lib.mlt_picture_predict(self._h, cur_pic._h, ref_pic._h, C.byref(cfg), dst_pic._h,
                                                  out["mv"].ctypes.data if want_field else None, out["cost"].ctypes.data if want_field else None))
        return out

    def compensate_refs(self, ref_pics, mv, ref_idx, dst_pic: Picture, block: int = 16):
        """dst_pic <- block by block the compensation of ref_pics[ref_idx[block]] with the field mv (mlt_picture_compensate_refs; motion.compensate_refs is the
        rule).  ref_idx: uint8 [by, bx], or None for reference 0 everywhere.  Returns once mv and ref_idx may be reused."""
        mv = np.ascontiguousarray(mv, np.int16)
        bx, by = motion_blocks(dst_pic.width, dst_pic.height, block or 16)
        assert (bx, by) == (0, 0) or mv.shape == (by, bx, 2), (mv.shape, (by, bx, 2))   # (a bad block: the library's error)
        if ref_idx is not None:
            ref_idx = np.ascontiguousarray(ref_idx, np.uint8)
            assert (bx, by) == (0, 0) or ref_idx.shape == (by, bx), (ref_idx.shape, (by, bx))
        cfg = motion_refs_config(block)
        self._check(self._lib.mlt_picture_compensate_refs(self._h, _picture_handles(ref_pics), len(ref_pics), C.byref(cfg), mv.ctypes.data,
                                                          None if ref_idx is None else ref_idx.ctypes.data, dst_pic._h))
        return dst_pic

    def predict_picture_refs(self, cur_pic: Picture, ref_pics, dst_pic: Picture, block: int = 16, search_range: int = 16, lam: int = 0, subpel: int = 2,
                             want_field: bool = True) -> dict:
        """dst_pic <- the prediction of cur_pic from up to MOTION_MAX_REFS references: an integer search per reference, the quarter-sample refinement of each
        winner (subpel 0 / 1 / 2: integer / half / quarter window) and the per-block choice among them, then compensation (mlt_picture_predict_refs;
        motion.predict_refs is the rule).  want_field: -> {"mv": int16 [by, bx, 2], "ref": uint8 [by, bx], "cost": uint32 [by, bx] (cost_q)} and the call is
        synchronous; else {} and it returns after enqueueing -- later calls on this context see dst_pic in stream order."""
        cfg = motion_refs_config(block, search_range, lam, subpel)
        out = {}
        if want_field:
            bx, by = motion_blocks(dst_pic.width, dst_pic.height, block or 16)
            out = {"mv": np.zeros((by, bx, 2), np.int16), "ref": np.zeros((by, bx), np.uint8), "cost": np.zeros((by, bx), np.uint32)}
        self._check(self._lib.mlt_picture_predict_refs(self._h, cur_pic._h, _picture_handles(ref_pics), len(ref_pics), C.byref(cfg), dst_pic._h,
                                                       out["mv"].ctypes.data if want_field else None, out["ref"].ctypes.data if want_field else None,
                                                       out["cost"].ctypes.data if want_field else None))
        return out

    def predict_at(self, size: int, org_pic: Picture, pred_pic: Picture, xy, poc, qp, want=("split", "logits", "decisions", "candidates")) -> dict:
        """CUs of size x size at xy[i] = (x, y) of the picture pair (mlt_predict_at) -> {name: array} for the names in `want`."""
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        n = xy.shape[0]
        poc = np.ascontiguousarray(poc, np.int32)
        qp = np.ascontiguousarray(qp, np.int32)
        assert poc.shape == (n,) and qp.shape == (n,) and set(want) <= {"split", "logits", "decisions", "candidates"}
        out = {}
        if "split" in want:
            out["split"] = np.full((n,), -1, np.int32)
        if "logits" in want:
            out["logits"] = np.zeros((n, self.num_logits(size) or 1), np.float32)
        if "decisions" in want:
            out["decisions"] = np.zeros((n,), DECISION_DTYPE)
            out["decisions"]["split_mode"] = -1
        if "candidates" in want:
            out["candidates"] = np.zeros((n,), CANDIDATES_DTYPE)
        ptr = lambda k: out[k].ctypes.data if k in out else None
        self._check(self._lib.mlt_predict_at(self._h, int(size), org_pic._h, pred_pic._h, n, xy.ctypes.data, poc.ctypes.data, qp.ctypes.data,
                                             ptr("split"), ptr("logits"), ptr("decisions"), ptr("candidates")))
        return out

    def predict_at_sweep(self, size: int, org_pic: Picture, pred_pic: Picture, xy, poc, qps, want=("split", "logits", "decisions", "candidates")) -> dict:
        """predict_at under every value of `qps` from ONE network pass (mlt_predict_at_sweep) -> {name: array with a leading [len(qps)] axis} for the names in
        `want`; slab q is predict_at's result with every qp = qps[q], byte for byte."""
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        n = xy.shape[0]
        poc = np.ascontiguousarray(poc, np.int32)
        qps = np.ascontiguousarray(qps, np.int32).reshape(-1)
        Q = qps.shape[0]
        assert poc.shape == (n,) and set(want) <= {"split", "logits", "decisions", "candidates"}
        out = {}
        if "split" in want:
            out["split"] = np.full((Q, n), -1, np.int32)
        if "logits" in want:
            out["logits"] = np.zeros((Q, n, self.num_logits(size) or 1), np.float32)
        if "decisions" in want:
            out["decisions"] = np.zeros((Q, n), DECISION_DTYPE)
            out["decisions"]["split_mode"] = -1
        if "candidates" in want:
            out["candidates"] = np.zeros((Q, n), CANDIDATES_DTYPE)
        ptr = lambda k: out[k].ctypes.data if k in out else None
        self._check(self._lib.mlt_predict_at_sweep(self._h, int(size), org_pic._h, pred_pic._h, n, xy.ctypes.data, poc.ctypes.data, qps.ctypes.data, Q,
                                                   ptr("split"), ptr("logits"), ptr("decisions"), ptr("candidates")))
        return out

    @staticmethod
    def _tree_config(top, min_size, descend, by_candidates, poc=0, qp=0) -> MltTreeConfig:
        cfg = MltTreeConfig()
        cfg.struct_size = C.sizeof(MltTreeConfig)
        cfg.top_size, cfg.min_size, cfg.poc, cfg.qp = int(top), int(min_size), int(poc), int(qp)
        cfg.flags = TREE_BY_CANDIDATES if by_candidates else 0
        for i, s in enumerate((128, 64, 32, 16)):
            cfg.descend_mask[i] = int((descend or {}).get(s, 0))
        return cfg

    @staticmethod
    def _tree_outputs(want, cap: int, map_shape):
        """-> the zeroed arrays named in `want` (`cap` rows per node array, one leaf map of map_shape) and the pointer-or-None of a name."""
        assert set(want) <= {"leaf_map", "logits", "decisions", "candidates"}
        rows = max(cap, 1)
        shapes = {"leaf_map": (map_shape, np.uint8), "logits": ((rows, 15), np.float32), "decisions": ((rows,), DECISION_DTYPE), "candidates": ((rows,), CANDIDATES_DTYPE)}
        out = {k: np.zeros(*shapes[k]) for k in shapes if k in want}
        return out, lambda k: out[k].ctypes.data if k in out else None

    @staticmethod
    def _tree_entries(pairs, poc, qp):
        """-> the pairs as a list and the MltTreePicture array of a several-pair call (poc / qp: one int for all pairs or one per pair)."""
        pairs = list(pairs)
        P = len(pairs)
        poc = np.broadcast_to(np.asarray(poc, np.int32), (P,))
        qp = np.broadcast_to(np.asarray(qp, np.int32), (P,))
        entries = (MltTreePicture * max(P, 1))()
        for i, (o, q) in enumerate(pairs):
            entries[i].org, entries[i].pred, entries[i].poc, entries[i].qp = o._h, q._h, int(poc[i]), int(qp[i])
        return pairs, entries

    @staticmethod
    def _tree_slices(first, nodes, out, union=None, per_union: int = 1) -> list:
        """The arrays of a batched tree call cut into one dict per tree: slice s is nodes [first[s], first[s + 1]), map s and the same rows of the per-node arrays
        (all copies) + "union_nodes": row s // per_union of `union`, where the call has one."""
        res = []
        for s in range(len(first) - 1):
            lo, hi = int(first[s]), int(first[s + 1])
            r = {"nodes": nodes[lo:hi].copy(), "first_node": lo}
            if union is not None:
                r["union_nodes"] = union[s // per_union].copy()
            if "leaf_map" in out:
                r["leaf_map"] = out["leaf_map"][s].copy()
            for k in ("logits", "decisions", "candidates"):
                if k in out:
                    r[k] = out[k][lo:hi].copy()
            res.append(r)
        return res

    def predict_tree(self, org_pic: Picture, pred_pic: Picture, poc: int, qp: int, top: int = 128, min_size: int = 16, descend: dict | None = None,
                     by_candidates: bool = False, want=("leaf_map",)) -> dict:
        """The partition tree of the picture pair (mlt_predict_tree): quadtree descent on the device from `top` down to `min_size`.
        descend: {size: mask of the decision head's classes that mean "quad split"} (default 1 << 1 everywhere).
        -> {"nodes": TREE_NODE_DTYPE [n] in the contract's order} + for the names in `want`: "leaf_map" uint8 [height // 16, width // 16],
        "logits" float32 [n, 15] (a 128 node fills the first 9 of its row, the rest stays 0), "decisions", "candidates" (one record per node)."""
        cfg = self._tree_config(top, min_size, descend, by_candidates, poc, qp)
        cap = tree_max_nodes(org_pic.width, org_pic.height, top, min_size)
        nodes = np.zeros((max(cap, 1),), TREE_NODE_DTYPE)
        out, ptr = self._tree_outputs(want, cap, (org_pic.height // 16, org_pic.width // 16))
        n = C.c_int(0)
        self._check(self._lib.mlt_predict_tree(self._h, org_pic._h, pred_pic._h, C.byref(cfg), nodes.ctypes.data, cap, C.byref(n), ptr("leaf_map"),
                                               ptr("logits"), 15, ptr("decisions"), ptr("candidates")))
        out["nodes"] = nodes[:n.value].copy()
        for k in ("logits", "decisions", "candidates"):
            if k in out:
                out[k] = out[k][:n.value].copy()
        return out

    def predict_trees(self, pairs, poc, qp, top: int = 128, min_size: int = 16, descend: dict | None = None, by_candidates: bool = False,
                      want=("leaf_map",)) -> list:
        """The partition trees of several picture pairs of one geometry in ONE descent (mlt_predict_trees).  pairs: [(org_pic, pred_pic), ...]; poc / qp: one int
        for all pairs or one per pair; the other arguments as predict_tree.
        -> one dict per pair, shaped like predict_tree's ("logits" rows are zero beyond the size's logit count) + "first_node": the pair's first index in the call's
        node array."""
        pairs, entries = self._tree_entries(pairs, poc, qp)
        P = len(pairs)
        cfg = self._tree_config(top, min_size, descend, by_candidates)
        w, h = (pairs[0][0].width, pairs[0][0].height) if P else (0, 0)
        cap = P * tree_max_nodes(w, h, top, min_size)
        nodes = np.zeros((max(cap, 1),), TREE_NODE_DTYPE)
        first = np.zeros((P + 1,), np.int32)
        out, ptr = self._tree_outputs(want, cap, (max(P, 1), h // 16, w // 16))
        self._check(self._lib.mlt_predict_trees(self._h, P, entries, C.byref(cfg), nodes.ctypes.data, cap, first.ctypes.data, ptr("leaf_map"),
                                                ptr("logits"), 15, ptr("decisions"), ptr("candidates")))
        return self._tree_slices(first, nodes, out)

    def predict_tree_sweep(self, org_pic: Picture, pred_pic: Picture, poc: int, qps, top: int = 128, min_size: int = 16, descend: dict | None = None,
                           by_candidates: bool = False, want=("leaf_map",)) -> list:
        """The partition trees of ONE picture pair under every value of `qps` from one descent over the union of the trees (mlt_predict_tree_sweep); the other
        arguments as predict_tree.
        -> one dict per point, shaped like predict_trees' ("nodes", "first_node" and the wanted arrays) + "union_nodes": int32 [4], the nodes the network
        evaluated per level from `top` down (the same array in every dict)."""
        qps = np.ascontiguousarray(qps, np.int32).reshape(-1)
        Q = qps.shape[0]
        cfg = self._tree_config(top, min_size, descend, by_candidates, poc, 0)
        w, h = org_pic.width, org_pic.height
        cap = Q * tree_max_nodes(w, h, top, min_size)
        nodes = np.zeros((max(cap, 1),), TREE_NODE_DTYPE)
        first = np.zeros((Q + 1,), np.int32)
        union = np.zeros((4,), np.int32)
        out, ptr = self._tree_outputs(want, cap, (max(Q, 1), h // 16, w // 16))
        self._check(self._lib.mlt_predict_tree_sweep(self._h, org_pic._h, pred_pic._h, C.byref(cfg), qps.ctypes.data, Q, nodes.ctypes.data, cap, first.ctypes.data,
                                                     union.ctypes.data, ptr("leaf_map"), ptr("logits"), 15, ptr("decisions"), ptr("candidates")))
        return self._tree_slices(first, nodes, out, union[None], max(Q, 1))

    def predict_trees_sweep(self, pairs, poc, qp_offset, qps, top: int = 128, min_size: int = 16, descend: dict | None = None, by_candidates: bool = False,
                            want=("leaf_map",)) -> list:
        """The partition trees of several picture pairs of one geometry under every value of `qps` each, from ONE descent over the unions of all entries
        (mlt_predict_trees_sweep).  pairs: [(org_pic, pred_pic), ...]; poc / qp_offset: one int for all pairs or one per pair -- entry p under point q runs at
        qp_offset[p] + qps[q]; the other arguments as predict_tree.
        -> result[p][q]: a dict shaped like predict_tree_sweep's; "union_nodes" is entry p's int32 [4]."""
        pairs, entries = self._tree_entries(pairs, poc, qp_offset)
        P = len(pairs)
        qps = np.ascontiguousarray(qps, np.int32).reshape(-1)
        Q = qps.shape[0]
        cfg = self._tree_config(top, min_size, descend, by_candidates)
        w, h = (pairs[0][0].width, pairs[0][0].height) if P else (0, 0)
        cap = P * Q * tree_max_nodes(w, h, top, min_size)
        nodes = np.zeros((max(cap, 1),), TREE_NODE_DTYPE)
        first = np.zeros((P * Q + 1,), np.int32)
        union = np.zeros((max(P, 1), 4), np.int32)
        out, ptr = self._tree_outputs(want, cap, (max(P * Q, 1), h // 16, w // 16))
        self._check(self._lib.mlt_predict_trees_sweep(self._h, P, entries, C.byref(cfg), qps.ctypes.data, Q, nodes.ctypes.data, cap, first.ctypes.data, union.ctypes.data,
                                                      ptr("leaf_map"), ptr("logits"), 15, ptr("decisions"), ptr("candidates")))
        flat = self._tree_slices(first, nodes, out, union, max(Q, 1))
        return [flat[p * Q:(p + 1) * Q] for p in range(P)]

    def synchronize(self):
        self._check(self._lib.mlt_synchronize(self._h))

    def set_stream(self, hip_stream: int):
        self._check(self._lib.mlt_set_stream(self._h, hip_stream))

    def profile_enable(self, on: bool = True):
        self._check(self._lib.mlt_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        arr = (MltKernelTime * 64)()
        k = self._lib.mlt_profile_read(self._h, arr, 64)
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms,
                     flops=arr[i].flops, bytes=arr[i].bytes) for i in range(max(k, 0))]
