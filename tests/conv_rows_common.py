"""Shared by tests/test_conv_table_cpu.py and tests/test_conv_rows_gpu.py: the fixed matrix of small calls that puts every row of the per-conv kernels' launch
table (csrc/mlt_kernels.hip, kRows; as text: mlt_debug_conv_table) the dispatcher can reach on the device at least once.

The dispatcher's tuning switches are read once per process, so the cases are grouped by ENVIRONMENT and every environment runs in a fresh child process
(`python tests/conv_rows_common.py plan|run <env> ...`: started, never exec'd).  A case is (size, n, tier, w2_units, x_units) in the terms of mlt_plan_describe;
on the device the same state is set up through the public flags (tier 0 / 1 / 5) or, for the hi+lo-weights masks of the 128 model, by forcing the calibration's
stage mask (MLT_W2_MASK) -- mlt_arithmetic must then report exactly the case's unit masks.  Calibration (but for the forced masks) and all guards are off: every logit
comes from the launches of the plan.

n is the smallest CU count whose plan still selects the rows of the case (worked out from the plan records over n = 1 .. 513); two larger fast-arithmetic
batches run the throughput rows on more than one workgroup per cout tile."""
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_rows.npz")
TABLE = os.path.join(ROOT, "tests", "golden", "conv_launch_table.txt")

ENVS = {  # name -> dispatcher switches (MLT_TUNING=1 alone changes nothing)
    "fused": {"MLT_TUNING": "1"},
    "tiled": {"MLT_TUNING": "1", "MLT_NO_BLOCK_FUSION": "1"},
    "tiled_nolat": {"MLT_TUNING": "1", "MLT_NO_BLOCK_FUSION": "1", "MLT_LAT_PIXELS": "0"},
}
# (env, size, n, tier, w2_units, x_units)
CASES = [
    ("fused", 32, 1, 0, 0, 0), ("fused", 64, 1, 1, 0, 0), ("fused", 64, 1, 5, 0, 0), ("fused", 16, 1, 0, 0, 0), ("fused", 16, 1, 1, 0, 0),
    ("fused", 128, 1, 0, 0xC, 0), ("fused", 128, 17, 1, 0, 0), ("fused", 128, 17, 5, 0, 0),
    ("tiled", 128, 1, 0, 0x3, 0), ("tiled", 128, 17, 0, 0, 0),
    ("tiled_nolat", 128, 1, 0, 0x30, 0), ("tiled_nolat", 128, 1, 0, 0xC0, 0), ("tiled_nolat", 128, 1, 1, 0, 0), ("tiled_nolat", 128, 1, 5, 0, 0),
    ("tiled_nolat", 128, 70, 0, 0, 0),
]
# Rows of the table no context can launch.  Only one is left, and it stays in the table because the host reads the layer's packing from it (mlt_conv_cfg) and the
# layer's hi+lo-weights row is derived from it (add_fast); every other row is launched by the cases above.
UNREACHABLE = {
    # 64->128 stride 2, fast, throughput tiling: only the 128 model has the layer, on 16 x 16 output maps, where run_conv picks the latency row (small launches) or the
    # ring-DMA row (hout >= 8) -- never neither
    "mfma<64,128,2,9,1,32,1,2,1,2,4,2,2,5,1,0,0,0>",
}
_NSPLIT = {"single pass": 1, "exact": 2, "hi+lo weights": 4, "exact-lite": 6}


def load_table(text):
    """{key: kernel} of the accepted lines ("conv <key>: <kernel> threads=..."), and the list of the rejected keys"""
    rows, rejected = {}, []
    for line in text.splitlines():
        if not line.startswith("conv "):
            continue
        key, rest = line[5:].split(": ", 1)
        if rest == "rejected":
            rejected.append(key)
        else:
            rows[key] = rest.split(" threads=")[0]
    return rows, rejected


def plan_keys(lines):
    """The table keys of a plan's per-conv launches ("conv3x3_s<stride>_<cin>to<cout>_h<h>[+sc] [<arithmetic>, <variant>, ...]")"""
    keys = set()
    for line in lines:
        m = re.match(r"conv3x3_s(\d)_(\d+)to(\d+)_h\d+(?:\+sc)? \[([^,\]]+)(.*)\]", line)
        if not m:
            continue
        rest = m.group(5)
        variant = "centre" if "centre tap" in rest else "latency" if "latency tiles" in rest else "dma" if "LDS-DMA" in rest else "default"
        keys.add(f"{m.group(2)}->{m.group(3)} s{m.group(1)} nsplit={_NSPLIT[m.group(4)]} {variant}")
    return sorted(keys)


def _pkg():
    sys.path.insert(0, ROOT)
    import mltcnn_pkg
    return mltcnn_pkg.load()


def plan_main(env):
    """-> JSON {case index: [table keys of the case's plan]} for the cases of `env` (host only)"""
    pkg = _pkg()
    lib = pkg.capi.load_library()
    lib.mlt_plan_describe.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(1 << 16)
    out = {}
    for i, (e, size, n, tier, w2, x) in enumerate(CASES):
        if e != env:
            continue
        blob = pkg.weights.synthetic_blob(pkg.synth.arch_for_size(size), 10)
        k = lib.mlt_plan_describe(blob, len(blob), size, n, tier, w2, x, 1, buf, 1 << 16)
        assert k > 0, (CASES[i], k)
        out[i] = plan_keys(buf.value.decode().splitlines())
    print(json.dumps(out))


def _flags(F, size, tier, w2):
    f = F.FLAG_NO_FLAT_GUARD | F.FLAG_NO_DECISION_GUARD | F.FLAG_NO_MAGNITUDE_GUARD
    if not w2:
        f |= F.FLAG_NO_CALIBRATION  # (a forced mask goes through the calibration's tier search)
    if tier in (1, 5) and size == 128:
        f |= F.FLAG_EXACT_128
    if tier == 0 and size != 128:
        f |= F.FLAG_FAST_SMALL
    if tier == 5:
        f |= F.FLAG_EXACT_LITE
    return f


def run_main(env, out_path):
    """The cases of `env` on device 0 -> npz {"c<i>_logits", "c<i>_split", "c<i>_arith" = (exact, w2_units, x_units)}"""
    import numpy as np
    pkg = _pkg()
    F = pkg.capi
    res = {}
    for i, (e, size, n, tier, w2, x) in enumerate(CASES):
        if e != env:
            continue
        assert x == 0
        os.environ.pop("MLT_W2_MASK", None)
        if w2:  # unit mask -> stage mask (two launch units per stage)
            stages = sum(1 << s for s in range(4) if (w2 >> (2 * s)) & 3)
            assert sum(3 << (2 * s) for s in range(4) if (stages >> s) & 1) == w2
            os.environ["MLT_W2_MASK"] = str(stages)
        blob = pkg.weights.synthetic_blob(pkg.synth.arch_for_size(size), 10)
        m = pkg.MltCnn(device=0, sizes=(size,), blobs={size: blob}, flags=_flags(F, size, tier, w2))
        a = m.arithmetic(size)
        org, pred = pkg.synth.make_patches(size, n, 4100 + i)
        poc, qp = pkg.synth.make_scalars(n, 4100 + i)
        split, logits = m.predict_batch(org, pred, poc, qp)
        m.close()
        res[f"c{i}_logits"] = logits
        res[f"c{i}_split"] = np.asarray(split, np.int32)
        res[f"c{i}_arith"] = np.array([a["exact"], a["w2_units"], a["x_units"]], np.int32)
        print(f"case {i} {CASES[i]}: arithmetic {a['exact']} w2_units {a['w2_units']:#x} x_units {a['x_units']:#x}, logits[0] {logits[0][:3]}", flush=True)
    np.savez(out_path, **res)


if __name__ == "__main__":
    if sys.argv[1] == "plan":
        plan_main(sys.argv[2])
    else:
        run_main(sys.argv[2], sys.argv[3])
