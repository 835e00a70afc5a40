#!/usr/bin/env python3
"""What a QP sweep saves over one call per QP (kernel table: `sweep_heads_kernel`).

One process, one context with all four sizes, seed-10 weights, flags = 0.  A 1920 x 1080 frame of natural patches (synth.natural_patches laid out on the 128
grid, the right and bottom border filled from further patches) as a resident picture pair; per size the complete CUs of its size-aligned grid, Q = 4 points
(22, 27, 32, 37):
  leg A  four mlt_predict_at calls, one per QP (what a caller does without the sweep)
  leg B  one mlt_predict_at_sweep call
Both legs fetch split modes and logits.  Legs alternate step by step; the medians of the timed steps are reported per size and for the frame (the four grids
one after the other), with the CUs each leg re-evaluated exactly (guard_reruns) and whether every slab equals its twin's bytes.

  python scripts/qp_sweep_ab.py [--steps 24] [--warmup 6] > profiles/qp_sweep_ab.txt"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QPS = (22, 27, 32, 37)
SIZES = (128, 64, 32, 16)
WIDTH, HEIGHT = 1920, 1080


def natural_frame(pkg, seed: int):
    """-> (org, pred) int16 [HEIGHT, WIDTH]: natural 128 x 128 patches on the 128 grid, cropped at the border."""
    cols, rows = -(-WIDTH // 128), -(-HEIGHT // 128)
    org, pred = pkg.synth.natural_patches(128, cols * rows, seed)
    lay = lambda a: np.ascontiguousarray(a.reshape(rows, cols, 128, 128).transpose(0, 2, 1, 3).reshape(rows * 128, cols * 128)[:HEIGHT, :WIDTH])
    return lay(org), lay(pred)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--weight-seed", type=int, default=10)
    a = ap.parse_args()
    assert a.steps >= 20 and a.warmup >= 5
    import torch
    import mltcnn_pkg
    pkg = mltcnn_pkg.load()
    assert torch.cuda.is_available(), "needs an MI355X (no CPU fallback)"
    pkg.build.build_lib()
    blobs = {s: pkg.weights.synthetic_blob(pkg.synth.arch_for_size(s), a.weight_seed) for s in SIZES}
    m = pkg.MltCnn(device=0, sizes=SIZES, blobs=blobs)
    org, pred = natural_frame(pkg, 0xC0FFEE)
    p_org, p_pred = m.picture(WIDTH, HEIGHT).upload(org), m.picture(WIDTH, HEIGHT).upload(pred)
    grids = {s: pkg.capi.grid_positions(WIDTH, HEIGHT, s) for s in SIZES}
    pocs = {s: np.full(len(grids[s]), 8, np.int32) for s in SIZES}
    qp_full = {(s, qp): np.full(len(grids[s]), qp, np.int32) for s in SIZES for qp in QPS}
    want = ("split", "logits")

    def leg_a(s):
        return [m.predict_at(s, p_org, p_pred, grids[s], pocs[s], qp_full[(s, qp)], want=want) for qp in QPS]

    def leg_b(s):
        return m.predict_at_sweep(s, p_org, p_pred, grids[s], pocs[s], QPS, want=want)

    times = {(leg, s): [] for leg in "AB" for s in SIZES}
    reruns = {(leg, s): 0 for leg in "AB" for s in SIZES}
    for k in range(a.warmup + a.steps):
        for s in SIZES:
            for name, leg in (("A", leg_a), ("B", leg_b)):
                r0 = m.arithmetic(s)["guard_reruns"]
                t0 = time.perf_counter()
                r = leg(s)
                dt = (time.perf_counter() - t0) * 1e3
                if k >= a.warmup:
                    times[(name, s)].append(dt)
                reruns[(name, s)] = m.arithmetic(s)["guard_reruns"] - r0
                if name == "A":
                    twins = r
            if k == 0:
                same = all(r[key][q].tobytes() == twins[q][key].tobytes() for q in range(len(QPS)) for key in want)
                assert same, f"size {s}: a slab differs from its twin"
    rows = []
    for s in SIZES:
        med_a, med_b = statistics.median(times[("A", s)]), statistics.median(times[("B", s)])
        rows.append({"size": s, "cus": int(len(grids[s])), "arithmetic_exact": m.arithmetic(s)["exact"], "four_calls_ms_median": round(med_a, 4), "sweep_ms_median": round(med_b, 4),
                     "ratio_sweep_over_four_calls": round(med_b / med_a, 4), "four_calls_ms_min_max": [round(min(times[("A", s)]), 4), round(max(times[("A", s)]), 4)],
                     "sweep_ms_min_max": [round(min(times[("B", s)]), 4), round(max(times[("B", s)]), 4)], "reruns_four_calls": int(reruns[("A", s)]), "reruns_sweep": int(reruns[("B", s)]),
                     "slabs_byte_equal": True})
    frame_a = statistics.median([sum(times[("A", s)][k] for s in SIZES) for k in range(a.steps)])
    frame_b = statistics.median([sum(times[("B", s)][k] for s in SIZES) for k in range(a.steps)])
    p_org.close()
    p_pred.close()
    m.close()
    print(f"QP sweep against one call per QP, Q = {len(QPS)} {QPS}, {WIDTH} x {HEIGHT} frame of natural patches, sources {pkg.build.source_signature()}, "
          f"{a.steps} alternating steps after {a.warmup} warm-up, split modes + logits to host arrays")
    for r in rows:
        print(f"size {r['size']:3d}: {r['cus']:5d} CUs  four mlt_predict_at calls median {r['four_calls_ms_median']:.3f} ms (min {r['four_calls_ms_min_max'][0]:.3f}, max {r['four_calls_ms_min_max'][1]:.3f})  "
              f"one sweep call median {r['sweep_ms_median']:.3f} ms (min {r['sweep_ms_min_max'][0]:.3f}, max {r['sweep_ms_min_max'][1]:.3f})  sweep / four = {r['ratio_sweep_over_four_calls']:.3f}  "
              f"CUs re-run exactly: {r['reruns_four_calls']} in the four calls, {r['reruns_sweep']} in the sweep")
    print(f"frame (all four grids): four calls per size median {frame_a:.3f} ms, one sweep per size median {frame_b:.3f} ms, sweep / four = {frame_b / frame_a:.3f}; every slab byte-equal to its twin")
    print(json.dumps({"source_sig": pkg.build.source_signature(), "qps": list(QPS), "frame_four_calls_ms_median": round(frame_a, 4), "frame_sweep_ms_median": round(frame_b, 4),
                      "frame_ratio_sweep_over_four_calls": round(frame_b / frame_a, 4), "sizes": rows}))


if __name__ == "__main__":
    main()
