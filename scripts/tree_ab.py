#!/usr/bin/env python3
"""What the partition tree of a frame costs on three paths (kernel table: `tree_expand_kernel`, `tree_raster_kernel`).

One process, one context with all four sizes (seeded weights, head 0 at every size, poc = qp = 0: the setting in which the seeded heads give mixed decisions,
tests/test_tree_gpu.py), one 1920 x 1080 frame of natural patches (synth.natural_patches, 135 tiles of 128 x 128, cropped) resident as a picture pair:
  leg A  mlt_predict_tree: the descent on the device, nodes + leaf map back
  leg B  the same descent driven from the host through mlt_predict_at, level by level (decisions.build_tree over MltCnn.predict_at asking for the decision
         records only) -- the path a caller had before, and the baseline.  Reported twice: the whole host loop in Python, and the time inside the mlt_predict_at
         calls alone (what a host loop in any language pays at least)
  leg C  the four full size-aligned grids tools/picture_map.py runs without --tree (decision + candidate records), whatever the parents decided
Legs alternate step by step; medians of the timed steps with min / max, the nodes each leg evaluates, and -- from a separate profiled run of leg A (HIP events
around every launch, mlt_profile_read) -- the time inside the two new kernels and inside all launches.

  python scripts/tree_ab.py [--steps 30] [--warmup 8] > profiles/tree_ab.txt"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (128, 64, 32, 16)


def frame(pkg, width, height, seed):
    cols, rows = (width + 127) // 128, (height + 127) // 128
    org, pred = pkg.synth.natural_patches(128, cols * rows, seed)
    tile = lambda p: np.ascontiguousarray(p.reshape(rows, cols, 128, 128).transpose(0, 2, 1, 3).reshape(rows * 128, cols * 128)[:height, :width])
    return tile(org), tile(pred)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--weight-seed", type=int, default=13)
    ap.add_argument("--picture-seed", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    assert a.steps >= 20 and a.warmup >= 5
    import torch
    import mltcnn_pkg
    pkg = mltcnn_pkg.load()
    assert torch.cuda.is_available(), "needs an MI355X (no CPU fallback)"
    pkg.build.build_lib()
    W, H = a.width, a.height
    org, pred = frame(pkg, W, H, a.picture_seed)
    blobs = {s: pkg.weights.synthetic_blob(pkg.synth.arch_for_size(s), a.weight_seed) for s in SIZES}
    m = pkg.MltCnn(device=0, sizes=SIZES, blobs=blobs, head_index={s: 0 for s in SIZES})
    p_org, p_pred = m.picture(W, H).upload(org), m.picture(W, H).upload(pred)
    grids = {s: pkg.capi.grid_positions(W, H, s) for s in SIZES}
    inside = [0.0]

    def leg_a():
        return m.predict_tree(p_org, p_pred, 0, 0, want=("leaf_map",))

    def decide(size, xy):
        z = np.zeros(len(xy), np.int32)
        t0 = time.perf_counter()
        d = m.predict_at(size, p_org, p_pred, xy, z, z, want=("decisions",))["decisions"]
        inside[0] += time.perf_counter() - t0
        return d["split_mode"], d["confidence"], np.uint32(1) << d["raw_mode"].astype(np.uint32)

    def leg_b():
        return pkg.decisions.build_tree(W, H, 128, 16, None, decide)

    def leg_c():
        for s in SIZES:
            z = np.zeros(len(grids[s]), np.int32)
            m.predict_at(s, p_org, p_pred, grids[s], z, z, want=("decisions", "candidates"))

    times = {"A": [], "B": [], "B_inside": [], "C": []}
    for k in range(a.warmup + a.steps):
        for name, leg in (("A", leg_a), ("B", leg_b), ("C", leg_c)):
            inside[0] = 0.0
            t0 = time.perf_counter()
            r = leg()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                times[name].append(dt)
                if name == "B":
                    times["B_inside"].append(inside[0] * 1e3)
            if name == "A":
                tree = r
            elif name == "B":
                host_nodes, host_map = r
    same = bool(tree["nodes"].tobytes() == host_nodes.tobytes() and tree["leaf_map"].tobytes() == host_map.tobytes())
    nodes = tree["nodes"]
    per_level = {s: [int((nodes["size"] == s).sum()), int(((nodes["size"] == s) & (nodes["first_child"] >= 0)).sum())] for s in SIZES}
    m.profile_enable(True)
    for _ in range(a.steps):
        leg_a()
    prof = {p["name"]: p for p in m.profile_read()}
    m.profile_enable(False)
    med = {k: statistics.median(v) for k, v in times.items()}
    rng = {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}
    kern = {k: {"launches_per_call": prof[k]["launches"] / a.steps, "us_per_call": round(1e3 * prof[k]["total_ms"] / a.steps, 2)} for k in ("tree_expand", "tree_raster")}
    all_ms = sum(p["total_ms"] for p in prof.values()) / a.steps
    row = {"picture": [W, H], "steps": a.steps, "warmup": a.warmup, "weight_seed": a.weight_seed, "picture_seed": a.picture_seed,
           "arithmetic": {s: m.arithmetic(s)["exact"] for s in SIZES}, "nodes_tree": int(len(nodes)), "nodes_per_level_and_descending": per_level,
           "nodes_full_grids": int(sum(len(g) for g in grids.values())), "tree_max_nodes": pkg.capi.tree_max_nodes(W, H),
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": rng, "device_tree_equals_host_tree": same,
           "kernels": kern, "all_launches_ms_per_call_profiled": round(all_ms, 4)}
    p_org.close()
    p_pred.close()
    m.close()
    print(f"partition tree of a {W} x {H} frame on three paths, sources {pkg.build.source_signature()}, {a.steps} alternating steps after {a.warmup} warm-up")
    print(f"  nodes: tree {row['nodes_tree']} (per size [nodes, descending]: {per_level}); four full grids {row['nodes_full_grids']}; device tree == host tree: {same}")
    print(f"  leg A  mlt_predict_tree (device descent)                 median {med['A']:.3f} ms  (min {rng['A'][0]:.3f}, max {rng['A'][1]:.3f})   {row['nodes_tree']} nodes")
    print(f"  leg B  host descent over mlt_predict_at, whole loop     median {med['B']:.3f} ms  (min {rng['B'][0]:.3f}, max {rng['B'][1]:.3f})   {row['nodes_tree']} nodes")
    print(f"         ... inside the mlt_predict_at calls alone        median {med['B_inside']:.3f} ms  (min {rng['B_inside'][0]:.3f}, max {rng['B_inside'][1]:.3f})")
    print(f"  leg C  four full grids (picture_map.py without --tree)  median {med['C']:.3f} ms  (min {rng['C'][0]:.3f}, max {rng['C'][1]:.3f})   {row['nodes_full_grids']} CUs")
    print(f"  A / B = {med['A'] / med['B']:.3f} (whole loop), A / B-inside = {med['A'] / med['B_inside']:.3f}, A / C = {med['A'] / med['C']:.3f}")
    for k in ("tree_expand", "tree_raster"):
        print(f"  {k}: {kern[k]['launches_per_call']:.0f} launches per call, {kern[k]['us_per_call']:.1f} us per call in all")
    print(f"  all launches of a leg-A call (profiled run, events around every launch): {all_ms:.3f} ms")
    print(json.dumps({"source_sig": pkg.build.source_signature(), "result": row}))


if __name__ == "__main__":
    main()
