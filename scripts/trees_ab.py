#!/usr/bin/env python3
"""What the partition trees of P frames cost in one call against P calls (kernel table: `tree_expand_kernel`, `tree_pack_kernel`).

One process, one context (seeded weights, head 0 at every size), P frames of natural patches (synth.natural_patches tiled and cropped, frame f from picture seed
--picture-seed + f, poc = f, qp = 0) resident as picture pairs:
  leg A  ONE mlt_predict_trees call over the P frames: per level one network pass over the nodes of all frames
  leg B  P mlt_predict_tree calls, one per frame: the same descent over one picture at a time, the baseline
Both legs ask for the nodes and the leaf maps.  Legs alternate pair by pair after the warm-up; medians with min / max and the spread of B; the trees of the two
legs are compared byte for byte.  From separate profiled runs of each leg (HIP events around every launch, mlt_profile_read): launches per call, and the time inside
the expand, raster, gather and pack launches and inside all launches.  Run it for the full descent and for the single-pass tier at the 128 level alone:

  python scripts/trees_ab.py                                          > profiles/trees_ab.txt
  python scripts/trees_ab.py --weight-seed 10 --top 128 --min-size 128 >> profiles/trees_ab.txt"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tree_ab import SIZES, frame  # noqa: E402  (scripts/tree_ab.py: the frame tiler)

OWN_A = ("tree_expand", "tree_raster", "picture_gather_multi", "tree_pack")   # the launches of a call beside the network's: batched | single
OWN_B = ("tree_expand", "tree_raster", "picture_gather")


def profiled(m, leg, steps):
    m.profile_enable(True)
    for _ in range(steps):
        leg()
    prof = {p["name"]: p for p in m.profile_read()}
    m.profile_enable(False)
    per = {k: {"launches_per_call": v["launches"] / steps, "us_per_call": round(1e3 * v["total_ms"] / steps, 2)} for k, v in prof.items()}
    return per, sum(v["launches"] for v in prof.values()) / steps, sum(v["total_ms"] for v in prof.values()) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=30, help="timed (A, B) pairs")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--weight-seed", type=int, default=13)
    ap.add_argument("--picture-seed", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--top", type=int, default=128)
    ap.add_argument("--min-size", type=int, default=16)
    a = ap.parse_args()
    assert a.pairs >= 30 and a.warmup >= 5 and 1 <= a.frames <= 256
    sizes = tuple(s for s in SIZES if a.min_size <= s <= a.top)
    assert sizes
    import torch
    import mltcnn_pkg
    pkg = mltcnn_pkg.load()
    assert torch.cuda.is_available(), "needs an MI355X (no CPU fallback)"
    pkg.build.build_lib()
    W, H, P = a.width, a.height, a.frames
    blobs = {s: pkg.weights.synthetic_blob(pkg.synth.arch_for_size(s), a.weight_seed) for s in sizes}
    m = pkg.MltCnn(device=0, sizes=sizes, blobs=blobs, head_index={s: 0 for s in sizes})
    pics = []
    for f in range(P):
        org, pred = frame(pkg, W, H, a.picture_seed + f)
        pics.append((m.picture(W, H).upload(org), m.picture(W, H).upload(pred)))
    poc = list(range(P))
    kw = dict(top=a.top, min_size=a.min_size, want=("leaf_map",))

    def leg_a():
        return m.predict_trees(pics, poc, 0, **kw)

    def leg_b():
        return [m.predict_tree(o, p, poc[f], 0, **kw) for f, (o, p) in enumerate(pics)]

    times = {"A": [], "B": []}
    for k in range(a.warmup + a.pairs):
        for name, leg in (("A", leg_a), ("B", leg_b)):
            t0 = time.perf_counter()
            r = leg()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                times[name].append(dt)
            if name == "A":
                batched = r
            else:
                singles = r
    same = all(x["nodes"].tobytes() == y["nodes"].tobytes() and x["leaf_map"].tobytes() == y["leaf_map"].tobytes() for x, y in zip(batched, singles))
    nodes = np.concatenate([x["nodes"] for x in batched])
    per_level = {s: [int((nodes["size"] == s).sum()), int(((nodes["size"] == s) & (nodes["first_child"] >= 0)).sum())] for s in sizes}
    prof_a, launches_a, ms_a = profiled(m, leg_a, a.pairs)
    prof_b, launches_b, ms_b = profiled(m, leg_b, a.pairs)
    med = {k: statistics.median(v) for k, v in times.items()}
    rng = {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}
    q = statistics.quantiles(times["B"], n=4)
    spread_b = {"min_max": round(rng["B"][1] - rng["B"][0], 4), "interquartile": round(q[2] - q[0], 4)}
    row = {"picture": [W, H], "frames": P, "pairs": a.pairs, "warmup": a.warmup, "weight_seed": a.weight_seed, "picture_seed": a.picture_seed, "top": a.top,
           "min_size": a.min_size, "arithmetic": {s: m.arithmetic(s)["exact"] for s in sizes}, "nodes": int(len(nodes)), "nodes_per_level_and_descending": per_level,
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": rng, "spread_b_ms": spread_b, "a_over_b": round(med["A"] / med["B"], 4),
           "batched_equals_singles": bool(same), "launches_per_call": {"A": launches_a, "B": launches_b},
           "all_launches_ms_per_call_profiled": {"A": round(ms_a, 4), "B": round(ms_b, 4)}, "kernels_a": prof_a, "kernels_b": prof_b}
    for o, p in pics:
        o.close()
        p.close()
    m.close()
    print(f"partition trees of {P} frames of {W} x {H}, sizes {a.top} .. {a.min_size}, weight seed {a.weight_seed}, sources {pkg.build.source_signature()}, "
          f"{a.pairs} alternating pairs after {a.warmup} warm-up")
    print(f"  nodes over the {P} frames: {len(nodes)} (per size [nodes, descending]: {per_level}); batched trees == single trees: {same}")
    print(f"  leg A  one mlt_predict_trees call          median {med['A']:.3f} ms  (min {rng['A'][0]:.3f}, max {rng['A'][1]:.3f})   {launches_a:.0f} launches")
    print(f"  leg B  {P} mlt_predict_tree calls            median {med['B']:.3f} ms  (min {rng['B'][0]:.3f}, max {rng['B'][1]:.3f})   {launches_b:.0f} launches; "
          f"spread max - min {spread_b['min_max']:.3f} ms, interquartile {spread_b['interquartile']:.3f} ms")
    print(f"  A / B = {med['A'] / med['B']:.3f}   (A - B = {med['A'] - med['B']:+.3f} ms)")
    for k in OWN_A:
        if k in prof_a:
            print(f"  leg A  {k}: {prof_a[k]['launches_per_call']:.0f} launches per call, {prof_a[k]['us_per_call']:.1f} us per call in all")
    for k in OWN_B:
        if k in prof_b:
            print(f"  leg B  {k}: {prof_b[k]['launches_per_call']:.0f} launches per {P} calls, {prof_b[k]['us_per_call']:.1f} us in all")
    net = lambda prof, own: sorted(((k, v) for k, v in prof.items() if k not in own), key=lambda kv: -kv[1]["us_per_call"])
    for name, prof, own in (("A", prof_a, OWN_A), ("B", prof_b, OWN_B)):
        print(f"  leg {name}  network launches (profiled run): " + "; ".join(f"{k} x{v['launches_per_call']:.0f} {v['us_per_call']:.0f} us" for k, v in net(prof, own)))
    print(f"  all launches, profiled runs (events around every launch): A {ms_a:.3f} ms, B {ms_b:.3f} ms")
    print(json.dumps({"source_sig": pkg.build.source_signature(), "result": row}))


if __name__ == "__main__":
    main()
