#!/usr/bin/env python3
"""What the partition trees of ONE frame under several QPs cost in one sweep call against the ways without it (kernel table:
`tree_expand_sweep_kernel`, `tree_sweep_pack_kernel`).

One process, one context (seeded weights, head 0 at every size), one frame of natural patches (scripts/tree_ab.py's tiler) resident as a picture pair, poc 0:
  leg A  ONE mlt_predict_tree_sweep call: one descent over the union of the trees, the trunk once per union node, the heads once per QP
  leg B  ONE mlt_predict_trees call with one entry of the pair per QP: the best way without the sweep -- the trunk once per node of every tree
  leg C  one mlt_predict_tree call per QP
All legs ask for the nodes and the leaf maps.  The legs alternate triple by triple after the warm-up, in --rounds rounds of --triples triples; per leg the median
over all samples, min / max, and the spread (max - min) of the rounds' medians; the trees of the three legs are compared byte for byte.  Reported besides:
union_nodes, the sum of the slices' node counts, and from a profiled run of A and of B the launches per call and the time inside the gather and the tree
kernels.  Run it for the usual QP set and for one whose descents diverge widely:

  python scripts/tree_sweep_ab.py                                         > profiles/tree_sweep_ab.txt
  python scripts/tree_sweep_ab.py --weight-seed 12 --qps 0,37,100,400    >> profiles/tree_sweep_ab.txt"""
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
from trees_ab import profiled  # noqa: E402

OWN = ("picture_gather", "picture_gather_multi", "heads", "heads_sweep", "tree_expand", "tree_raster", "tree_pack", "tree_expand_sweep", "tree_sweep_raster",
       "tree_sweep_rank", "tree_sweep_pack")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--triples", type=int, default=10, help="timed (A, B, C) triples per round")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--qps", default="22,27,32,37")
    ap.add_argument("--weight-seed", type=int, default=13)
    ap.add_argument("--picture-seed", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    qps = [int(v) for v in a.qps.split(",")]
    assert a.rounds >= 3 and a.rounds * a.triples >= 30 and a.warmup >= 5 and 1 <= len(qps) <= 32
    import torch
    import mltcnn_pkg
    pkg = mltcnn_pkg.load()
    assert torch.cuda.is_available(), "needs an MI355X (no CPU fallback)"
    pkg.build.build_lib()
    W, H, Q = a.width, a.height, len(qps)
    blobs = {s: pkg.weights.synthetic_blob(pkg.synth.arch_for_size(s), a.weight_seed) for s in SIZES}
    m = pkg.MltCnn(device=0, sizes=SIZES, blobs=blobs, head_index={s: 0 for s in SIZES})
    org, pred = frame(pkg, W, H, a.picture_seed)
    o, p = m.picture(W, H).upload(org), m.picture(W, H).upload(pred)
    kw = dict(want=("leaf_map",))
    legs = {"A": lambda: m.predict_tree_sweep(o, p, 0, qps, **kw), "B": lambda: m.predict_trees([(o, p)] * Q, 0, np.array(qps, np.int32), **kw),
            "C": lambda: [m.predict_tree(o, p, 0, q, **kw) for q in qps]}
    last = {}
    for _ in range(a.warmup):
        for name, leg in legs.items():
            last[name] = leg()
    rounds = {k: [] for k in legs}
    for _ in range(a.rounds):
        t = {k: [] for k in legs}
        for _ in range(a.triples):
            for name, leg in legs.items():
                t0 = time.perf_counter()
                last[name] = leg()
                t[name].append((time.perf_counter() - t0) * 1e3)
        for k in legs:
            rounds[k].append(t[k])
    same = all(x["nodes"].tobytes() == y["nodes"].tobytes() == z["nodes"].tobytes() and x["leaf_map"].tobytes() == y["leaf_map"].tobytes() == z["leaf_map"].tobytes()
               for x, y, z in zip(last["A"], last["B"], last["C"]))
    union = [int(v) for v in last["A"][0]["union_nodes"]]
    slices = [len(x["nodes"]) for x in last["A"]]
    prof_a, launches_a, ms_a = profiled(m, legs["A"], 10)
    prof_b, launches_b, ms_b = profiled(m, legs["B"], 10)
    med = {k: statistics.median([x for r in v for x in r]) for k, v in rounds.items()}
    rng = {k: [round(min(x for r in v for x in r), 4), round(max(x for r in v for x in r), 4)] for k, v in rounds.items()}
    round_med = {k: [round(statistics.median(r), 4) for r in v] for k, v in rounds.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in round_med.items()}
    row = {"picture": [W, H], "qps": qps, "rounds": a.rounds, "triples_per_round": a.triples, "warmup": a.warmup, "weight_seed": a.weight_seed, "picture_seed": a.picture_seed,
           "arithmetic": {s: m.arithmetic(s)["exact"] for s in SIZES}, "union_nodes": union, "union_total": sum(union), "slice_nodes": slices, "slices_total": sum(slices),
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": rng, "round_medians_ms": round_med, "spread_of_round_medians_ms": spread,
           "a_over_b": round(med["A"] / med["B"], 4), "a_over_c": round(med["A"] / med["C"], 4), "a_beats_b_by_more_than_b_spread": bool(med["B"] - med["A"] > spread["B"]),
           "legs_equal": bool(same), "launches_per_call": {"A": launches_a, "B": launches_b}, "all_launches_ms_per_call_profiled": {"A": round(ms_a, 4), "B": round(ms_b, 4)},
           "kernels_a": prof_a, "kernels_b": prof_b}
    o.close()
    p.close()
    m.close()
    print(f"partition trees of one {W} x {H} frame under qps {qps}, sizes 128 .. 16, weight seed {a.weight_seed}, sources {pkg.build.source_signature()}, "
          f"{a.rounds} rounds of {a.triples} alternating triples after {a.warmup} warm-up")
    print(f"  union_nodes {union} = {sum(union)} nodes evaluated by A; slices {slices} = {sum(slices)} nodes evaluated by B and C; the three legs' trees are equal: {same}")
    names = {"A": "one mlt_predict_tree_sweep call        ", "B": f"one mlt_predict_trees call, {Q} entries ", "C": f"{Q} mlt_predict_tree calls              "}
    for k in legs:
        print(f"  leg {k}  {names[k]} median {med[k]:.3f} ms  (min {rng[k][0]:.3f}, max {rng[k][1]:.3f})   round medians {round_med[k]}, spread {spread[k]:.3f} ms")
    print(f"  A / B = {med['A'] / med['B']:.3f}   (B - A = {med['B'] - med['A']:+.3f} ms against B's spread {spread['B']:.3f} ms)   A / C = {med['A'] / med['C']:.3f}")
    for name, prof, launches in (("A", prof_a, launches_a), ("B", prof_b, launches_b)):
        print(f"  leg {name}  {launches:.0f} launches per call; " + "; ".join(f"{k} x{prof[k]['launches_per_call']:.0f} {prof[k]['us_per_call']:.1f} us" for k in OWN if k in prof))
    print(f"  all launches, profiled runs (events around every launch): A {ms_a:.3f} ms, B {ms_b:.3f} ms")
    print(json.dumps({"source_sig": pkg.build.source_signature(), "result": row}))


if __name__ == "__main__":
    main()
