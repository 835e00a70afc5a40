#!/usr/bin/env python3
"""What the partition trees of SEVERAL frames under several QPs each cost in one mlt_predict_trees_sweep call against the two ways without it (kernel
table: the segmented `tree_expand_sweep_kernel`, `tree_sweep_rank_kernel`, `tree_sweep_pack_kernel`).

One process, one context (seeded weights, head 0 at every size), --frames frames of natural patches (scripts/tree_ab.py's tiler, picture seeds --picture-seed + f)
resident as picture pairs, frame f at poc f and QP offset 0:
  leg A  ONE mlt_predict_trees_sweep call: one descent over the unions of all frames, the trunk once per union node, the heads once per QP
  leg B  one mlt_predict_tree_sweep call per frame: the trunk once per union node too, but every level of every call is a small pass and a host synchronisation
  leg C  ONE mlt_predict_trees call with frames x QPs entries: level-wide passes, but the trunk once per node of every tree
B and C are entry points this call leaves as they were.  All legs ask for the nodes and the leaf maps.  The legs alternate triple by triple after the warm-up, in
--rounds rounds of --triples triples; per leg the median over all samples, min / max, and the spread (max - min) of the rounds' medians; the trees of the three legs
must be byte-equal (asserted before anything is reported).  Reported besides: the unions' node counts, the sum of the slices' node counts, and from a profiled run of
each leg the launches per call and the time inside the gather and the tree kernels.  Run it for the usual QP set and for one whose descents diverge widely:

  python scripts/trees_sweep_ab.py                                         > profiles/trees_sweep_ab.txt
  python scripts/trees_sweep_ab.py --weight-seed 12 --qps 0,37,100,400    >> profiles/trees_sweep_ab.txt"""
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
from tree_sweep_ab import OWN  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--triples", type=int, default=6, help="timed (A, B, C) triples per round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--qps", default="22,27,32,37")
    ap.add_argument("--weight-seed", type=int, default=13)
    ap.add_argument("--picture-seed", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    qps = [int(v) for v in a.qps.split(",")]
    assert a.rounds >= 3 and a.rounds * a.triples >= 30 and a.warmup >= 5 and 1 <= len(qps) <= 32 and 1 <= a.frames <= 256
    import torch
    import mltcnn_pkg
    pkg = mltcnn_pkg.load()
    assert torch.cuda.is_available(), "needs an MI355X (no CPU fallback)"
    pkg.build.build_lib()
    W, H, P, Q = a.width, a.height, a.frames, len(qps)
    blobs = {s: pkg.weights.synthetic_blob(pkg.synth.arch_for_size(s), a.weight_seed) for s in SIZES}
    m = pkg.MltCnn(device=0, sizes=SIZES, blobs=blobs, head_index={s: 0 for s in SIZES})
    pairs = []
    for f in range(P):
        org, pred = frame(pkg, W, H, a.picture_seed + f)
        pairs.append((m.picture(W, H).upload(org), m.picture(W, H).upload(pred)))
    pocs = list(range(P))
    kw = dict(want=("leaf_map",))
    flat_pairs = [pairs[f] for f in range(P) for _ in qps]
    flat_poc = np.array([f for f in range(P) for _ in qps], np.int32)
    flat_qp = np.array([q for _ in range(P) for q in qps], np.int32)
    legs = {"A": lambda: [t for row in m.predict_trees_sweep(pairs, pocs, 0, qps, **kw) for t in row],
            "B": lambda: [t for f in range(P) for t in m.predict_tree_sweep(pairs[f][0], pairs[f][1], f, qps, **kw)],
            "C": lambda: m.predict_trees(flat_pairs, flat_poc, flat_qp, **kw)}
    last = {}
    for _ in range(a.warmup):
        for name, leg in legs.items():
            last[name] = leg()
    same = all(len(last[k]) == P * Q for k in legs) and all(
        x["nodes"].tobytes() == y["nodes"].tobytes() == z["nodes"].tobytes() and x["leaf_map"].tobytes() == y["leaf_map"].tobytes() == z["leaf_map"].tobytes()
        for x, y, z in zip(last["A"], last["B"], last["C"]))
    assert same, "the three legs' trees differ: no timing counts"
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
    unions = [[int(v) for v in last["A"][f * Q]["union_nodes"]] for f in range(P)]
    union_total = sum(sum(u) for u in unions)
    slices_total = sum(len(x["nodes"]) for x in last["A"])
    prof = {k: profiled(m, legs[k], 5) for k in legs}
    med = {k: statistics.median([x for r in v for x in r]) for k, v in rounds.items()}
    rng = {k: [round(min(x for r in v for x in r), 4), round(max(x for r in v for x in r), 4)] for k, v in rounds.items()}
    round_med = {k: [round(statistics.median(r), 4) for r in v] for k, v in rounds.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in round_med.items()}
    row = {"picture": [W, H], "frames": P, "qps": qps, "rounds": a.rounds, "triples_per_round": a.triples, "warmup": a.warmup, "weight_seed": a.weight_seed,
           "picture_seed": a.picture_seed, "arithmetic": {s: m.arithmetic(s)["exact"] for s in SIZES}, "union_nodes_per_frame": unions, "union_total": union_total,
           "slices_total": slices_total, "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": rng, "round_medians_ms": round_med,
           "spread_of_round_medians_ms": spread, "a_over_b": round(med["A"] / med["B"], 4), "a_over_c": round(med["A"] / med["C"], 4),
           "a_beats_b_by_more_than_b_spread": bool(med["B"] - med["A"] > spread["B"]), "a_beats_c_by_more_than_c_spread": bool(med["C"] - med["A"] > spread["C"]),
           "legs_equal": bool(same), "launches_per_call": {k: prof[k][1] for k in legs}, "all_launches_ms_per_call_profiled": {k: round(prof[k][2], 4) for k in legs},
           "kernels": {k: prof[k][0] for k in legs}}
    for o, p in pairs:
        o.close()
        p.close()
    m.close()
    print(f"partition trees of {P} {W} x {H} frames under qps {qps}, sizes 128 .. 16, weight seed {a.weight_seed}, sources {pkg.build.source_signature()}, "
          f"{a.rounds} rounds of {a.triples} alternating triples after {a.warmup} warm-up")
    print(f"  unions {union_total} nodes evaluated by A and B (per frame and level: {unions}); slices {slices_total} nodes evaluated by C; "
          f"the three legs' trees are equal: {same}")
    names = {"A": "one mlt_predict_trees_sweep call         ", "B": f"{P} mlt_predict_tree_sweep calls           ", "C": f"one mlt_predict_trees call, {P * Q} entries "}
    for k in legs:
        print(f"  leg {k}  {names[k]} median {med[k]:.3f} ms  (min {rng[k][0]:.3f}, max {rng[k][1]:.3f})   round medians {round_med[k]}, spread {spread[k]:.3f} ms")
    print(f"  A / B = {med['A'] / med['B']:.3f}   (B - A = {med['B'] - med['A']:+.3f} ms against B's spread {spread['B']:.3f} ms)   "
          f"A / C = {med['A'] / med['C']:.3f}   (C - A = {med['C'] - med['A']:+.3f} ms against C's spread {spread['C']:.3f} ms)")
    for k in legs:
        per, launches, ms = prof[k]
        print(f"  leg {k}  {launches:.0f} launches per call, {ms:.3f} ms inside them (profiled run, events around every launch); " +
              "; ".join(f"{n} x{per[n]['launches_per_call']:.0f} {per[n]['us_per_call']:.1f} us" for n in OWN if n in per))
    print(json.dumps({"source_sig": pkg.build.source_signature(), "result": row}))


if __name__ == "__main__":
    main()
