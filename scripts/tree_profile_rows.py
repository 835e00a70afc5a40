#!/usr/bin/env python3
"""The profile table of the picture and tree entry points on one fixed case: mlt_profile_read's rows, in order, as (name, launches, bytes) -- no times -- for one
call each of predict_at, predict_at_sweep, predict_tree, predict_trees, predict_tree_sweep and predict_trees_sweep.  tests/test_tree_profile_rows_gpu.py replays
`rows()` against the committed capture (tests/golden/tree_profile_rows.json), so a change to how the host runtime fills the table is seen.

The case: weights of seed 12 (the diverging-descent seed of scripts/trees_sweep_ab.py) at all four sizes, head 0; the 424 x 280 natural picture of the tree tests
(twelve natural 128 x 128 patches tiled 4 x 3 and cropped), picture seed 1 for the one-pair calls and seeds 1 .. 3 (poc 0 .. 2) for the several-pair calls; QPs
0 and 37 (the plain calls run at QP 0, the sweeps under both); every output wanted.  predict_at / predict_at_sweep take the picture's whole 16 x 16 grid.

  python scripts/tree_profile_rows.py --out tests/golden/tree_profile_rows.json     # on the commit whose rows are to be pinned

The case runs twice in the process; "reproduced" says whether the second run gave the first one's rows."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (128, 64, 32, 16)
W, H = 424, 280
CASE = {"weight_seed": 12, "sizes": list(SIZES), "head": 0, "picture": [W, H], "picture_seeds": [1, 2, 3], "qps": [0, 37], "at_size": 16,
        "want": "everything", "calls": ["predict_at", "predict_at_sweep", "predict_tree", "predict_trees", "predict_tree_sweep", "predict_trees_sweep"]}
TREE_ALL = ("leaf_map", "logits", "decisions", "candidates")


def picture(pkg, seed):
    org, pred = pkg.synth.natural_patches(128, 12, seed)
    tile = lambda p: np.ascontiguousarray(p.reshape(3, 4, 128, 128).transpose(0, 2, 1, 3).reshape(384, 512)[:H, :W])
    return tile(org), tile(pred)


def rows(pkg, m=None):
    """-> {call: [[name, launches, bytes], ...]} of the case on context `m` (default: a context of its own, closed afterwards)."""
    own = m is None
    if own:
        blobs = {s: pkg.weights.synthetic_blob(pkg.synth.arch_for_size(s), CASE["weight_seed"]) for s in SIZES}
        m = pkg.MltCnn(device=0, sizes=SIZES, blobs=blobs, head_index={s: CASE["head"] for s in SIZES})
    pairs = []
    for seed in CASE["picture_seeds"]:
        org, pred = picture(pkg, seed)
        pairs.append((m.picture(W, H).upload(org), m.picture(W, H).upload(pred)))
    (o, p), qps, pocs = pairs[0], CASE["qps"], list(range(len(pairs)))
    xy = pkg.capi.grid_positions(W, H, CASE["at_size"])
    z = np.zeros(len(xy), np.int32)
    calls = {"predict_at": lambda: m.predict_at(CASE["at_size"], o, p, xy, z, z),
             "predict_at_sweep": lambda: m.predict_at_sweep(CASE["at_size"], o, p, xy, z, qps),
             "predict_tree": lambda: m.predict_tree(o, p, 0, qps[0], want=TREE_ALL),
             "predict_trees": lambda: m.predict_trees(pairs, pocs, qps[0], want=TREE_ALL),
             "predict_tree_sweep": lambda: m.predict_tree_sweep(o, p, 0, qps, want=TREE_ALL),
             "predict_trees_sweep": lambda: m.predict_trees_sweep(pairs, pocs, 0, qps, want=TREE_ALL)}
    got = {}
    try:
        for name in CASE["calls"]:
            m.profile_enable(True)   # (clears the accumulated launches)
            calls[name]()
            got[name] = [[r["name"], int(r["launches"]), float(r["bytes"])] for r in m.profile_read()]
    finally:
        m.profile_enable(False)
        for a, b in pairs:
            a.close()
            b.close()
        if own:
            m.close()
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the capture here (default: print it)")
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git rev-parse HEAD)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import mltcnn_pkg
    pkg = mltcnn_pkg.load()
    assert torch.cuda.is_available(), "needs an MI355X (no CPU fallback)"
    pkg.build.build_lib()
    first, second = rows(pkg), rows(pkg)
    head = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    doc = {"commit": head, "source_sig": pkg.build.source_signature(), "case": CASE, "reproduced": first == second, "rows": first}
    text = json.dumps(doc, indent=1) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    print(f"rows reproduced by a second run: {first == second}", file=sys.stderr)


if __name__ == "__main__":
    main()
