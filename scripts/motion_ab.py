#!/usr/bin/env python3
"""What a prediction picture made on the device costs (kernel table: `motion_search_kernel`, `picture_compensate_kernel`).

One process, one context with all four sizes (seeded weights, head 0 at every size, poc = qp = 0 as scripts/tree_ab.py), one 1920 x 1080 pair of natural patches
(synth.natural_patches: the "pred" patches -- the org field displaced by a few samples and smoothed -- serve as the REFERENCE frame), both resident.  Legs, block 16:
  P8 / P16 / P32  mlt_picture_predict with range 8 / 16 / 32 (lambda 4), no field back, then mlt_synchronize: the prediction picture of one frame
  T               mlt_predict_tree on (original, the prediction P16 left): what the prediction is made for
  U               mlt_picture_upload of a ready 1920 x 1080 prediction from pageable host memory: the host alternative's floor (its motion search not counted)
Legs alternate step by step; medians of the timed steps with min / max.  From a separate profiled run per range (HIP events around every launch,
mlt_profile_read), range 64 included: the time inside the two kernels, and the search per block and per candidate.  The range-8 prediction is compared with the numpy restatement
(fastintercu_vvc_amd/motion.py) byte for byte.  No threshold: what is printed is what is claimed.

  python scripts/motion_ab.py [--steps 30] [--warmup 8] > profiles/motion_ab.txt"""
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
RANGES = (8, 16, 32)
PROFILED_RANGES = RANGES + (64,)   # the largest range: profiled only, for the per-candidate figure
BLOCK, LAMBDA = 16, 4


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
    cur, ref = frame(pkg, W, H, a.picture_seed)
    blobs = {s: pkg.weights.synthetic_blob(pkg.synth.arch_for_size(s), a.weight_seed) for s in SIZES}
    m = pkg.MltCnn(device=0, sizes=SIZES, blobs=blobs, head_index={s: 0 for s in SIZES})
    p_cur, p_ref = m.picture(W, H).upload(cur), m.picture(W, H).upload(ref)
    dst, up = m.picture(W, H), m.picture(W, H)
    bx, by = pkg.capi.motion_blocks(W, H, BLOCK)

    def predict(rng):
        def leg():
            m.predict_picture(p_cur, p_ref, dst, block=BLOCK, search_range=rng, lam=LAMBDA, want_field=False)
            m.synchronize()
        return leg

    # the restatement, once, at the smallest range
    field = m.predict_picture(p_cur, p_ref, dst, block=BLOCK, search_range=RANGES[0], lam=LAMBDA)
    want_plane, want_mv, want_cost = pkg.motion.predict(cur, ref, BLOCK, RANGES[0], LAMBDA)
    same = bool(field["mv"].tobytes() == want_mv.tobytes() and field["cost"].tobytes() == want_cost.tobytes() and dst.download().tobytes() == want_plane.tobytes())
    moved = float((want_mv.reshape(-1, 2) != 0).any(axis=1).mean())

    predict(16)()
    ready = dst.download()
    legs = [(f"P{r}", predict(r)) for r in RANGES]
    legs += [("T", lambda: m.predict_tree(p_cur, up, 0, 0, want=("leaf_map",))), ("U", lambda: up.upload(ready))]
    up.upload(ready)
    times = {name: [] for name, _ in legs}
    for k in range(a.warmup + a.steps):
        for name, leg in legs:
            t0 = time.perf_counter()
            leg()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                times[name].append(dt)
    nodes = len(m.predict_tree(p_cur, up, 0, 0, want=("leaf_map",))["nodes"])
    kern = {}
    for r in PROFILED_RANGES:
        m.profile_enable(True)
        for _ in range(a.steps):
            predict(r)()
        prof = {p["name"]: p for p in m.profile_read()}
        m.profile_enable(False)
        assert prof["motion_search"]["launches"] == a.steps and prof["picture_compensate"]["launches"] == a.steps
        s_us = 1e3 * prof["motion_search"]["total_ms"] / a.steps
        c_us = 1e3 * prof["picture_compensate"]["total_ms"] / a.steps
        cands = (2 * r + 1) ** 2
        kern[r] = {"motion_search_us": round(s_us, 2), "picture_compensate_us": round(c_us, 2), "candidates": cands,
                   "search_ns_per_block": round(1e3 * s_us / (bx * by), 2), "search_ps_per_block_candidate": round(1e6 * s_us / (bx * by * cands), 2),
                   "compensate_gbps_algorithmic": round(prof["picture_compensate"]["bytes"] / a.steps / (c_us * 1e-6) / 1e9, 1)}
    med = {k: statistics.median(v) for k, v in times.items()}
    rng = {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}
    row = {"picture": [W, H], "block": BLOCK, "lambda": LAMBDA, "blocks": [bx, by], "steps": a.steps, "warmup": a.warmup, "weight_seed": a.weight_seed,
           "picture_seed": a.picture_seed, "device_equals_restatement_range8": same, "blocks_with_nonzero_vector_range8": round(moved, 4), "tree_nodes": nodes,
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": rng, "kernels": {str(r): v for r, v in kern.items()},
           "predict_share_of_tree": {f"P{r}": round(med[f"P{r}"] / med["T"], 4) for r in RANGES}}
    for p in (p_cur, p_ref, dst, up):
        p.close()
    m.close()
    print(f"prediction picture of a {W} x {H} frame on the device, block {BLOCK}, lambda {LAMBDA}, sources {pkg.build.source_signature()}, {a.steps} alternating steps after "
          f"{a.warmup} warm-up")
    print(f"  {bx} x {by} blocks; device == numpy restatement at range {RANGES[0]} (field, costs, plane): {same}; blocks with a non-zero vector there: {100 * moved:.1f} %")
    for r in RANGES:
        k = kern[r]
        print(f"  leg P{r:<2} mlt_picture_predict, range {r:2d} ({k['candidates']:4d} candidates)  median {med[f'P{r}']:.3f} ms  (min {rng[f'P{r}'][0]:.3f}, max {rng[f'P{r}'][1]:.3f})   "
              f"= {med[f'P{r}'] / med['T']:.3f} of leg T")
        print(f"         motion_search {k['motion_search_us']:.1f} us ({k['search_ns_per_block']:.1f} ns per block, {k['search_ps_per_block_candidate']:.1f} ps per block and candidate), "
              f"picture_compensate {k['picture_compensate_us']:.1f} us ({k['compensate_gbps_algorithmic']:.0f} GB/s algorithmic)")
    k = kern[64]
    print(f"  range 64 ({k['candidates']} candidates, profiled run only): motion_search {k['motion_search_us']:.1f} us ({k['search_ns_per_block']:.1f} ns per block, "
          f"{k['search_ps_per_block_candidate']:.1f} ps per block and candidate)")
    print(f"  leg T   mlt_predict_tree on (original, prediction), {nodes} nodes       median {med['T']:.3f} ms  (min {rng['T'][0]:.3f}, max {rng['T'][1]:.3f})")
    print(f"  leg U   mlt_picture_upload of a ready prediction (pageable host)      median {med['U']:.3f} ms  (min {rng['U'][0]:.3f}, max {rng['U'][1]:.3f})   the host path's floor")
    print(json.dumps({"source_sig": pkg.build.source_signature(), "result": row}))


if __name__ == "__main__":
    main()
