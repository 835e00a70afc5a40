#!/usr/bin/env python3
"""What the picture path costs beside the dense path it is built on (kernel table: `picture_gather_kernel`).

One process, one context, seed-10 weights, flags = 0.  The CUs of the bench workload (synth.make_patches_bulk) are laid out on the size-aligned grid of a
picture pair, so both legs evaluate THE SAME CUs:
  leg A  mlt_predict_batch_device on the pre-cut dense device planes (the existing path: the baseline), synchronised after every step
  leg B  mlt_predict_at on the two device-resident pictures with grid_positions (positions, poc, qp from host arrays, results to host arrays)
Legs alternate step by step; the medians of the timed steps are reported with their ratio, then -- from a separate profiled run (HIP events around every
launch, mlt_profile_read) -- the gather launch's own time, its algorithmic read + write bandwidth and that as a fraction of the device copy rate in
profiles/r01e_machine_peaks.json (copy_1GiB_read_plus_write_TBps).  Two workloads: 4096 CUs of 128 x 128 (an 8192 x 8192 picture) and the 8040 CUs of 16 x 16
of a 1920 x 1080 picture.

  python scripts/picture_gather_ab.py [--steps 30] [--warmup 8] > profiles/picture_gather_ab.txt"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grid_picture(cus: np.ndarray, width: int, height: int) -> np.ndarray:
    """CUs [n][S][S] in raster order of the size-aligned grid -> int16 [height, width] (zeros in the partial border)."""
    n, S, _ = cus.shape
    cols, rows = width // S, height // S
    assert n == cols * rows
    pic = np.zeros((height, width), np.int16)
    pic[:rows * S, :cols * S] = cus.reshape(rows, cols, S, S).transpose(0, 2, 1, 3).reshape(rows * S, cols * S)
    return pic


def workload(pkg, torch, m, size, width, height, steps, warmup, copy_tbps):
    dev = torch.device("cuda", 0)
    xy = pkg.capi.grid_positions(width, height, size)
    n = len(xy)
    org, pred = pkg.synth.make_patches_bulk(size, n, 0xC0FFEE)
    poc, qp = pkg.synth.make_scalars(n, 0xC0FFEE)
    p_org, p_pred = m.picture(width, height).upload(grid_picture(org, width, height)), m.picture(width, height).upload(grid_picture(pred, width, height))
    d = [torch.from_numpy(x).to(dev) for x in (org, pred, poc, qp)]
    d_split = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_logits = torch.zeros((n, m.num_logits(size)), dtype=torch.float32, device=dev)

    def leg_a():
        m.predict_batch_device(n, size, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d_split.data_ptr(), d_logits.data_ptr())
        m.synchronize()

    def leg_b():
        return m.predict_at(size, p_org, p_pred, xy, poc, qp, want=("split", "logits"))

    times = {"A": [], "B": []}
    for k in range(warmup + steps):
        for name, leg in (("A", leg_a), ("B", leg_b)):
            t0 = time.perf_counter()
            r = leg()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= warmup:
                times[name].append(dt)
    same = bool(np.array_equal(r["split"], d_split.cpu().numpy()) and r["logits"].tobytes() == d_logits.cpu().numpy().tobytes())
    m.profile_enable(True)
    for _ in range(steps):
        leg_b()
    prof = {p["name"]: p for p in m.profile_read()}
    m.profile_enable(False)
    g = prof["picture_gather"]
    us = 1e3 * g["total_ms"] / g["launches"]
    tbps = g["bytes"] / (g["total_ms"] * 1e-3) / 1e12
    med_a, med_b = statistics.median(times["A"]), statistics.median(times["B"])
    p_org.close()
    p_pred.close()
    return {"size": size, "picture": [width, height], "cus": n, "steps": steps, "warmup": warmup, "arithmetic": m.arithmetic(size)["exact"],
            "dense_device_ms_median": round(med_a, 4), "picture_path_ms_median": round(med_b, 4), "ratio_picture_over_dense": round(med_b / med_a, 4),
            "dense_device_ms_min_max": [round(min(times["A"]), 4), round(max(times["A"]), 4)], "picture_path_ms_min_max": [round(min(times["B"]), 4), round(max(times["B"]), 4)],
            "results_byte_equal": same, "gather_launches_per_step": g["launches"] / steps, "gather_us_per_launch": round(us, 2),
            "gather_bytes_per_launch": g["bytes"] / g["launches"], "gather_read_plus_write_TBps": round(tbps, 3), "gather_fraction_of_device_copy": round(tbps / copy_tbps, 3),
            "all_kernels_ms_per_step_profiled": round(sum(p["total_ms"] for p in prof.values()) / steps, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--weight-seed", type=int, default=10)
    a = ap.parse_args()
    assert a.steps >= 20 and a.warmup >= 5
    import torch
    import mltcnn_pkg
    pkg = mltcnn_pkg.load()
    assert torch.cuda.is_available(), "needs an MI355X (no CPU fallback)"
    pkg.build.build_lib()
    copy_tbps = json.load(open(os.path.join(ROOT, "profiles", "r01e_machine_peaks.json")))["copy_1GiB_read_plus_write_TBps"]
    rows = []
    for size, width, height in ((128, 8192, 8192), (16, 1920, 1080)):
        blob = pkg.weights.synthetic_blob(pkg.synth.arch_for_size(size), a.weight_seed)
        m = pkg.MltCnn(device=0, sizes=(size,), blobs={size: blob}, max_batch=4096)
        rows.append(workload(pkg, torch, m, size, width, height, a.steps, a.warmup, copy_tbps))
        m.close()
    print(f"picture path against the dense device path, sources {pkg.build.source_signature()}, device copy rate {copy_tbps} TB/s (profiles/r01e_machine_peaks.json)")
    for r in rows:
        print(f"{r['cus']} CUs of {r['size']} x {r['size']} ({r['picture'][0]} x {r['picture'][1]} picture), {r['steps']} alternating steps after {r['warmup']} warm-up:")
        print(f"  leg A  mlt_predict_batch_device, dense planes   median {r['dense_device_ms_median']:.3f} ms  (min {r['dense_device_ms_min_max'][0]:.3f}, max {r['dense_device_ms_min_max'][1]:.3f})")
        print(f"  leg B  mlt_predict_at, resident pictures       median {r['picture_path_ms_median']:.3f} ms  (min {r['picture_path_ms_min_max'][0]:.3f}, max {r['picture_path_ms_min_max'][1]:.3f})")
        print(f"  B / A = {r['ratio_picture_over_dense']:.4f}; results byte-equal: {r['results_byte_equal']}")
        print(f"  picture_gather: {r['gather_launches_per_step']:.0f} launch(es) per step, {r['gather_us_per_launch']:.1f} us each, {r['gather_bytes_per_launch'] / 1e6:.1f} MB read + written "
              f"-> {r['gather_read_plus_write_TBps']:.2f} TB/s = {100 * r['gather_fraction_of_device_copy']:.0f} % of the device copy rate")
    print(json.dumps({"source_sig": pkg.build.source_signature(), "workloads": rows}))


if __name__ == "__main__":
    main()
