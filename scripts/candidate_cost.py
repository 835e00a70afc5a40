#!/usr/bin/env python3
"""What the candidate records and the candidate guard cost on the bench workload (docs/KERNEL_NOTES.md, "Candidate sets").

The 4096-CU device-resident batch bench.py times (seed-10 weights, texture content, flags = 0), through mlt_predict_batch_device (split
modes), mlt_predict_batch_device_decisions (records) and mlt_predict_batch_device_candidates (candidate records), policy at its default and
set, with HIP events around every launch (mlt_profile_read): total and per-launch time of the heads launch, CUs the guards re-evaluated per
step (the candidate guard's share is the difference to the default-policy figure), and the wall-clock step time.  Prints one JSON line.

  python scripts/candidate_cost.py [--steps 50] [--warmup 20] [--coverage 0.9] [--max-modes 0] [--batch 4096] [--size 128]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--coverage", type=float, default=0.9)
    ap.add_argument("--max-modes", type=int, default=0)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--weight-seed", type=int, default=10)
    a = ap.parse_args()
    import torch
    import mltcnn_pkg
    pkg = mltcnn_pkg.load()
    assert torch.cuda.is_available(), "needs an MI355X (no CPU fallback)"
    pkg.build.build_lib()
    size, B = a.size, a.batch
    dev = torch.device("cuda", 0)
    blob = pkg.weights.synthetic_blob(pkg.synth.arch_for_size(size), a.weight_seed)
    m = pkg.MltCnn(device=0, sizes=(size,), blobs={size: blob}, max_batch=B)
    org, pred = pkg.synth.make_patches_bulk(size, B, 0xC0FFEE)
    poc, qp = pkg.synth.make_scalars(B, 0xC0FFEE)
    d = [torch.from_numpy(x).to(dev) for x in (org, pred, poc, qp)]
    nl = m.num_logits(size)
    d_split = torch.full((B,), -1, dtype=torch.int32, device=dev)
    d_dec = torch.zeros((B * 48,), dtype=torch.uint8, device=dev)
    d_cand = torch.zeros((B * 40,), dtype=torch.uint8, device=dev)
    d_logits = torch.zeros((B, nl), dtype=torch.float32, device=dev)
    m.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def step(kind):
        m.predict_batch_device(B, size, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                               d_split.data_ptr() if kind == "split" else None, d_logits.data_ptr(),
                               d_decisions=d_dec.data_ptr() if kind != "split" else None, d_candidates=d_cand.data_ptr() if kind == "candidates" else None)

    out = {"size": size, "batch": B, "steps": a.steps, "policy": [a.coverage, a.max_modes], "arithmetic": m.arithmetic(size)["exact"], "configs": {}}
    for name, kind, policy in (("split, default policy", "split", (0.0, 0)), ("records, default policy", "records", (0.0, 0)),
                               ("candidates, default policy", "candidates", (0.0, 0)), ("split, policy set", "split", (a.coverage, a.max_modes)),
                               ("candidates, policy set", "candidates", (a.coverage, a.max_modes))):
        m.set_candidate_policy(size, *policy)
        for _ in range(a.warmup):
            step(kind)
        torch.cuda.synchronize()
        r0 = m.arithmetic(size)["guard_reruns"]
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step(kind)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) / a.steps * 1e3
        reruns = (m.arithmetic(size)["guard_reruns"] - r0) / a.steps
        m.profile_enable(True)
        for _ in range(a.steps):
            step(kind)
        torch.cuda.synchronize()
        prof = m.profile_read()
        m.profile_enable(False)
        heads = next(p for p in prof if p["name"] == "heads")
        cfg = {"ms_per_step": round(wall_ms, 4), "guard_reruns_per_step": round(reruns, 2), "guard_rerun_share": round(reruns / B, 5),
               "heads_launches_per_step": heads["launches"] / a.steps, "heads_total_ms_per_step": round(heads["total_ms"] / a.steps, 5),
               "heads_us_per_launch": round(1e3 * heads["total_ms"] / max(heads["launches"], 1), 3),
               "all_kernels_ms_per_step": round(sum(p["total_ms"] for p in prof) / a.steps, 4)}
        if kind == "candidates":
            c = np.frombuffer(d_cand.cpu().numpy().tobytes(), pkg.capi.CANDIDATES_DTYPE)
            cfg["mean_kept"] = round(float(c["count"].mean()), 4)
        out["configs"][name] = cfg
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
