#!/usr/bin/env python3
"""What quarter-sample refinement and a per-block reference choice cost, and what they buy (`motion_refine_kernel`; include/mltcnn.h: mlt_picture_predict_refs).

One process, one context (no weights: the motion calls need none), one 1920 x 1080 pair of natural patches as scripts/motion_ab.py (the "pred" patches serve as
reference 0; references 1 .. 3 are that frame moved by a few whole samples), everything resident.  Block 16, lambda 4.  Legs:
  P8 / P16        mlt_picture_predict with range 8 / 16, no field back, then mlt_synchronize: the UNCHANGED integer, one-reference call -- the yardstick
  S0 / S1 / S2    mlt_picture_predict_refs, range 16, one reference, subpel 0 / 1 / 2 (1 / 9 / 49 candidates per block)
  S2x2 / S2x4     ... subpel 2 with two / four references
Legs alternate step by step; medians of the timed steps with min / max.  From a separate profiled run per leg (HIP events around every launch, mlt_profile_read):
the time inside the kernels.  Byte equality with the numpy restatement (fastintercu_vvc_amd/motion.py) is asserted FIRST, at range 8, subpel 2, two references, and
subpel 0 with one reference is asserted equal to mlt_picture_predict.
Quality: a pair with a planted sub-sample shift -- cur = the compensation of a natural frame with the uniform vector (9, -6) quarter samples plus +-2 of noise;
reference 0 is that frame with a band of columns replaced by other content (an occlusion), reference 1 the frame moved by (3, 2) whole samples without the band --
and the mean |cur - dst| per sample for integer / half / quarter refinement with one and two references.  No threshold: what is printed is what is claimed.

  python scripts/motion_refs_ab.py [--steps 30] [--warmup 8] > profiles/motion_refs_ab.txt"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK, LAMBDA, RANGE = 16, 4, 16
CHECK_RANGE = 8


def frame(pkg, width, height, seed):
    cols, rows = (width + 127) // 128, (height + 127) // 128
    org, pred = pkg.synth.natural_patches(128, cols * rows, seed)
    tile = lambda p: np.ascontiguousarray(p.reshape(rows, cols, 128, 128).transpose(0, 2, 1, 3).reshape(rows * 128, cols * 128)[:height, :width])
    return tile(org), tile(pred)


def shifted(ref, sx, sy):
    h, w = ref.shape
    ys, xs = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(ref[np.clip(ys + sy, 0, h - 1), np.clip(xs + sx, 0, w - 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
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
    refs = [ref, shifted(ref, 2, -1), shifted(ref, -3, 1), shifted(ref, 1, 4)]
    m = pkg.MltCnn(device=0, sizes=(16,))
    p_cur = m.picture(W, H).upload(cur)
    p_refs = [m.picture(W, H).upload(r) for r in refs]
    dst, dst2 = m.picture(W, H), m.picture(W, H)
    bx, by = pkg.capi.motion_blocks(W, H, BLOCK)

    # byte equality first
    out = m.predict_picture_refs(p_cur, p_refs[:2], dst, block=BLOCK, search_range=CHECK_RANGE, lam=LAMBDA, subpel=2)
    want_plane, want_mv, want_ref, want_cost = pkg.motion.predict_refs(cur, refs[:2], BLOCK, CHECK_RANGE, LAMBDA, 2)
    same = bool(out["mv"].tobytes() == want_mv.tobytes() and out["ref"].tobytes() == want_ref.tobytes() and out["cost"].tobytes() == want_cost.tobytes()
                and dst.download().tobytes() == want_plane.tobytes())
    assert same, "device != numpy restatement"
    fractional = float((want_mv.reshape(-1, 2) & 3).any(axis=1).mean())
    second = float((want_ref != 0).mean())
    o0 = m.predict_picture_refs(p_cur, p_refs[:1], dst, block=BLOCK, search_range=RANGE, lam=LAMBDA, subpel=0)
    o1 = m.predict_picture(p_cur, p_refs[0], dst2, block=BLOCK, search_range=RANGE, lam=LAMBDA)
    same_int = bool(o0["mv"].tobytes() == o1["mv"].tobytes() and dst.download().tobytes() == dst2.download().tobytes())
    assert same_int, "subpel 0, one reference != mlt_picture_predict"

    def predict(rng):
        def leg():
            m.predict_picture(p_cur, p_refs[0], dst, block=BLOCK, search_range=rng, lam=LAMBDA, want_field=False)
            m.synchronize()
        return leg

    def predict_refs(subpel, n_refs):
        def leg():
            m.predict_picture_refs(p_cur, p_refs[:n_refs], dst, block=BLOCK, search_range=RANGE, lam=LAMBDA, subpel=subpel, want_field=False)
            m.synchronize()
        return leg

    legs = [("P8", predict(8)), ("P16", predict(16)), ("S0", predict_refs(0, 1)), ("S1", predict_refs(1, 1)), ("S2", predict_refs(2, 1)),
            ("S2x2", predict_refs(2, 2)), ("S2x4", predict_refs(2, 4))]
    n_refs_of = {"S0": 1, "S1": 1, "S2": 1, "S2x2": 2, "S2x4": 4}
    times = {name: [] for name, _ in legs}
    for k in range(a.warmup + a.steps):
        for name, leg in legs:
            t0 = time.perf_counter()
            leg()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                times[name].append(dt)
    kern = {}
    for name, leg in legs:
        m.profile_enable(True)
        for _ in range(a.steps):
            leg()
        prof = {p["name"]: p for p in m.profile_read()}
        m.profile_enable(False)
        if name in n_refs_of:
            assert prof["motion_search"]["launches"] == a.steps * n_refs_of[name] and prof["motion_refine"]["launches"] == a.steps
        assert prof["picture_compensate"]["launches"] == a.steps
        kern[name] = {k + "_us": round(1e3 * p["total_ms"] / a.steps, 2) for k, p in prof.items()}
    med = {k: statistics.median(v) for k, v in times.items()}
    rng = {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}

    # what it buys: a planted sub-sample shift, an occlusion in reference 0
    base = cur
    noise = np.random.default_rng(a.picture_seed).integers(-2, 3, size=(H, W)).astype(np.int16)
    q_cur = (pkg.motion.compensate(base, np.tile(np.array([9, -6], np.int16), (by, bx, 1)), BLOCK) + noise).astype(np.int16)
    q_ref0 = base.copy()
    q_ref0[:, W // 3: W // 3 + W // 8] = ref[:, W // 2: W // 2 + W // 8]
    q_ref1 = shifted(base, 3, 2)
    q_pics = [m.picture(W, H).upload(p) for p in (q_cur, q_ref0, q_ref1)]
    quality = {}
    for n_refs in (1, 2):
        for subpel in (0, 1, 2):
            m.predict_picture_refs(q_pics[0], q_pics[1:1 + n_refs], dst, block=BLOCK, search_range=RANGE, lam=LAMBDA, subpel=subpel, want_field=False)
            quality[f"refs{n_refs}_subpel{subpel}"] = round(float(np.abs(q_cur.astype(np.int32) - dst.download().astype(np.int32)).mean()), 4)
    row = {"picture": [W, H], "block": BLOCK, "lambda": LAMBDA, "range": RANGE, "blocks": [bx, by], "steps": a.steps, "warmup": a.warmup,
           "picture_seed": a.picture_seed, "device_equals_restatement_range8_subpel2_refs2": same, "subpel0_refs1_equals_mlt_picture_predict": same_int,
           "blocks_with_fractional_vector": round(fractional, 4), "blocks_on_reference_1": round(second, 4),
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": rng, "kernels": kern,
           "ratio_to_P16": {k: round(v / med["P16"], 3) for k, v in med.items()}, "mean_abs_residual_planted_shift": quality}
    for p in [p_cur, dst, dst2] + p_refs + q_pics:
        p.close()
    m.close()
    print(f"refinement and reference choice on a {W} x {H} frame, block {BLOCK}, lambda {LAMBDA}, sources {pkg.build.source_signature()}, {a.steps} alternating steps "
          f"after {a.warmup} warm-up")
    print(f"  {bx} x {by} blocks; device == numpy restatement at range {CHECK_RANGE}, subpel 2, two references (field, indices, costs, plane): {same}; "
          f"blocks with a fractional vector there: {100 * fractional:.1f} %, on reference 1: {100 * second:.1f} %")
    print(f"  subpel 0 with one reference == mlt_picture_predict at range {RANGE} (field, plane): {same_int}")
    what = {"P8": "mlt_picture_predict, range 8", "P16": "mlt_picture_predict, range 16", "S0": "predict_refs, 1 ref, subpel 0", "S1": "predict_refs, 1 ref, subpel 1",
            "S2": "predict_refs, 1 ref, subpel 2", "S2x2": "predict_refs, 2 refs, subpel 2", "S2x4": "predict_refs, 4 refs, subpel 2"}
    for name, _ in legs:
        print(f"  leg {name:<5} {what[name]:<32} median {med[name]:.3f} ms  (min {rng[name][0]:.3f}, max {rng[name][1]:.3f})   = {med[name] / med['P16']:.2f} x leg P16")
        print("            " + ", ".join(f"{k[:-3]} {v:.1f} us" for k, v in kern[name].items()))
    print("  mean |cur - dst| per sample, planted shift (9, -6) quarter samples + noise of +-2, an occluded band in reference 0:")
    for n_refs in (1, 2):
        print(f"    {n_refs} reference(s): integer {quality[f'refs{n_refs}_subpel0']:.3f}, half {quality[f'refs{n_refs}_subpel1']:.3f}, quarter {quality[f'refs{n_refs}_subpel2']:.3f}")
    print(json.dumps({"source_sig": pkg.build.source_signature(), "result": row}))


if __name__ == "__main__":
    main()
