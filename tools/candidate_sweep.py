#!/usr/bin/env python3
"""Choose a candidate policy before re-encoding: how many split modes would stay in the RDO?  CPU only.

Reads a call dump (host/mlt_split_predictor.hpp, MLTCNN_CALL_DUMP_FILE in a -DMLTCNN_TEST_HOOKS build: every predictSplitMode call with all
its head logits) and prints, per CU size and per (coverage, max_modes) of a grid, the histogram of the kept count, the share of the calls the
cap sends to full RDO (every class kept) and the mean number of kept modes -- what MLTCNN_CANDIDATES / mlt_set_candidate_policy would hand the
encoder.  The records are evaluated with decisions.candidates_from_logits, the host restatement of what the device computes.

  python tools/candidate_sweep.py calls.bin [--coverage 0.5,0.8,0.9,0.95,0.99] [--max-modes 0,2,3] [--head 128:2,64:3] [--json]"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEFAULT_COVERAGE = (0.5, 0.8, 0.9, 0.95, 0.99)
DEFAULT_MAX_MODES = (0, 2, 3)


def _decisions():
    """fastintercu-vvc_amd/decisions.py on its own (numpy only: the sweep needs neither torch nor the HIP library)."""
    spec = importlib.util.spec_from_file_location("mlt_decisions", os.path.join(ROOT, "fastintercu-vvc_amd", "decisions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sweep(calls, coverage=DEFAULT_COVERAGE, max_modes=DEFAULT_MAX_MODES, heads=None) -> dict:
    """calls: records of read_call_dump -> {size: {"calls", "decision_head", "classes", "policies": [{"coverage", "max_modes", "kept_count_histogram" (index 0 = one
    class kept), "full_rdo", "full_rdo_share", "mean_kept"}]}}.  A cap above the head's class count is skipped for that size."""
    dec = _decisions()
    by_size = {}
    for c in calls:
        if c["cuw"] in dec.HEAD_CLASSES and len(c["logits"]) == sum(dec.HEAD_CLASSES[c["cuw"]]):
            by_size.setdefault(c["cuw"], []).append(c["logits"])
    rep = {}
    for size, lg in sorted(by_size.items(), reverse=True):
        lg = np.stack(lg)
        head = (heads or {}).get(size)
        dh = dec.default_head(size) if head is None else head
        K = dec.HEAD_CLASSES[size][dh]
        rows = []
        for cov in coverage:
            for mx in max_modes:
                if mx > K:
                    continue
                c = dec.candidates_from_logits(size, lg, head_index=dh, coverage=float(cov), max_modes=int(mx))
                hist = np.bincount(c["count"], minlength=K + 1)[1:]
                full = int((c["count"] == K).sum())
                rows.append({"coverage": float(cov), "max_modes": int(mx), "kept_count_histogram": [int(v) for v in hist], "full_rdo": full,
                             "full_rdo_share": full / len(c), "mean_kept": float(c["count"].mean())})
        rep[size] = {"calls": int(len(lg)), "decision_head": dh, "classes": K, "policies": rows}
    return rep


def format_report(rep: dict) -> str:
    lines = []
    for size, r in rep.items():
        lines.append(f"size {size}: {r['calls']} calls, decision head {r['decision_head']} ({r['classes']} classes)")
        for t in r["policies"]:
            hist = " ".join(f"{k + 1}:{v}" for k, v in enumerate(t["kept_count_histogram"]))
            lines.append(f"  coverage {t['coverage']:.3f} max {t['max_modes']}  full RDO {t['full_rdo']:6d} ({100.0 * t['full_rdo_share']:5.1f} %)  "
                         f"mean kept {t['mean_kept']:.3f}  by kept count  {hist}")
    return "\n".join(lines)


def _pairs(text, cast):
    return {int(k): cast(v) for k, v in (tok.split(":", 1) for tok in text.split(",") if tok)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dump")
    ap.add_argument("--coverage", default=",".join(str(v) for v in DEFAULT_COVERAGE), help="comma-separated coverages, each in [0, 1)")
    ap.add_argument("--max-modes", default=",".join(str(v) for v in DEFAULT_MAX_MODES), help="comma-separated caps (0 = none), each in [0, 6]")
    ap.add_argument("--head", default="", help="decision head per size, e.g. 128:2,64:3 (default: the reference's)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args(argv)
    cov = [float(v) for v in a.coverage.split(",") if v]
    caps = [int(v) for v in a.max_modes.split(",") if v]
    if not cov or any(not (0.0 <= v < 1.0) for v in cov):
        raise SystemExit("--coverage: values must lie in [0, 1)")
    if not caps or any(not (0 <= v <= 6) for v in caps):
        raise SystemExit("--max-modes: values must lie in [0, 6]")
    from run_ra_eval import read_call_dump
    rep = sweep(read_call_dump(a.dump), cov, caps, _pairs(a.head, int) if a.head else None)
    if not rep:
        raise SystemExit(f"{a.dump} holds no call of a known CU size")
    print(json.dumps(rep, indent=1) if a.json else format_report(rep))
    return 0


if __name__ == "__main__":
    sys.exit(main())
