"""The partition tree's descent driven from the HOST: decisions.build_tree over MltCnn.predict_at, level by level -- the anchor that mlt_predict_tree
(tests/test_tree_gpu.py) and slices of mlt_predict_trees (tests/test_trees_gpu.py) are compared with byte for byte.  Needs the MI355X through its callers."""
import numpy as np

from tree_gpu_common import SIZES, reruns

ALL = ("split", "logits", "decisions", "candidates")


def host_tree(pkg, m, p_org, p_pred, width, height, top=128, min_size=16, descend=None, by_candidates=False, poc=0, qp=0):
    """The descent driven from the host: build_tree over m.predict_at -> (nodes, leaf_map, per-node logits [n, 15] / decisions / candidates, guard re-runs)."""
    rec = {"logits": [], "decisions": [], "candidates": []}

    def decide(size, xy):
        r = m.predict_at(size, p_org, p_pred, xy, np.full(len(xy), poc, np.int32), np.full(len(xy), qp, np.int32), want=ALL)
        assert np.array_equal(r["split"], r["decisions"]["split_mode"])
        row = np.zeros((len(xy), 15), np.float32)
        row[:, :r["logits"].shape[1]] = r["logits"]
        rec["logits"].append(row)
        rec["decisions"].append(r["decisions"])
        rec["candidates"].append(r["candidates"])
        return r["decisions"]["split_mode"], r["decisions"]["confidence"], r["candidates"]["mask"]

    sizes = [s for s in SIZES if min_size <= s <= top]
    r0 = reruns(m, sizes)
    nodes, leaf_map = pkg.decisions.build_tree(width, height, top, min_size, descend, decide, by_candidates)
    return nodes, leaf_map, {k: np.concatenate(v) for k, v in rec.items()}, reruns(m, sizes) - r0
