"""GPU (MI355X): the profile table of the picture and tree entry points is the committed one.

tests/golden/tree_profile_rows.json holds mlt_profile_read's rows -- name, launches, bytes, in order; no times -- for one call each of predict_at,
predict_at_sweep, predict_tree, predict_trees, predict_tree_sweep and predict_trees_sweep on a fixed case (seeded weights, synthetic pictures: deterministic),
captured by scripts/tree_profile_rows.py on the commit the file names, where a second run in the process and a second process gave the same rows.  The byte-equality
tests of the tree modules do not see the profile table; this one replays the case and asserts the rows EQUAL: names, order, launch counts and bytes."""
import importlib.util
import json
import os

import pytest

from tree_gpu_common import gpu   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_are_the_committed_ones(gpu):
    with open(os.path.join(ROOT, "tests", "golden", "tree_profile_rows.json")) as fh:
        golden = json.load(fh)
    spec = importlib.util.spec_from_file_location("tree_profile_rows", os.path.join(ROOT, "scripts", "tree_profile_rows.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert golden["reproduced"] and golden["case"] == tool.CASE, "the committed capture is of another case than the tool replays"
    got = tool.rows(gpu)
    assert list(got) == list(golden["rows"]) == tool.CASE["calls"]
    for call in tool.CASE["calls"]:
        want = golden["rows"][call]
        print(call, [(r[0], r[1]) for r in got[call] if "tree" in r[0] or "gather" in r[0]])
        assert [r[0] for r in got[call]] == [r[0] for r in want], (call, "names or order")
        for g, w in zip(got[call], want):
            assert g == w, (call, g, w)
