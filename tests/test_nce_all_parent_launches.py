"""With patchnce.nce_includes_all_negatives_from_minibatch false or absent, cut.CutTrainer builds launch for launch the PatchNCE term of the
commit before the key was read: the same entry points in the same order in the G-features program and in its backward (the hooks), the same
scalars, view geometries and workspace sizes (tools/make_golden_nce_parent.py lists the cases and what a record holds)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_nce_parent as M  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(M.GOLDEN) as f:
        return json.load(f)


def test_every_case_of_the_tool_is_in_the_golden_file(golden):
    assert sorted(golden) == sorted(M.CASES)
    assert golden["absent"] == golden["false"] and len(golden["false"]["nce"]) == 16 and golden["no-nce"]["nce"] == []


@pytest.mark.parametrize("name", list(M.CASES))
def test_builds_the_parents_launches(golden, name):
    """tests/golden/nce_parent_launches.json was recorded ON the parent commit by tools/make_golden_nce_parent.py (copied into its tree); it
    is not recomputed from the code under test."""
    want, got = golden[name], M.record(name)
    assert got["ws_floats"] == want["ws_floats"]
    assert len(got["nce"]) == len(want["nce"])
    for i, (g, w) in enumerate(zip(got["nce"], want["nce"])):
        assert g == w, (i, g, w)
    assert got["programs"] == want["programs"]
