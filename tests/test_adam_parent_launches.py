"""training.HipAdam and training.fused_adam_launch on runtime.AdamPlan build exactly the optimiser launches of the commit before it: same
entry point, same scalars, same chunk lists, same workspace sizes, same table entries, the same rate in lr_dev at every run, and as many
plans and tables (tools/make_golden_adam.py lists the cases and what a record holds)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_adam as M  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(M.GOLDEN) as f:
        return json.load(f)


def test_every_case_of_the_tool_is_in_the_golden_file(golden):
    assert sorted(golden) == sorted(M.CASES)


@pytest.mark.parametrize("name", list(M.CASES))
def test_builds_the_parents_launches(golden, name):
    """tests/golden/adam_parent_launches.json was recorded ON the parent commit by tools/make_golden_adam.py (copied into its tree); it is
    not recomputed from the code under test."""
    want, got = golden[name], M.record(name)
    assert len(got["calls"]) == len(want["calls"]), (len(got["calls"]), len(want["calls"]))
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, (i, {k: (g[k], w[k]) for k in w if g.get(k) != w[k]})
    assert got["tables"] == want["tables"] and got["plans"] == want["plans"]
    if name.startswith(("hipadam", "fused")):      # a moved rate keeps the plan, the table and the launch: one record ran at both rates
        assert want["plans"][:2] == [1, 1] and len(want["calls"][0]["rates"]) == 2 and len(set(want["calls"][0]["rates"])) == 2
