"""The planner after its bf16 and e4m3 paths were merged (one builder per direction in convplan.py, one residual-convolution backward in
nets.py) plans exactly the launches of the commit before the merge: same op, same arguments, same stream, same order, in both fused
trainers and in every mode the merged arms serve (tools/make_golden_plan.py lists the records and what each one reaches)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_plan as M  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_parent_launches.json")


def test_every_record_of_the_tool_is_in_the_golden_file():
    assert sorted(json.load(open(GOLDEN))["records"]) == sorted(M.RECORDS)


@pytest.mark.parametrize("name", list(M.RECORDS))
def test_plans_the_parents_launches(name):
    """tests/golden/plan_parent_launches.json was recorded ON the parent commit by tools/make_golden_plan.py (copied into its tree) with
    tests.emulator_fp8wgrad.LaunchLog -- it is not recomputed from the code under test."""
    want = M.unpack(json.load(open(GOLDEN)))[name]
    log = M.plan(name)
    got = log.hashed()
    print(name, "launches:", len(got), "parent:", len(want))
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w, log.entries[i])
