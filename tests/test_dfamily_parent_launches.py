"""The discriminator family after its three host-side planners became one (nets.DiscriminatorFamilyNet / DFamilyPass under both fused
trainers and under the autograd bridge) plans what the commit before planned: the fused trainers exactly the same launches -- same op,
same arguments, same stream, same order -- and the bridge the same launches with independent ones reordered on its single stream
(tools/make_golden_dfamily_plan.py lists the records and what each one reaches)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_dfamily_plan as M  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dfamily_parent_launches.json")


def test_every_record_of_the_tool_is_in_the_golden_file():
    blob = json.load(open(GOLDEN))
    assert sorted(blob["launches"]["records"]) == sorted(M.RECORDS) and sorted(blob["bridge"]) == sorted(M.BRIDGE)


@pytest.mark.parametrize("name", list(M.RECORDS))
def test_fused_trainers_plan_the_parents_launches(name):
    """tests/golden/dfamily_parent_launches.json was recorded ON the parent commit by tools/make_golden_dfamily_plan.py (copied into its
    tree) with tests.emulator_fp8wgrad.LaunchLog -- it is not recomputed from the code under test."""
    want = M.unpack(json.load(open(GOLDEN))["launches"])[name]
    log = M.plan(name)
    got = log.hashed()
    print(name, "launches:", len(got), "parent:", len(want))
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w, log.entries[i])


@pytest.mark.parametrize("name", list(M.BRIDGE))
def test_bridge_plans_the_parents_launches_order_aside(name):
    """Per phase (a slot's forward, its backward with each (need_x, need_w), R1) the bridge plans as many launches of every op on every
    stream as the parent did.  Their order is not compared: layout conversions moved out from between the scales and R1 forwards every
    scale before the first-order halves, as the fused trainer always did -- independent launches of one stream."""
    want = json.load(open(GOLDEN))["bridge"][name]
    got = M.bridge_counts(name)
    print(name, {p: sum(c.values()) for p, c in got.items()})
    assert list(got) == list(want)
    for phase in want:
        assert got[phase] == want[phase], phase
