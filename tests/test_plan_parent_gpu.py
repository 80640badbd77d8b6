"""fp8 + fp8_wgrad iterations of both fused trainers on the GPU equal, bit for bit, what the commit before the planner's bf16 and e4m3
paths were merged computed (the existing bit-level goldens cover the modes with the switches off)."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_plan as M  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_parent_gpu.json")


@pytest.mark.parametrize("which", ["cut", "basic"])
def test_fp8_wgrad_iteration_equals_the_parents_to_the_bit(which):
    """One iteration at 64x64, batch 2 with fp8 + fp8_wgrad: the losses and every optimiser's parameter block equal
    tests/golden/plan_parent_gpu.json, recorded ON the parent commit on an MI355X by tools/make_golden_plan.py gpu (float.hex() of the
    losses, SHA-256 of the parameter blocks; there the iteration ran twice from fresh trainers and gave the same bits)."""
    want = json.load(open(GOLDEN))[which]
    got = M.gpu_iteration(which)
    print(which, {k: float.fromhex(v) for k, v in got["losses"].items()}, {k: float.fromhex(v) for k, v in want["losses"].items()})
    assert got == want
