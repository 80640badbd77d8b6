"""The module-API discriminators on the GPU after the autograd bridge moved onto nets.DiscriminatorFamilyNet compute, bit for bit, what
the commit before computed: the move only reorders independent launches on the bridge's single stream."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_dfamily_plan as M  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dfamily_bridge_parent_gpu.json")


def test_every_case_of_the_tool_is_in_the_golden_file():
    """Every case was bit-reproducible on the parent commit, so none was left out of the record."""
    assert sorted(json.load(open(GOLDEN))) == sorted(M.GPU_TAGS)


@pytest.mark.parametrize("tag", M.GPU_TAGS)
def test_bridge_equals_the_parents_to_the_bit(tag):
    """ms3 / sn2 / bsn of tests/golden/cut_optional.npz in fp32: every scale's logits, the input and parameter gradients of
    optional_cases' loss mix, R1 with its parameter gradients and weight_u / weight_v afterwards equal
    tests/golden/dfamily_bridge_parent_gpu.json, recorded ON the parent commit on an MI355X by tools/make_golden_dfamily_plan.py gpu
    (SHA-256 of the tensors, float.hex() of the scalars; there each case ran twice from fresh modules and gave the same bits)."""
    want = json.load(open(GOLDEN))[tag]
    got = M.bridge_bits(tag)
    print(tag, "differing:", [k for k in want if got.get(k) != want[k]])
    assert got == want
