"""The range-patch weight gradient after the stage ring (csrc/wgrad_patch.hip: 64-pixel stages, a ring of g tiles and x image rows, LDS-DMA
waits counted by hand) computes the bits it computed before: every accumulator keeps its summation order (stages in pixel order, k-steps in
order, one k permutation), so the partial slabs `part` and the reduced gradient equal tests/golden/wgrad_patch_parent.json -- recorded by
tools/make_golden_wgrad_patch.py on the commit before the ring -- bit for bit, and the golden itself is held to float64."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import wgrad_patch_ring_cases as W                                      # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_patch_parent.json")
_runs = {}


def result(kind, shape):
    """One launch per case, shared by the tests below and left unchanged."""
    key = W.case_id(kind, shape)
    if key not in _runs:
        _runs[key] = W.run(kind, shape)
    return _runs[key]


@pytest.mark.parametrize("kind,shape", W.CASES, ids=[W.case_id(k, s) for k, s in W.CASES])
def test_part_and_gradient_equal_the_parent_commit(kind, shape):
    with open(GOLDEN) as f:
        want = json.load(f)[W.case_id(kind, shape)]
    r = result(kind, shape)
    got = {"nsplit": r["nsplit"], "part": W.sha(r["part"]), "grad": W.sha(r["grad"])}
    assert got == want


@pytest.mark.parametrize("kind,shape", W.CASES, ids=[W.case_id(k, s) for k, s in W.CASES])
def test_summed_part_within_fp32_accumulation_of_float64(kind, shape):
    """sum_s part[s] against float64 on the operands the kernel multiplied.  Every product of two bf16 (or e4m3) values is exact in fp32, so
    an accumulator's error is its additions': K of them for the K = B * H * W / nsplit pixels of a split (rounded up to whole 128-pixel
    ranges), each at most one fp32 ulp (2^-23, which also covers a truncating adder inside the MFMA) of a running sum that never exceeds the
    sum of the |products|.  Hence |sum_s part[s] - ref| <= K * 2^-23 * sum |g| |x|, element by element; the sum over s is taken in float64."""
    B, H, W_, Cx, N = shape
    r = result(kind, shape)
    assert torch.isfinite(r["part"]).all(), "a slab element was not written"
    got = r["part"].double().sum(0)
    ref, ref_abs = W.ref64(r), W.ref64(r, absolute=True)
    per = (B * H * W_ + r["nsplit"] - 1) // r["nsplit"]
    K = (per + 127) // 128 * 128
    bound = K * 2.0 ** -23 * ref_abs
    excess = ((got - ref).abs() - bound).max().item()
    worst = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"{W.case_id(kind, shape)}: nsplit {r['nsplit']}, K {K}, max |err| / bound = {worst:.3e}")
    assert excess <= 0.0, (excess, worst)
