"""The loss, augmentation, pooling and layout kernels (csrc/pointwise.hip; gan_nchw_to_view, gan_view_to_nchw, gan_view_copy of
csrc/norm.hip) on the GPU through HipOps, element by element against the float64 statements of tests/pointwise_ref64.py with the derived
bounds of tests/pointwise_cases.py (tests/test_pointwise_family_cpu.py runs the same bodies on the emulator).

What the cases reach that test_layout_and_losses_twins and test_avgpool_twins do not: the second trip of every grid-stride loop (the
one-block sums past 1024 pixels, the L1 / R1 partials past 512 x 256 pixels, the 4096 x 256 grid cap, the one-block patch loss past 1024
logits), the hinge kinks, expf underflow in the BCE, x == t in L1, every DiffAugment edge (shifts by H - 1 and H, clipped, whole and
one-pixel cutouts, saturation 0 and contrast about a large mean), pooled sizes from 1 x 1 with short last windows, reflect and replicate
halos at their limits, loss scalars held to the fp32 summation bound in bf16 too, sentinels in halos, pad channels and workspaces, repeated
calls, NaN and Inf in read and unread elements, and the refused arguments.
"""
import pytest
import torch

from gan_variant_research_amd import BF16
from gan_variant_research_amd.runtime import Ctx, HipOps
from tests import pointwise_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make():
    return Ctx(HipOps(torch.device(DEV)), DEV, BF16)


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_family_within_the_derived_bounds(c):
    P.body(make, c)


def test_refused_arguments_return_their_error_and_write_nothing():
    P.body_refused(make)


@pytest.mark.parametrize("wrong,cases", P.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_family_rejects_a_wrong_reference(wrong, cases):
    """The kernels' results held to a deliberately wrong reference fail.  The kernels are never made to misbehave."""
    P.rejects(make, wrong, cases)


def test_worst_ratios_are_reported_and_no_bound_is_idle():
    """error / bound per group and dtype over everything above; a group whose worst ratio is below 0.01 has a bound too loose to catch
    anything (the copies are exact: their ratio is 0 by construction)"""
    worst = P.worst_table()
    idle = {key: r for key, r in worst.items() if key[0] not in ("layout", "aug_sums") and r < 0.01}
    assert not idle, f"bounds too loose to catch anything: {idle}"
