"""The weight-gradient family on the GPU through HipOps: gan_conv_wgrad's generic kernel (bf16 and fp32), the range-patch kernel and
the two 7x7 window kernels, gan_wgrad_reduce and gan_bias_grad, against the float64 statements of tests/wgrad_ref64.py with the bounds
the project derives (tests/cases.derived_bound; for the reduction alone the worst-case bound of any summation order).
tests/test_wgrad_family_cpu.py runs the same bodies on the emulator and shows that the bounds admit it and reject the listed mistakes.

What the cases reach that the square twins of tests/test_gpu_parity.py and the bench-size tests do not: both addressing paths of the
generic kernel on non-square maps, M < 64, the zeroed tail of a split, splits that begin in the middle of an image, each slab on its
own, the skinny tiles, the tap and channel clamps, Wo = 1 and Ho = 1, fp32 off the squares, accumulate = 1 everywhere, every lane count
of the reduction and its stride loop, the bias gradient at one chunk lane, at its block cap and with a ragged last block, the persistent
walk of the window kernels past 256 tiles, and one NaN.  Each case asserts from the planned call that it reached the kernel it names."""
import pytest
import torch

from gan_variant_research_amd.runtime import Ctx, HipOps
from tests import wgrad_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make(dtype):
    return Ctx(HipOps(torch.device(DEV)), DEV, dtype)


@pytest.mark.parametrize("S", W.CASES, ids=W.case_id)
def test_case_within_the_derived_bounds(S):
    """one planned weight gradient: the kernel it names, guard zones, every slab element written, bit-unchanged operands, repeat
    (tests/wgrad_cases.run), then grad_w, the sum of the slabs, each slab of the generic kernel and grad_b against float64"""
    W.check(make, S)


@pytest.mark.parametrize("S", W.ACCUMULATE, ids=W.case_id)
def test_accumulate_is_one_fp32_addition(S):
    W.check_accumulate(make, S)


def test_bias_accumulate_can_differ():
    W.check_accumulate(make, W.BIAS_ACCUMULATE_DIFFERS, bias_differs=True)


@pytest.mark.parametrize("where", ["dy", "x"])
@pytest.mark.parametrize("S", W.NAN_CASES, ids=W.case_id)
def test_one_nan_stays_in_its_footprint(S, where):
    """every element whose float64 reference is NaN is NaN, every other one is bit-identical to the clean run: the excused set is empty"""
    W.check_nan(make, S, where)


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("r", W.REDUCE + W.REDUCE_PAST_THE_GRID, ids=W.rcase_id)
def test_reduction_alone(r, accumulate):
    W.body_reduce(make, r, accumulate)


@pytest.mark.parametrize("halo", [0, 2])
@pytest.mark.parametrize("b", W.BIAS, ids=W.bcase_id)
def test_bias_gradient_alone(b, halo):
    W.body_bias(make, b, halo)


def test_family_has_a_figure_for_every_variant():
    """the worst error / bound per kernel variant; a variant without a figure fails (a case that misses fails in its own test)"""
    W.summary(make)


@pytest.mark.parametrize("wrong", W.WRONG, ids=lambda w: w.__name__)
def test_family_rejects_a_wrong_reference(wrong):
    """The kernels' results held to a deliberately wrong reference: the assertions fail.  The kernels are never made to misbehave."""
    W.rejects(make, wrong)


def test_refused_descriptors_return_their_error_and_leave_the_sentinel():
    assert W.body_refused(HipOps(torch.device(DEV)), DEV) >= 15
