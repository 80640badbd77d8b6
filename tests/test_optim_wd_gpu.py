"""gan_adam_step_wd on the GPU through HipOps, element by element against the float64 statement of tests/optim_wd_ref64.py with the derived
bounds of tests/optim_wd_cases.py (tests/test_optim_wd_cpu.py runs the same bodies on the emulator): both decay modes over tensors that cross
the 16384-element chunk, tail chunks, unaligned slices, a skipped tensor in the middle of the grid, hard clipping and none, GradScaler's
scales, the device learning rate, EMA on and off, chained steps, an exactly-zero gradient, NaN and +-Inf with and without skip_nonfinite,
the four builders, weight_decay = 0 against gan_adam_step, and the refused arguments."""
import pytest
import torch

from gan_variant_research_amd import BF16
from gan_variant_research_amd.runtime import Ctx, HipOps
from tests import optim_wd_cases as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make():
    return Ctx(HipOps(torch.device(DEV)), DEV, BF16)


@pytest.mark.parametrize("c", Q.CASES, ids=Q.case_id)
def test_family_within_the_derived_bounds(c):
    Q.body(make, c)


@pytest.mark.parametrize("wrong,names", Q.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_family_rejects_a_wrong_reference(wrong, names):
    """The kernels' results held to a deliberately wrong reference fail.  The kernels are never made to misbehave."""
    Q.rejects(make, wrong, names)


@pytest.mark.parametrize("decoupled", [False, True])
def test_zero_decay_is_adam_step_bit_for_bit(decoupled):
    Q.body_zero_decay_is_adam_step(make, decoupled)


def test_refused_arguments_return_their_error_and_write_nothing():
    Q.body_refused(make)


def test_worst_ratios_are_reported_and_no_bound_is_idle():
    for c in Q.CASES:          # run alone, this test fills the table itself (results are cached per case)
        Q.body(make, c)
    worst = Q.worst_table(True)
    idle = {g: r for g, r in worst.items() if r < 0.01}
    assert not idle, f"bounds too loose to catch anything: {idle}"
