"""gan_adam_step, gan_scaler_update, gan_fill_f32 and gan_axpy_f32 on the GPU through HipOps, element by element against the float64
statements of tests/optim_ref64.py with the derived bounds of tests/optim_cases.py (tests/test_optim_family_cpu.py runs the same bodies on
the emulator).

What the tables reach that test_adam_twins and test_adam_gradscaler_knobs_twins do not: tensors that cross the 16384-element chunk, tail
chunks, more than 256 chunks (the second trip of the partial-sum loop) and more than 64 tensors (five blocks of the counter kernel),
skipped tensors in the middle of the grid, unaligned slices, both arms of the lerp and their boundary, saturated bias corrections, the
coefficient where + 1e-6 matters, the device learning rate and 1 / scale, gradients at both ends of the range where their squares stay
normal, NaN and +-Inf in read and unread tensors with and without skip_nonfinite and clipping, sentinels behind the workspace, norm_out
and around every slice, repeated calls, and the refused arguments."""
import pytest
import torch

from gan_variant_research_amd import BF16
from gan_variant_research_amd.runtime import Ctx, HipOps
from tests import optim_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make():
    return Ctx(HipOps(torch.device(DEV)), DEV, BF16)


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_family_within_the_derived_bounds(c):
    P.body(make, c)


@pytest.mark.parametrize("name", list(P.SCALER_SEQS))
def test_scaler_update(name):
    P.body_scaler(make, name)


@pytest.mark.parametrize("n", P.HELPER_N)
def test_fill_and_axpy(n):
    P.body_fill_axpy(make, n)


def test_refused_arguments_return_their_error_and_write_nothing():
    P.body_refused(make)


@pytest.mark.parametrize("wrong,names", P.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_family_rejects_a_wrong_reference(wrong, names):
    """The kernels' results held to a deliberately wrong reference fail.  The kernels are never made to misbehave."""
    P.rejects(make, wrong, names)


def test_worst_ratios_are_reported_and_no_bound_is_idle():
    for c in P.CASES:          # run alone, this test fills the table itself (results are cached per case)
        P.body(make, c)
    for name in P.SCALER_SEQS:
        P.body_scaler(make, name)
    P.body_fill_axpy(make, 257)
    worst = P.worst_table(True)
    idle = {g: r for g, r in worst.items() if r < 0.01}
    assert not idle, f"bounds too loose to catch anything: {idle}"
