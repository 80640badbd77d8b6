"""PatchNCE with negatives from the whole minibatch (gan_patchnce_all_*, csrc/patchnce.hip) on the GPU through HipOps, element by element
against the float64 statement of tests/nce_all_ref64.py with the derived bounds of tests/nce_all_cases.py (tests/test_nce_all_cpu.py runs
the same bodies on the emulator): the loss increment on a prior loss, Sn, Tn, tnorm, lse, rowloss, flag and dX in the workspace, gtgt on a
prior with duplicates accumulating, sentinels in halos, in channels >= C, past the workspace and between key segments, the same bits from a
repeated call; less than one key tile, several key trips with a tail, full tiles, the scalar path's shapes (Q = 1, 2, 51, 200, C = 40, 320,
512, B = 257), foreign key segments with self = 0, 1, 2, the clamp, the eps branch, non-finite rows in the own and in a foreign segment."""
import pytest
import torch

from gan_variant_research_amd import BF16
from gan_variant_research_amd.runtime import Ctx, HipOps
from tests import nce_all_cases as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make():
    return Ctx(HipOps(torch.device(DEV)), DEV, BF16)


@pytest.mark.parametrize("r", N.RUNS, ids=N.run_id)
def test_kernels_within_the_derived_bounds(r):
    N.body(make, r)


@pytest.mark.parametrize("r", N.EQUIV, ids=N.run_id)
def test_b1_s1_agrees_with_the_per_image_entry_points(r):
    N.body_equivalence(make, r)


def test_refused_arguments_return_their_error_and_write_nothing():
    N.body_refused(make)


@pytest.mark.parametrize("wrong,runs", N.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_rejects_a_wrong_reference(wrong, runs):
    """The kernels' results held to a deliberately wrong reference fail.  The kernels are never made to misbehave."""
    N.rejects(make, wrong, runs)
