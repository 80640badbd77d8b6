"""The PatchNCE kernels of csrc/patchnce.hip on the GPU through HipOps, element by element against the float64 statement of
tests/nce_ref64.py with the derived bounds of tests/nce_cases.py (tests/test_nce_family_cpu.py runs the same bodies on the emulator).

What the cases reach that test_patchnce_twins does not: the clamp at +-50 and its zero gradient, the eps branch of the normalisation in
source and target rows, Inf / NaN in a sampled row (flag 0, nothing added to the loss, that image's part of gtgt bit for bit its prior) and
outside the sampled rows, the tile edges of the MFMA path (P = 16, 48, 80, 240; C = 192), the scalar path's (P = 1, 17; C = 40, 320, 512),
C below the view's channel count, B = 257 and B = 5, all-equal ids, duplicates across the 64-position chunks, a non-square map, rows of
norm 5e18, and the call sequence: a prior loss, a prior gtgt, sentinels in halos, in channels >= C and past the workspace's extent, and
the same bits from a repeated call.  The workspace intermediates (Sn, Tn, tnorm, lse, rowloss, flag, dX; layout in include/mi355x_gan.h)
are held to the reference too.
"""
import pytest
import torch

from gan_variant_research_amd import BF16
from gan_variant_research_amd.runtime import Ctx, HipOps
from tests import nce_cases as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make():
    return Ctx(HipOps(torch.device(DEV)), DEV, BF16)


@pytest.mark.parametrize("r", N.RUNS, ids=N.run_id)
def test_family_within_the_derived_bounds(r):
    N.body(make, r)


def test_refused_arguments_return_their_error_and_write_nothing():
    N.body_refused(make)


@pytest.mark.parametrize("wrong,runs", N.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_family_rejects_a_wrong_reference(wrong, runs):
    """The kernels' results held to a deliberately wrong reference fail.  The kernels are never made to misbehave."""
    N.rejects(make, wrong, runs)
