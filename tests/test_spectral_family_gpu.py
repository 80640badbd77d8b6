"""gan_spectral_norm_fwd / _bwd and gan_spectral_norm_batch_fwd / _bwd on the GPU through HipOps, element by element against the float64
statements of tests/spectral_ref64.py with the derived bounds of tests/spectral_cases.py (tests/test_spectral_family_cpu.py runs the same
bodies on the emulator).

What the tables reach that test_batched_spectral_norm_vs_float64 and test_spectral_norm_twins do not: h at 31 / 32 / 33 and w at 255 / 256 /
257 (the tile edges), 512 x 4352 (272 tiles: the second trip of the tile-partial loop of the backward, and w > 1024 in the finishing
block), 1030 x 40 (its row loop), descriptor tables of 1, 2, 3, 16 and 17 entries with runs of one-tile descriptors and the largest first,
in the middle and last (the binary search), the single-matrix kernels past their 1024-thread, 256-partial and 2048-block limits, rank-one,
cancelling, all-zero, 1e15 and range-end weights, G = W_sn and G orthogonal to W, sentinels behind every output and both workspaces, repeated
calls, a NaN in one descriptor of three, and the refused arguments."""
import pytest
import torch

from gan_variant_research_amd import BF16
from gan_variant_research_amd.runtime import Ctx, HipOps
from tests import spectral_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make():
    return Ctx(HipOps(torch.device(DEV)), DEV, BF16)


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_family_within_the_derived_bounds(c):
    P.body(make, c)


@pytest.mark.parametrize("where", ["W", "u", "G"])
def test_nan_stays_in_its_descriptor(where):
    P.body_nonfinite(make, where)


@pytest.mark.parametrize("where", ["W", "u", "v", "G"])
def test_nan_single_matrix_path(where):
    P.body_nonfinite_single(make, where)


def test_refused_arguments_return_their_error_and_write_nothing():
    P.body_refused(make)


@pytest.mark.parametrize("wrong,names", P.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_family_rejects_a_wrong_reference(wrong, names):
    """The kernels' results held to a deliberately wrong reference fail.  The kernels are never made to misbehave."""
    P.rejects(make, wrong, names)


def test_worst_ratios_are_reported_and_no_bound_is_idle():
    for c in P.CASES:          # run alone, this test fills the table itself (results are cached per case)
        P.body(make, c)
    worst = P.worst_table(True)
    idle = {g: r for g, r in worst.items() if r < 0.01}
    assert not idle, f"bounds too loose to catch anything: {idle}"
