"""The InstanceNorm kernel family of csrc/norm.hip on the GPU through HipOps, element by element against the float64 statements of
tests/norm_ref64.py with the derived bounds of tests/norm_cases.py (tests/test_norm_family_cpu.py runs the same bodies on the emulator
and shows that the bounds admit an honest fp32 implementation and reject the listed mistakes).

What the cases reach that the twins of tests/test_gpu_parity.py do not: exactly 96 statistics chunks and 16 partials, a capped chunk
count with an empty and a short last chunk, one chunk lane with 256 row lanes on a 5-wide map, 256 chunk lanes with one row lane,
C = 512 / 1024 / 2048 (the limits of the backward, of gan_in_apply_parts and of the forward), the reflect fold at H = 2 pad + 2, the
two-level bias sum, HW = 1, and data with a mean (mean / sigma up to 100 inside the bounded group; 1000 in the known-limit group).
Outputs and workspaces start from a sentinel: halos a mode does not write and floats past every documented extent must keep it, and a
repeated call must give the same bits.
"""
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd.runtime import Ctx, HipOps
from tests import norm_cases as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make():
    return Ctx(HipOps(torch.device(DEV)), DEV, BF16)


@pytest.mark.parametrize("group", ["stats", "apply", "bwd", "fold"])
@pytest.mark.parametrize("p", N.CASE_IDS, ids=N.case_id)
def test_family_within_the_derived_bounds(p, group):
    """stats: gan_in_stats, gan_in_partial + gan_in_stats_from_parts, the statistics gan_in_apply_parts writes, gan_in_finalize;
    apply: gan_in_apply / gan_in_apply_parts x activation x residual x halo mode, given the statistics the producer wrote;
    bwd: gan_in_bwd (with and without g2), gan_in_bwd_bias (overwrite, accumulate; bias_grad against the float64 sum of the rows
    gan_in_bwd_bias_deferred hands out, one- and two-level), gan_in_bwd_bias_deferred, gan_in_bwd_parts (raw-x sums
    in 1, 4 and 96 partials, sums against relu(xhat)), gan_bias_finalize_batch with two descriptors;
    fold: gan_fold_add, gan_pad_fold (reflect, replicate), gan_act_bwd (four activations)."""
    N.body(make, group, p[0], p[1])


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("shape", N.LIMIT_SHAPES)
def test_known_limit_of_the_statistics(shape, dtype):
    """mean / sigma = 1000 / 1 and 30 / 0.1: rstd finite, in (0, eps^-1/2], inside the interval of the conditioning contract; the error
    is printed beside torch float32 instance_norm's"""
    N.body_limit(make, shape, dtype)


def test_unsupported_widths_return_their_error():
    N.body_unsupported(make)


@pytest.mark.parametrize("group,wrong", [(g, w) for g, ws in N.WRONG.items() for w in ws], ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_family_rejects_a_wrong_reference(group, wrong):
    """The kernels' results held to a deliberately wrong reference: every group's assertions fail.  The kernels are never made to misbehave."""
    N.rejects(make, group, wrong)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_nan_plane(dtype):
    """a NaN in x reaches its whole (image, channel) plane of y through every activation -- ReLU included -- and no other plane"""
    assert N.body_nan_plane(make, dtype) == 16
