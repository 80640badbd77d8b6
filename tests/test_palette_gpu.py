"""Palette prior on the GPU: the bodies of tests/palette_cases.py on HipOps (tests/test_palette_cpu.py runs them on the emulator) -- the
kernels of csrc/palette.hip at their edge shapes against the float64 statement, the edge semantics, losses.PalettePriorLoss and
cut.CutTrainer with loss_weights.palette."""
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd.runtime import HipOps
from tests import palette_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_ops():
    return HipOps(torch.device(DEV))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "B%d_%dx%d_T%d" % s)
def test_family_against_float64(shape, dtype):
    P.body_family(make_ops(), DEV, shape, dtype)


@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "B%d_%dx%d_T%d" % s)
def test_family_with_nan_in_halo_and_pad_channels(shape):
    P.body_family(make_ops(), DEV, shape, BF16, halo=3, nan=True)


def test_saturated_pixels():
    P.body_saturation(make_ops(), DEV)


def test_constant_image():
    P.body_constant(make_ops(), DEV)


def test_nan_pixel_poisons_its_own_image_only():
    P.body_nan_pixel(make_ops(), DEV)


def test_one_cell_is_refused():
    P.body_t1_raises(make_ops(), DEV)


def test_batch_mean_and_prior_update():
    P.body_prior_update(make_ops(), DEV)


def test_module_path():
    P.body_module(DEV)


@pytest.mark.parametrize("merged,nce", [(True, True), (True, False), (False, True), (False, False)], ids=["merged-fold", "merged-plain", "separate-fold", "separate-plain"])
def test_trainer_term_in_every_shape_of_the_step(merged, nce):
    P.body_trainer_term(make_ops, DEV, merged, nce)


def test_trainer_gradient_is_affine_in_the_weight():
    P.body_linearity(make_ops, DEV)


def test_weight_zero_builds_todays_programs():
    P.body_weight_zero(make_ops, DEV)


def test_saturated_generator_does_not_raise_the_nan_stop():
    P.body_saturated_generator(make_ops, DEV)


def test_checkpoint_carries_the_prior_and_resumes_bit_for_bit(tmp_path):
    P.body_checkpoint(make_ops, DEV, tmp_path)
