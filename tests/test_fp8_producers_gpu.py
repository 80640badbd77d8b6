"""The kernels that MAKE the e4m3 operands and their scales, on the GPU through HipOps, byte for byte against a float64 statement:
gan_quantize_fp8 (unit scale and per-image amax), gan_quantize_fp8_pow2, the y8 store of gan_in_apply_parts_fp8, gan_in_bwd_amax,
gan_weight_scale_batch and the GAN_FP8 branch of gan_pack_weight_batch.  The cases, the byte contract and the assertions are in
tests/fp8_producer_cases.py (tests/test_fp8_producers_cpu.py runs the same ones on the emulator's statements); the encoder is
tests/e4m3_ref.py, which uses no torch.float8_e4m3fn.

Decisions these tests encode (include/mi355x_gan.h states them):
  * a NaN source element yields an e4m3 NaN byte from every producer, +-inf and everything beyond +-448 yield +-448;
  * gan_quantize_fp8 never writes a per-image scale below 2^-126: an image whose amax is below 448 * 2^-126 gets finite bytes;
  * gan_in_bwd_amax reports max|dx| over the interior BEFORE the store rounds dx to its dtype, and overwrites amax on every call.
"""
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd.runtime import Ctx, HipOps
from tests import fp8_producer_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make():
    return Ctx(HipOps(torch.device(DEV)), DEV, BF16)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_unit_quantiser_every_pattern(dtype):
    """bf16: all 65 536 bit patterns in a (1, 62, 62, 16) halo-1 view, halo converted too; fp32: the same values plus every midpoint
    between two codes and its two fp32 neighbours.  Finite patterns byte-exact, +-inf -> +-448."""
    P.body_unit(make, dtype)


def test_unit_quantiser_grid_stride():
    """2 359 296 sixteen-element chunks, more than 8192 blocks of 256 threads: the only case in which a thread converts two chunks.
    The reference is computed on the device."""
    P.body_unit_grid(make)


@pytest.mark.parametrize("shape", P.AMAX_SHAPES)
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_amax_quantiser(dtype, shape):
    """Eight images more than 2x apart in magnitude (1.75 * 2^k twice: exact power-of-two scale and frequent ties; 0.013; 448; 6e4; 0;
    2^-20; one below 448 * 2^-126): the scale within one ulp of amax / 448, every image's bytes on ITS scale, +-amax -> +-448, floats
    past B untouched."""
    P.body_amax(make, dtype, shape)


@pytest.mark.parametrize("shape", P.NORM_SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_apply_parts_fp8(dtype, shape):
    """activation {none, relu} x residual x halo {reflect, none}: y and stats bit-identical to gan_in_apply_parts, halo bytes equal to the
    bytes at their reflect pre-images (or untouched), y8 = encode(y) exactly in fp32 and encode(float64 InstanceNorm) in bf16 up to the
    measured margin, and y8 within one e4m3 spacing of y."""
    P.body_apply(make, dtype, shape)


@pytest.mark.parametrize("shape", P.NORM_SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_in_bwd_amax(dtype, shape):
    """activation {relu, none} x bias_part {given, NULL}, fold where the map allows it: dx and bias_part bit-identical to the op without
    amax, amax = max|dx| over the interior (exact in fp32, before the rounding in bf16), the 1e6 halo neither written nor counted, a
    second call on a gradient 2^-6 as large gives 2^-6 the amax, and the chained quantiser's bytes peak at 448 without a NaN."""
    P.body_bwd(make, dtype, shape)


def test_weight_scale_and_fp8_pack():
    """One batch of four descriptors (256x256x3x3; 128x256x3x3 swapped; all zero; 100x60x3x3 with rows, channels and a tap padded and its
    largest element negative and last): scale within one ulp of max|W| / 448, bytes on the GPU's own scale, padding zero."""
    P.body_weights(make)


def test_tiny_weight_gets_the_scale_floor():
    """max|W| = 2^-135: the scale is 2^-126 like gan_quantize_fp8's, not a subnormal whose reciprocal is infinite"""
    P.body_tiny_weight(make)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_pow2_quantiser_against_the_independent_encoder(dtype):
    """test_basic_fp8_gpu.test_pow2_quantiser_equals_its_emulator_statement's inputs against e4m3_ref.encode: exact, no exceptions"""
    P.body_pow2(make, dtype)


@pytest.mark.parametrize("producer", ["unit-bf16", "unit-fp32", "amax-bf16", "amax-fp32", "y8-bf16", "y8-fp32", "pack"])
def test_nan_becomes_a_nan_byte(producer):
    P.body_nan(make, producer)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("group,wrong", [(g, w) for g, ws in P.WRONG.items() for w in ws])
def test_producers_reject_a_wrong_reference(group, wrong, dtype):
    """The kernels' results held to a deliberately wrong reference (truncation, the scale of image b + 1, a halo left unconverted, amax
    over the padded domain, amax not reset): every group's assertions fail.  The kernels are never made to misbehave."""
    P.rejects(make, group, wrong, dtype)
