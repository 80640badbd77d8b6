"""The e4m3 operand producers without a GPU: tests/e4m3_ref.py (an e4m3 statement from the format definition) against itself and against
torch's own cast -- which licenses the emulators' use of that cast -- and the emulator's statements of the producers run through the
very assertions tests/test_fp8_producers_gpu.py holds the HIP kernels to (tests/fp8_producer_cases.py), at the same shapes."""
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd.runtime import Ctx
from tests import e4m3_ref as R
from tests import fp8_producer_cases as P
from tests.emulator_basic_fp8 import BasicFp8EmuOps


def make():
    return Ctx(BasicFp8EmuOps(), "cpu", BF16)


# ---------------------------------------------------------------------------------------------- the reference itself
def test_decode_table_is_the_format_definition():
    assert float(R.DECODE[0x7E]) == 448.0 and float(R.DECODE[0x01]) == 2.0 ** -9 and float(R.DECODE[0x08]) == 2.0 ** -6
    assert float(R.DECODE[0x38]) == 1.0 and float(R.DECODE[0xB8]) == -1.0 and float(R.DECODE[0x3C]) == 1.5
    assert bool(torch.isnan(R.DECODE[[0x7F, 0xFF]]).all()) and int(torch.isnan(R.DECODE).sum()) == 2
    assert R.MAGS.numel() == 127 and R.MIDS.numel() == 126


def test_encode_round_trips_every_finite_code():
    codes = torch.tensor([c for c in range(256) if c not in R.NAN_CODES], dtype=torch.uint8)
    assert torch.equal(R.encode(R.decode(codes)), codes)                       # -0 (0x80) included
    assert bool(R.is_nan_code(R.encode(torch.tensor([float("nan")], dtype=torch.float64))).all())


def test_encode_ties_to_even_and_neighbours_to_their_side():
    lo, hi = torch.arange(126), torch.arange(1, 127)
    even = torch.where(lo % 2 == 0, lo, hi).to(torch.uint8)
    below, above = torch.nextafter(R.MIDS, torch.zeros_like(R.MIDS)), torch.nextafter(R.MIDS, torch.full_like(R.MIDS, 1e9))
    for sign, bit in ((1.0, 0), (-1.0, 128)):
        assert torch.equal(R.encode(sign * R.MIDS), even + bit)
        assert torch.equal(R.encode(sign * below), lo.to(torch.uint8) + bit)
        assert torch.equal(R.encode(sign * above), hi.to(torch.uint8) + bit)
    assert torch.equal(R.encode_truncate(R.MIDS), lo.to(torch.uint8)) and torch.equal(R.encode_truncate(above), lo.to(torch.uint8))


def test_encode_clamps_and_keeps_the_sign_of_zero():
    x = torch.tensor([float("inf"), -float("inf"), 1e30, -1e30, 448.0, 464.0, 0.0, -0.0], dtype=torch.float64)
    assert R.encode(x).tolist() == [0x7E, 0xFE, 0x7E, 0xFE, 0x7E, 0x7E, 0x00, 0x80]


def test_near_midpoint_names_the_two_neighbours():
    x = torch.tensor([1.0625, -1.0625 * (1 + 2.0 ** -23), 1.0625 * (1 + 2.0 ** -20), 1.0, 0.0], dtype=torch.float64)
    m, lo, hi = R.near_midpoint(x, 2.0 ** -22)
    assert m.tolist() == [True, True, False, False, False]
    assert (int(lo[0]), int(hi[0]), int(lo[1]), int(hi[1])) == (0x38, 0x39, 0xB8, 0xB9)
    m, lo, hi = R.near_midpoint_abs(torch.tensor([1e-7, -1e-7, 1e-3], dtype=torch.float64), torch.full((3,), 1e-6, dtype=torch.float64))
    assert m.tolist() == [True, True, False] and (int(lo[0]), int(hi[0])) == (0x00, 0x80)


# ---------------------------------------------------------------------------------------------- agreement with torch's cast
def torch_bytes(x):
    return x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def test_encode_equals_torchs_cast_on_every_finite_bf16():
    x = P.bf16_patterns()
    x = x[torch.isfinite(x.float())]
    assert x.numel() == 65280
    assert torch.equal(R.encode(x.double()), torch_bytes(x)) and torch.equal(R.encode(x.double()), torch_bytes(x.float()))
    nan = torch.tensor([float("nan")])
    assert bool(R.is_nan_code(torch_bytes(nan)).all()) and bool(R.is_nan_code(torch_bytes(nan.bfloat16())).all())       # clamp keeps NaN, the cast too


def test_encode_equals_torchs_cast_on_random_fp32():
    g = torch.Generator().manual_seed(2)
    x = torch.exp(torch.rand(4_000_000, generator=g) * (torch.log(torch.tensor(1e3)) - torch.log(torch.tensor(1e-4))) + torch.log(torch.tensor(1e-4)))
    x = x * (torch.randint(0, 2, x.shape, generator=g) * 2.0 - 1.0)
    assert torch.equal(R.encode(x.double()), torch_bytes(x))
    assert torch.equal(R.encode(P.fp32_set().double()), torch_bytes(P.fp32_set()))


# ---------------------------------------------------------------------------------------------- the emulator's statements
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_emulated_unit_quantiser(dtype):
    P.body_unit(make, dtype)


def test_emulated_unit_quantiser_grid_stride_shape():
    P.body_unit_grid(make)


@pytest.mark.parametrize("shape", P.AMAX_SHAPES)
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_emulated_amax_quantiser(dtype, shape):
    P.body_amax(make, dtype, shape)


@pytest.mark.parametrize("shape", P.AMAX_SHAPES)
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_amax_data_alone_stays_under_the_midpoint_cap(dtype, shape):
    """The seeds are chosen so that the REFERENCE has few elements within 2^-22 of a midpoint: the cap cannot be met by the data alone."""
    vals, _ = P.amax_data(dtype, shape)
    v = vals.double()
    sc = (v.abs().amax((1, 2, 3)) / 448.0).float().double().clamp_min(2.0 ** -126)
    open_ = [b for b in range(P.AMAX_B) if b not in P.POW2_IMAGES + (P.ZERO_IMAGE, P.TINY_IMAGE)]
    m, _, _ = R.near_midpoint(v[open_] / sc[open_].view(-1, 1, 1, 1), P.REL)
    share = float(m.float().mean())
    print(f"[fp8-producers] amax data {P.NAME[dtype]} {shape}: near-midpoint share of the reference alone {share:.2e}")
    assert share <= P.CAP / 2


@pytest.mark.parametrize("shape", P.NORM_SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_emulated_apply_parts_fp8(dtype, shape):
    P.body_apply(make, dtype, shape)


def test_normal_data_near_midpoints_at_the_expected_delta():
    """The share of N(0,1) values within 1e-5 (1 + |v|) of a midpoint, the figure the 0.5 % cap of the bf16 y8 comparison rests on."""
    v = torch.randn(4_000_000, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    m, _, _ = R.near_midpoint_abs(v, 1e-5 * (1 + v.abs()))
    share = float(m.float().mean())
    print(f"[fp8-producers] N(0,1) within 1e-5 (1 + |v|) of a midpoint or of zero: {share:.3e}")
    assert share <= P.AMB_CAP_NORM / 2


@pytest.mark.parametrize("shape", P.NORM_SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_emulated_in_bwd_amax(dtype, shape):
    P.body_bwd(make, dtype, shape)


def test_emulated_weight_scale_and_fp8_pack():
    P.body_weights(make)


def test_emulated_tiny_weight_gets_the_scale_floor():
    P.body_tiny_weight(make)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_emulated_pow2_quantiser_against_the_independent_encoder(dtype):
    P.body_pow2(make, dtype)


@pytest.mark.parametrize("producer", ["unit-bf16", "unit-fp32", "amax-bf16", "amax-fp32", "y8-bf16", "y8-fp32", "pack"])
def test_emulated_nan_becomes_a_nan_byte(producer):
    P.body_nan(make, producer)


# ---------------------------------------------------------------------------------------------- the assertions bite
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("group,wrong", [(g, w) for g, ws in P.WRONG.items() for w in ws])
def test_emulated_producers_reject_a_wrong_reference(group, wrong, dtype):
    """Held to a deliberately wrong reference -- truncation instead of round-to-nearest-even, the scale of image b + 1, a halo left
    unconverted, amax over the padded domain, amax not reset -- each group's assertions fail."""
    P.rejects(make, group, wrong, dtype)
