"""The convolution launches behind gan_conv_igemm (csrc/conv_igemm.hip, conv_patch.hip, conv_win7.hip) on the GPU through HipOps, element
by element against the float64 statements of tests/conv_ref64.py with the derived bounds there (tests/test_conv_family_cpu.py runs the
same bodies on the emulator and shows that the bounds admit it and reject the listed mistakes).

What the cases reach that the square twins of tests/test_gpu_parity.py do not: H != W on every kernel, B = 1 / 3 / 20, maps smaller than
a tile, Ho * Wo = 128 / 129, the persistent walk with skipped virtual tiles, the 256-row Nw = 16 tile, 7- and 9-slice buffers, 256- and
288-row and 128- and 256-column tiles, every static tap schedule and the generic tap loop, M_img around a tile, Wo = 2 and Wo = 1, both
paired-phase launches, the input gradient of stride-2 layers on odd maps (phases of different extents, never paired), both window
kernels in both directions; every activation with and without bias, cout 1 / 3 / 20, the LeakyReLU'
mask with zeros and -0.0 through halo 0 and 1, fused partials and chain sums, and one NaN / +Inf.  Each case asserts from the library's
own plan that it reached the kernel and branch it names."""
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd.runtime import Ctx, HipOps
from tests import conv_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make(dtype):
    return Ctx(HipOps(torch.device(DEV)), DEV, dtype)


@pytest.mark.parametrize("S", C.GEOMETRY + C.EPILOGUE, ids=C.spec_id)
def test_case_within_the_derived_bounds(S):
    """one planned request: its key (the kernel and branch it names), sentinels, bit-unchanged inputs, repeat, pad channels
    (tests/conv_cases.run), then elements, partials and chain sums against the float64 statement"""
    C.check(make, "geometry" if S in C.GEOMETRY else "epilogue", S)


@pytest.mark.parametrize("group", list(C.GROUPS))
def test_family_within_the_derived_bounds(group):
    """the worst error / bound per kernel variant of the group; a variant without a figure fails (a case that misses fails in its own test)"""
    C.summary(make, group)


@pytest.mark.parametrize("S", C.NONFINITE, ids=C.spec_id)
def test_nonfinite_contract(S):
    """One NaN, then one +Inf, in a real channel of one pixel near the top of image 1 of 3.  Images 0 and 2 and their partials are
    bit-identical to the clean run; every real element of image 1 whose float64 reference is not finite is not finite, a NaN a NaN,
    through every activation and the mask; every other real element is within the bound, except the widened footprint of a paired launch.
    A +Inf behind ReLU or tanh is the sharp case: relu(-Inf) = 0 and tanh(-Inf) = -1 are finite in the reference, so a kernel that multiplies
    the poisoned pixel by the zero weights of a padded tap (0 x Inf = NaN) fails here; the generic kernel reads zeros for padded taps."""
    C.check(make, "nonfinite", S)


def test_paired_phase_footprint():
    """the excused set is empty on every unpaired launch and 3 pixels on the paired 128 -> 64 transposed forward"""
    C.summary(make, "nonfinite")
    exc = {k[1]: n for k, n in C._excused.items() if k[0] == "cuda"}
    assert exc["128-64k3s2Tz-6x10-B3-bf16-fwd-nan"] == 3
    assert all(n == 0 for what, n in exc.items() if not what.startswith("128-64k3s2T")), exc


@pytest.mark.parametrize("S", [s for s in C.EPILOGUE if s.B == 3 and not s.env], ids=C.spec_id)
def test_image_0_does_not_depend_on_the_batch(S):
    C.check_batch_invariance(make, S)


def test_tile_width_does_not_enter_the_result():
    """128- against 256-channel tiles: result, fused partials and chain sums bit-identical (csrc/conv_patch.hip)"""
    by = {(s.op, dict(s.env).get("GAN_PATCH_BN")): s for s in C.EPILOGUE if s.g == C.Geom(*C.E_WIDE) and s.env}
    for op in ("fwd", "dgrad"):
        C.check_tile_width_invariance(make, by[(op, "128")], by[(op, "256")])


@pytest.mark.parametrize("wrong", C.WRONG, ids=lambda w: w.__name__)
def test_family_rejects_a_wrong_reference(wrong):
    """The kernels' results held to a deliberately wrong reference: the assertions fail.  The kernels are never made to misbehave."""
    C.rejects(make, wrong)


def test_refused_descriptors_return_their_error_and_leave_the_sentinel():
    assert C.body_refused(HipOps(torch.device(DEV)), DEV) >= 8


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_weight_pack_is_the_float64_statement(dtype):
    assert C.body_pack(make, dtype) == 0
