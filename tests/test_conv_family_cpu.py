"""The convolution launches behind gan_conv_igemm without a GPU: tests/cases.conv_ref64 against float64 F.conv2d / F.conv_transpose2d /
autograd on non-square maps, the emulator's statement of every case of tests/conv_cases.py inside the derived bounds of
tests/conv_ref64.py (which therefore admit an honest implementation), every deliberately wrong reference outside them, the planner
predicates of the emulator against the library's, the refused descriptors, and the weight pack.
tests/test_conv_family_gpu.py runs the same bodies on the HIP kernels."""
import pytest
import torch
import torch.nn.functional as F

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd.runtime import Ctx, HipOps
from tests import conv_cases as C
from tests import conv_ref64 as R
from tests.cases import conv_ref64
from tests.emulator import EmuOps

TOL = dict(rtol=1e-12, atol=1e-12)


def make(dtype):
    return Ctx(EmuOps(), "cpu", dtype)


# ---------------------------------------------------------------------------------------------- the reference against float64 torch
@pytest.mark.parametrize("g", [(5, 7, 3, 1, 1, False, 6, 11, True), (4, 6, 4, 2, 1, False, 6, 10, False), (6, 5, 3, 2, 1, True, 3, 7, False),
                               (3, 4, 7, 1, 3, False, 9, 5, True), (4, 6, 4, 2, 1, False, 7, 9, False), (4, 6, 3, 2, 1, False, 7, 13, False)], ids=str)
def test_reference_equals_float64_torch_on_non_square_maps(g):
    cin, cout, k, s, p, tr, H, W, reflect = g
    gen = torch.Generator().manual_seed(3)
    w = torch.randn((cin, cout, k, k) if tr else (cout, cin, k, k), generator=gen, dtype=torch.float64).requires_grad_(True)
    x = torch.randn(2, cin, H, W, generator=gen, dtype=torch.float64).requires_grad_(True)
    if tr:
        y = F.conv_transpose2d(x, w, None, stride=2, padding=1, output_padding=1)
    else:
        xp = F.pad(x, (p, p, p, p), mode="reflect" if reflect else "constant")
        xp.retain_grad()
        y = F.conv2d(xp, w, None, stride=s)
    gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(gy)
    wd, xd = w.detach(), x.detach()
    torch.testing.assert_close(conv_ref64("fwd", k, s, p, tr, reflect, wd, x=xd)[0], y.detach(), **TOL)
    torch.testing.assert_close(conv_ref64("wgrad", k, s, p, tr, reflect, wd, x=xd, dy=gy)[0], w.grad, **TOL)
    if tr:
        torch.testing.assert_close(conv_ref64("dgrad", k, s, p, tr, reflect, wd, dy=gy, x_hw=(H, W))[0], x.grad, **TOL)
    else:      # the gradient on the padded domain is the gradient of the explicitly padded input; its interior is the zero-padded layer's
        torch.testing.assert_close(conv_ref64("dgrad", k, s, p, tr, reflect, wd, dy=gy, x_hw=(H, W), padded_domain=True)[0], xp.grad, **TOL)
        if not reflect:
            torch.testing.assert_close(conv_ref64("dgrad", k, s, p, tr, reflect, wd, dy=gy, x_hw=(H, W))[0], x.grad, **TOL)


def test_epilogue_statement_equals_torch():
    t = torch.randn(1000, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    t[:3] = torch.tensor([0.0, -0.0, float("nan")], dtype=torch.float64)
    for act, fn in ((R.ACT_RELU, torch.relu), (R.ACT_LRELU, lambda v: F.leaky_relu(v, 0.2)), (R.ACT_TANH, torch.tanh), (R.ACT_NONE, lambda v: v)):
        torch.testing.assert_close(R.act64(t, act), fn(t), equal_nan=True, **TOL)
    v = t.clone().requires_grad_(True)
    F.leaky_relu(v[3:], 0.2).sum().backward()
    torch.testing.assert_close(R.mask_factor64(F.leaky_relu(t[3:], 0.2)), v.grad[3:], **TOL)          # LeakyReLU' from the saved output
    assert R.mask_factor64(torch.tensor([0.0, -0.0, 1e-30, -1e-30], dtype=torch.float64)).tolist() == [0.2, 0.2, 1.0, 0.2]


# ---------------------------------------------------------------------------------------------- the emulator inside the bounds
@pytest.mark.parametrize("S", C.GEOMETRY + C.EPILOGUE, ids=C.spec_id)
def test_emulated_case_within_the_derived_bounds(S):
    """one planned request: its key (the kernel and branch it names), sentinels, bit-unchanged inputs, repeat, pad channels
    (tests/conv_cases.run), then elements, partials and chain sums against the float64 statement"""
    C.check(make, "geometry" if S in C.GEOMETRY else "epilogue", S)


@pytest.mark.parametrize("group", list(C.GROUPS))
def test_emulated_family_within_the_derived_bounds(group):
    """the worst error / bound per kernel variant of the group; a variant without a figure fails (a case that misses fails in its own test)"""
    C.summary(make, group)


@pytest.mark.parametrize("S", C.NONFINITE, ids=C.spec_id)
def test_emulated_nonfinite_contract(S):
    """One NaN, then one +Inf, in a real channel of one pixel near the top of image 1 of 3.  Images 0 and 2 and their partials are
    bit-identical to the clean run; every real element of image 1 whose float64 reference is not finite is not finite, a NaN a NaN,
    through every activation and the mask; every other real element is within the bound, except the widened footprint of a paired launch.
    A +Inf behind ReLU or tanh is the sharp case: relu(-Inf) = 0 and tanh(-Inf) = -1 are finite in the reference, so a kernel that multiplies
    the poisoned pixel by the zero weights of a padded tap (0 x Inf = NaN) fails here; the generic kernel reads zeros for padded taps."""
    C.check(make, "nonfinite", S)


def test_emulated_paired_phase_footprint():
    """the paired launch of the 128 -> 64 transposed forward on a 6x10 input: one NaN pixel reaches 9 output pixels in the reference and
    3 more through the zero weights of the other x-phase; the unpaired 256 -> 128 layer none"""
    C.summary(make, "nonfinite")
    exc = {k[1]: n for k, n in C._excused.items() if k[0] == "cpu"}
    assert exc["128-64k3s2Tz-6x10-B3-bf16-fwd-nan"] == 3 and exc["256-128k3s2Tz-6x10-B3-bf16-fwd-nan"] == 0
    assert all(n == 0 for what, n in exc.items() if not what.startswith("128-64k3s2T")), exc


@pytest.mark.parametrize("S", [s for s in C.EPILOGUE if s.B == 3 and not s.env], ids=C.spec_id)
def test_emulated_image_0_does_not_depend_on_the_batch(S):
    C.check_batch_invariance(make, S)


def test_emulated_tile_width_does_not_enter_the_result():
    by = {(s.op, dict(s.env).get("GAN_PATCH_BN")): s for s in C.EPILOGUE if s.g == C.Geom(*C.E_WIDE) and s.env}
    for op in ("fwd", "dgrad"):
        C.check_tile_width_invariance(make, by[(op, "128")], by[(op, "256")])


# ---------------------------------------------------------------------------------------------- the assertions bite
@pytest.mark.parametrize("wrong", C.WRONG, ids=lambda w: w.__name__)
def test_emulated_family_rejects_a_wrong_reference(wrong):
    C.rejects(make, wrong)


# ---------------------------------------------------------------------------------------------- host side of the library
@pytest.mark.parametrize("group", list(C.GROUPS))
def test_planner_predicates_of_emulator_and_library_agree(group):
    hip = HipOps(torch.device("cpu"))          # the predicates are pure host functions
    for S in C.GROUPS[group]:
        C.check_predicates(hip, S)


@pytest.mark.parametrize("S", C.GEOMETRY + C.EPILOGUE + C.NONFINITE, ids=C.spec_id)
def test_library_plans_the_branch_the_case_names(S):
    C.check_plan(HipOps(torch.device("cpu")), S)


def test_one_pixel_wide_and_4gib_maps_are_refused_by_both_predicates():
    """the two rules the emulator's statement lacked: Wo < 2 (a 37x1 map with Cin 64) and operand tensors past 4 GiB"""
    hip, emu = HipOps(torch.device("cpu")), EmuOps()
    _, (c,) = C.plan_only(emu, C.Spec((64, 128, 3, 1, 1, False, 37, 1, False), 1, BF16, "fwd", "generic"))
    assert not emu.conv_patch_ok(c) and not hip.conv_patch_ok(c) and not c.w_frag
    _, (c,) = C.plan_only(emu, C.Spec((64, 128, 3, 1, 1, False, 6, 11, True), 1, BF16, "fwd", "patch"))
    assert emu.conv_patch_ok(c) and hip.conv_patch_ok(c)
    c.B = 600000                                   # 600,000 x 8 x 13 x 64 x 2 bytes > 4 GiB (planning only: nothing is allocated)
    assert not emu.conv_patch_ok(c) and not hip.conv_patch_ok(c)


def test_refused_descriptors_return_their_error():
    assert C.body_refused(HipOps(torch.device("cpu")), "cpu") >= 8


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_emulated_weight_pack_is_the_float64_statement(dtype):
    assert C.body_pack(make, dtype) == 0
