"""The operator library torch.ops.mi355x_gan.* op by op without a GPU: every case of tests/oplib_cases.py on the emulator (through
autograd._OPS_FACTORY) against float64 inside the project's derived bounds, every deliberately wrong reference outside them, the schemas
under torch.library.opcheck, and the trainers at an image size whose discriminator maps are odd.  tests/test_oplib_family_gpu.py runs the
same bodies on the HIP kernels."""
import pytest
import torch

from gan_variant_research_amd import BF16, F32  # noqa: F401
from gan_variant_research_amd import autograd as AG
from gan_variant_research_amd import losses as LS
from gan_variant_research_amd import ops_library as L
from gan_variant_research_amd import training as T
from gan_variant_research_amd._lib import GanError
from tests import cases
from tests import oplib_cases as O
from tests.emulator import EmuOps
from tests.emulator_palette import PaletteEmuOps

DEV = "cpu"


@pytest.fixture(autouse=True)
def recording(monkeypatch):
    rec = O.Recording(lambda device: PaletteEmuOps())
    monkeypatch.setattr(AG, "_OPS_FACTORY", rec)
    monkeypatch.setattr(L, "_PLANS", {})
    monkeypatch.setattr(LS, "_PLANS", {})
    monkeypatch.setattr(T, "_FUSED_PLANS", {})
    return rec


def reset_of(rec):
    def reset():
        L._PLANS.clear()
        rec.made.clear()
    return reset


@pytest.mark.parametrize("S", O.CONVS, ids=O.conv_id)
def test_emulated_convolution_op_within_the_derived_bounds(S, recording):
    """conv2d_fwd / conv_transpose2d_fwd and their autograd formulas: y, the activation's backward, dx, dw and db against float64"""
    O.body_conv(DEV, S, recording)


@pytest.mark.parametrize("p", O.NORMS, ids=O.norm_id)
def test_emulated_instance_norm_op_within_the_derived_bounds(p):
    """instance_norm_fwd / _bwd: the returned statistics, y and dx; d(residual) bit for bit; one pixel gives exactly 0 (+ residual)"""
    O.body_norm(DEV, *p)


def test_emulated_act_bwd_is_the_headers_statement():
    O.body_act_bwd(DEV)


def test_emulated_pads_are_exact():
    O.body_pads(DEV)


@pytest.mark.parametrize("momentum", [0.1, None])
def test_emulated_batchnorm_module_equals_float64_torch(momentum):
    O.body_batchnorm(DEV, momentum)


def test_emulated_autograd_plumbing():
    """gradient subsets, inputs that are not contiguous float32, two layers sharing one plan in one graph: all bit for bit"""
    O.body_plumbing(DEV)


@pytest.mark.parametrize("wrong", O.WRONG, ids=lambda w: w.__name__)
def test_emulated_family_rejects_a_wrong_reference(wrong, recording):
    O.rejects(DEV, wrong, reset_of(recording))


def test_emulated_family_worst_ratios(recording):
    """worst error / bound per group and dtype; a group below 0.01 of its bound fails: that bound would catch nothing"""
    O.summary(DEV, reset_of(recording))


# ---------------------------------------------------------------------------------------------- registration
@pytest.mark.parametrize("i", range(len(O.opcheck_args())), ids=lambda i: O.opcheck_args()[i][0])
def test_schemas_hold_under_opcheck(i):
    """torch.library.opcheck on the emulator: the schema (a write to an argument it calls read-only fails) and, for the functional ops,
    the autograd registration.  No fake implementation is registered, so the fake-tensor and AOT utilities are not run."""
    name, args, utils = O.opcheck_args()[i]
    torch.library.opcheck(getattr(torch.ops.mi355x_gan, name).default, args, test_utils=utils)


# ---------------------------------------------------------------------------------------------- refusals, on the host
def test_a_strided_input_gradient_that_cannot_be_planned_is_refused_when_the_plan_is_built():
    from gan_variant_research_amd.convplan import ConvLayer
    from gan_variant_research_amd.runtime import Ctx, cpad
    ctx = Ctx(EmuOps(), "cpu", F32)
    w = torch.zeros(8, 8, 3, 3)
    layer = ConvLayer(ctx, w, None, torch.zeros_like(w), None, 3, 2, 1)
    with pytest.raises(GanError, match=r"B2 7x13 k3 s2 p1"):           # a dy that is not the forward output of the map
        layer.dgrad(ctx.view(2, 3, 7, 8, 1), ctx.view(2, 7, 13, 8, 0))
    with pytest.raises(GanError, match=r"B2 7x13 k3 s2 p1"):           # no padded-domain gradient for a strided layer
        layer.dgrad(ctx.view(2, 4, 7, 8, 1), ctx.view(2, 7, 13, 8, 1), padded_domain=True)
    w5 = torch.zeros(8, 8, 5, 5)
    layer5 = ConvLayer(ctx, w5, None, torch.zeros_like(w5), None, 5, 2, 2)
    with pytest.raises(GanError, match=r"B1 9x9 k5 s2 p2.*halo 0"):     # a halo the taps outrun
        layer5.dgrad(ctx.view(1, 5, 5, 8, 0), ctx.view(1, 9, 9, 8, 0))
    assert len(layer.dgrad(ctx.view(2, 4, 7, 8, 1), ctx.view(2, 7, 13, 8, 0))) == 4
    assert len(layer.dgrad(ctx.view(2, 1, 1, 8, 1), ctx.view(2, 1, 1, 8, 0))) == 1      # one pixel: phase (0, 0) alone


# ---------------------------------------------------------------------------------------------- the trainers on odd discriminator maps
def test_emulated_cut_step_at_36():
    """36 -> 18 -> 9: the PatchGAN's third 4x4 stride-2 layer sees a 9x9 map; fp32 mode against the oracle at run_cut_steps' own tolerances"""
    tr, img, ref_img = cases.run_cut_steps("cpu", EmuOps(), False, S=36, B=1, nsteps=1)
    torch.testing.assert_close(img, ref_img, rtol=2e-4, atol=2e-4)


def test_emulated_cyclegan_iteration_at_36():
    cases.run_basic_iterations("cpu", EmuOps(), S=36, B=1, niter=1)
