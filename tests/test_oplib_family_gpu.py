"""The operator library torch.ops.mi355x_gan.* op by op on the HIP kernels: the cases, float64 references and derived bounds of
tests/oplib_cases.py (tests/test_oplib_family_cpu.py runs the same bodies on the emulator and shows that the bounds admit it and reject
the listed mistakes).  Each op plans its own launches at shapes the fused trainers never use: odd and non-square maps, B = 1, Cout = 1,
channel counts that are no multiple of 8, the epilogue activations and their backward chain, bias=None, both compute dtypes; the BF16
cases assert from the recorded launches that they reached the kernel they name."""
import pytest
import torch

from gan_variant_research_amd import autograd as AG
from gan_variant_research_amd import ops_library as L
from gan_variant_research_amd.runtime import HipOps
from tests import oplib_cases as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def recording(monkeypatch):
    rec = O.Recording(lambda device: HipOps(device))
    monkeypatch.setattr(AG, "_OPS_FACTORY", rec)
    monkeypatch.setattr(L, "_PLANS", {})
    return rec


def reset_of(rec):
    def reset():
        L._PLANS.clear()
        rec.made.clear()
    return reset


@pytest.mark.parametrize("S", O.CONVS, ids=O.conv_id)
def test_convolution_op_within_the_derived_bounds(S, recording):
    """conv2d_fwd / conv_transpose2d_fwd and their autograd formulas: y, the activation's backward, dx, dw and db against float64"""
    O.body_conv(DEV, S, recording)


@pytest.mark.parametrize("p", O.NORMS, ids=O.norm_id)
def test_instance_norm_op_within_the_derived_bounds(p):
    """instance_norm_fwd / _bwd: the returned statistics, y and dx; d(residual) bit for bit; one pixel gives exactly 0 (+ residual)"""
    O.body_norm(DEV, *p)


def test_act_bwd_is_the_headers_statement():
    O.body_act_bwd(DEV)


def test_pads_are_exact():
    O.body_pads(DEV)


@pytest.mark.parametrize("momentum", [0.1, None])
def test_batchnorm_module_equals_float64_torch(momentum):
    O.body_batchnorm(DEV, momentum)


def test_autograd_plumbing():
    """gradient subsets, inputs that are not contiguous float32, two layers sharing one plan in one graph: all bit for bit"""
    O.body_plumbing(DEV)


@pytest.mark.parametrize("wrong", O.WRONG, ids=lambda w: w.__name__)
def test_family_rejects_a_wrong_reference(wrong, recording):
    """The kernels' results held to a deliberately wrong reference: the assertions fail.  The kernels are never made to misbehave."""
    O.rejects(DEV, wrong, reset_of(recording))


def test_family_worst_ratios(recording):
    """worst error / bound per group and dtype; a group below 0.01 of its bound fails: that bound would catch nothing"""
    O.summary(DEV, reset_of(recording))
