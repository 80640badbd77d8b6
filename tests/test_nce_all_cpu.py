"""PatchNCE with negatives from the whole minibatch (gan_patchnce_all_*) without a GPU: the float64 statement of tests/nce_all_ref64.py
against float64 autograd, the regimes the cases of tests/nce_all_cases.py name, the conditions the bounds rest on (asserted by the case
builder for every run), the emulator's fp32 statement inside the derived bounds (loss and gtgt) -- which therefore admit an honest fp32
implementation -- the equivalence with the per-image entry points at B = 1, the refused arguments, and every deliberately wrong reference
outside the bounds.  tests/test_nce_all_gpu.py runs the same bodies on the HIP kernels."""
import pytest
import torch

from gan_variant_research_amd import BF16
from gan_variant_research_amd.runtime import Ctx
from tests import nce_all_cases as N
from tests import nce_all_ref64 as R
from tests.emulator_nce_all import NceAllEmuOps

TOL = dict(rtol=1e-12, atol=1e-12)


def make():
    return Ctx(NceAllEmuOps(), "cpu", BF16)


AUTOGRAD_RUNS = [r for r in N.RUNS if r.cls in ("corr", "clamp", "eps") and r.ids == "dup" and N.regime(r.shape, r.segs)["K"] <= 512]


@pytest.mark.parametrize("r", AUTOGRAD_RUNS, ids=N.run_id)
def test_closed_form_gradient_equals_float64_autograd(r):
    """backward64 (clamp mask, eps branch of the Jacobian, 1 / (Q T), the positive at self Q + i) against autograd of the forward statement"""
    B, H, W, Cv, halo, P, C = r.shape
    src, tgt, ids, T, foreign = N.make_data(r)
    T = N.t32(T)
    foreign = [f.double() for f in foreign]
    s, t = R.gather64(src.double(), ids, C), R.gather64(tgt.double(), ids, C)
    fw = R.forward64(s, t, T, foreign, r.self_seg)
    assert float(((fw["raw"].abs() - R.CLAMP).abs()).min()) > 1e-9
    tt = t.clone().requires_grad_(True)
    loss = R.loss_autograd64(s, tt, T, N.WEIGHT, foreign, r.self_seg)
    loss.backward()
    torch.testing.assert_close(R.loss64(fw, N.WEIGHT), loss.detach(), **TOL)
    torch.testing.assert_close(R.backward64(fw, T, N.WEIGHT)[2].view(B, P, C), tt.grad, **TOL)


@pytest.mark.parametrize("shape", [s for s, _ in N.SHAPES], ids=lambda s: "x".join(map(str, s)))
def test_every_case_is_in_the_regime_it_names(shape):
    N.check_regime(shape)


def test_b1_s1_is_the_per_image_statement():
    """the float64 statements agree where the issue says they are the same statement"""
    from tests import nce_cases as N0
    from tests import nce_ref64 as R0
    r = N.EQUIV[0]
    src, tgt, ids, T, _ = N.make_data(r)
    C = r.shape[6]
    s, t = R.gather64(src.double(), ids, C), R.gather64(tgt.double(), ids, C)
    a, b = R.forward64(s, t, N.t32(T)), R0.forward64(s, t, N.t32(T))
    torch.testing.assert_close(R.loss64(a, N.WEIGHT), R0.loss64(b, N0.WEIGHT), **TOL)
    torch.testing.assert_close(R.backward64(a, N.t32(T), N.WEIGHT)[2], R0.backward64(b, N.t32(T), N0.WEIGHT)[2][0], **TOL)


@pytest.mark.parametrize("r", N.RUNS, ids=N.run_id)
def test_emulator_within_the_derived_bounds(r):
    N.body(make, r)


@pytest.mark.parametrize("r", N.EQUIV, ids=N.run_id)
def test_b1_s1_agrees_with_the_per_image_entry_points(r):
    N.body_equivalence(make, r)


def test_refused_arguments_return_their_error_and_write_nothing():
    N.body_refused(make)


@pytest.mark.parametrize("wrong,runs", N.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_rejects_a_wrong_reference(wrong, runs):
    """The results held to a deliberately wrong reference fail.  The op layer is never made to misbehave."""
    N.rejects(make, wrong, runs)
