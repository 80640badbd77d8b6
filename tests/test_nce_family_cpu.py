"""The PatchNCE kernels of csrc/patchnce.hip without a GPU: the float64 statement of tests/nce_ref64.py against float64 autograd, the regimes
the cases of tests/nce_cases.py name, the conditions the bounds rest on (asserted by the case builder for every run, no element excluded),
the emulator's statement inside the derived bounds (loss and gtgt; the emulator keeps no workspace) -- which therefore admit an honest fp32
implementation -- and every deliberately wrong reference outside them.  tests/test_nce_family_gpu.py runs the same bodies on the HIP
kernels."""
import pytest
import torch

from gan_variant_research_amd import BF16
from gan_variant_research_amd.runtime import Ctx
from tests import nce_cases as N
from tests import nce_ref64 as R
from tests.emulator import EmuOps

TOL = dict(rtol=1e-12, atol=1e-12)


def make():
    return Ctx(EmuOps(), "cpu", BF16)


AUTOGRAD_RUNS = [r for r in N.RUNS if r.cls in ("corr", "clamp", "eps") and r.shape[0] * r.shape[5] * r.shape[5] <= 2 * 240 * 240 and r.shape[0] <= 5]


@pytest.mark.parametrize("r", AUTOGRAD_RUNS, ids=N.run_id)
def test_closed_form_gradient_equals_float64_autograd(r):
    """backward64 (clamp mask, eps branch of the Jacobian, 1 / (P B T)) against autograd of the forward statement, on the stored inputs of
    the finite runs; the case builder's condition keeps every logit away from +-50, where the clamp has no derivative"""
    B, H, W, Cv, halo, P, C = r.shape
    src, tgt, ids, T = N.make_data(r)
    T = N.t32(T)
    s, t = R.gather64(src.double(), ids, C), R.gather64(tgt.double(), ids, C)
    fw = R.forward64(s, t, T)
    assert float(((fw["raw"].abs() - R.CLAMP).abs()).min()) > 1e-9
    tt = t.clone().requires_grad_(True)
    loss = R.loss_autograd64(s, tt, T, N.WEIGHT)
    loss.backward()
    torch.testing.assert_close(R.loss64(fw, N.WEIGHT), loss.detach(), **TOL)
    torch.testing.assert_close(R.backward64(fw, T, N.WEIGHT)[2], tt.grad, **TOL)


@pytest.mark.parametrize("shape", list(N.REGIME), ids=lambda s: "x".join(map(str, s)))
def test_case_is_in_the_regime_it_names(shape):
    N.check_regime(shape)
    B, H, W, Cv, halo, P, C = shape
    assert B * (H + 2 * halo) * (W + 2 * halo) * Cv <= 3.3e6


def test_every_listed_shape_and_class_is_run():
    for shape, _ in N.SHAPES:
        for dt in (N.BF16, N.F32):
            assert {r.cls for r in N.RUNS if r.shape == shape and r.dtype == dt} >= {"corr", "clamp", "eps"}
    for cls in ("corr", "clamp", "eps", "big", "nf_src_inf", "nf_tgt_nan", "nf_unsampled"):
        assert {N.regime(r.shape)["path"] for r in N.RUNS if r.cls == cls} == {"mfma", "scalar"}, cls
    for ids in ("dup", "perm", "equal"):
        assert {N.regime(r.shape)["path"] for r in N.RUNS if r.ids == ids} == {"mfma", "scalar"}, ids
    assert any(r.ids == "equal" and r.shape[5] == 256 for r in N.RUNS)          # the leader adds 256 rows
    assert len(set(N.RUNS)) == len(N.RUNS)


@pytest.mark.parametrize("r", N.RUNS, ids=N.run_id)
def test_emulated_family_within_the_derived_bounds(r):
    N.body(make, r)


@pytest.mark.parametrize("wrong,runs", N.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_emulated_family_rejects_a_wrong_reference(wrong, runs):
    N.rejects(make, wrong, runs)
