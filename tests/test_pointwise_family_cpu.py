"""The loss, augmentation, pooling and layout kernels without a GPU: every closed-form backward of tests/pointwise_ref64.py against float64
autograd of its own forward, the DiffAugment statement against the reference's own run (tests/golden/cut_losses.npz), the regimes the
cases of tests/pointwise_cases.py name, the emulator's statement inside the derived bounds -- which therefore admit an honest fp32
implementation -- and every deliberately wrong reference outside them.  tests/test_pointwise_family_gpu.py runs the same bodies on the HIP
kernels."""
import os

import numpy as np
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd import cut as C
from gan_variant_research_amd.runtime import Ctx
from tests import pointwise_cases as P
from tests import pointwise_ref64 as R
from tests.emulator import EmuOps

TOL = dict(rtol=1e-12, atol=1e-12)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cut_losses.npz")


def make():
    return Ctx(EmuOps(), "cpu", BF16)


def grad_of(f, x, w):
    x = x.clone().requires_grad_(True)
    (f(x) * w).sum().backward()
    return x.grad


@pytest.mark.parametrize("H,W,Cr", [(1, 1, 1), (24, 24, 3), (33, 31, 1), (9, 14, 3)])
def test_diffaug_backward_equals_float64_autograd(H, W, Cr):
    g = torch.Generator().manual_seed(H * 100 + W)
    prm = torch.zeros(10, 12)
    prm[:, :9] = torch.tensor(P.aug_rows(H, W))
    x = torch.randn(10, H, W, Cr, generator=g, dtype=torch.float64)
    gy = torch.randn(10, H, W, Cr, generator=g, dtype=torch.float64)
    torch.testing.assert_close(R.diffaug_bwd64(gy, prm), grad_of(lambda t: R.diffaug_fwd64(t, prm), x, gy), **TOL)
    wrong = P._wrong("PerChannel", contrast_per_channel=True)
    torch.testing.assert_close(R.diffaug_bwd64(gy, prm, wrong), grad_of(lambda t: R.diffaug_fwd64(t, prm, wrong), x, gy), **TOL)


def test_diffaug_statement_equals_the_reference_run():
    """aug.* of the golden file: DiffAugment(color, translation, cutout) of the reference, its draws remade as new_op_cases
    (tests/test_ops_library.py) makes them.  The reference ran in fp32: held to the fp32 bounds of the statement's own chain."""
    z = np.load(GOLDEN)
    aug = C.DiffAugment(["color", "translation", "cutout"])
    torch.manual_seed(int(z["aug.seed"]))
    prm = aug.to_params(aug.sample(3, 32, 32, None), 3, 32, 32)
    nhwc = lambda a: torch.tensor(a).double().permute(0, 2, 3, 1)
    x, y, w, gx = (nhwc(z["aug." + n]) for n in ("x", "y", "w", "gx"))
    B, H, W_ = 3, 32, 32
    sh, sw, valid = R.aug_geometry(prm, H, W_)
    bb = torch.arange(B).view(B, 1, 1).expand(B, H, W_)
    zero = torch.zeros((), dtype=torch.float64)
    v, _ = P.aug_fwd_tol(x, prm, F32)
    tol_y = torch.where(valid.unsqueeze(-1), v.stored(F32)[bb, sh, sw], zero)
    assert P.ratio(y, R.diffaug_fwd64(x, prm), tol_y) <= 1.0
    gv = torch.where(valid.unsqueeze(-1), w, zero)
    gs = torch.zeros_like(w)
    gs.index_put_((bb[valid], sh[valid], sw[valid]), gv[valid], accumulate=True)
    t, _ = P.aug_bwd_tol(gs, gv, prm, F32)
    assert P.ratio(gx, R.diffaug_bwd64(w, prm), t.stored(F32)) <= 1.0
    assert bool((~valid).any()) and float(prm[:, 3].abs().max()) > 0          # the run translates and cuts


@pytest.mark.parametrize("mode,target", P.PATCH_VARIANTS)
def test_patch_gradient_equals_float64_autograd(mode, target):
    g = torch.Generator().manual_seed(mode)
    v = torch.randn(3, 5, 7, generator=g, dtype=torch.float64) * 3          # no value on a kink
    v[0, 0, :2] = torch.tensor([60.0, -60.0], dtype=torch.float64)
    loss, grad = R.patch_loss64(v, mode, target, 0.7)
    torch.testing.assert_close(grad, grad_of(lambda t: R.patch_loss64(t, mode, target, 0.7)[0], v, torch.ones(())), **TOL)
    kink = torch.tensor([[[1.0, -1.0]]], dtype=torch.float64)              # relu' at 0 is 0 in torch
    if mode in (0, 1):
        want = grad_of(lambda t: 0.7 * torch.relu(1 - t if mode == 0 else 1 + t).mean(), kink, torch.ones(()))
        torch.testing.assert_close(R.patch_loss64(kink, mode, target, 0.7)[1], want, **TOL)
        assert float(want[0, 0, mode]) == 0.0


def test_l1_r1_and_pool_gradients_equal_float64_autograd():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 6, 3, generator=g, dtype=torch.float64)
    t = torch.randn(2, 3, 5, 6, generator=g, dtype=torch.float64)
    t[0, 1, 2, 3] = x[0, 2, 3, 1]                                           # sign(0) = 0, as torch's |.|' is
    loss, grad = R.l1_loss64(x, t, 0.7, 0.3)
    torch.testing.assert_close(grad, 0.3 * grad_of(lambda a: R.l1_loss64(a, t, 0.7, None)[0], x, torch.ones(())), **TOL)
    assert float(grad[0, 2, 3, 1]) == 0.0
    loss, u = R.r1_reduce64(x, 0.7)
    torch.testing.assert_close(u, 0.7 * grad_of(lambda a: R.r1_reduce64(a, 0.7)[0], x, torch.ones(())), **TOL)
    for H, W in P.POOL_SIZES:
        x = torch.randn(2, H, W, 8, generator=g, dtype=torch.float64)
        y = R.avgpool_fwd64(x)[0]
        gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        torch.testing.assert_close(R.avgpool_bwd64(gy, H, W)[0], grad_of(lambda a: R.avgpool_fwd64(a)[0], x, gy), **TOL)
        want = torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, count_include_pad=False).permute(0, 2, 3, 1)
        torch.testing.assert_close(y, want, **TOL)


def test_halo_statements_equal_torch_padding():
    x = torch.arange(2 * 4 * 5 * 2, dtype=torch.float64).view(2, 4, 5, 2)
    for mode, name in ((R.HALO_REFLECT, "reflect"), (R.HALO_REPLICATE, "replicate")):
        want = torch.nn.functional.pad(x.permute(0, 3, 1, 2), (3, 3, 3, 3), mode=name).permute(0, 2, 3, 1)
        assert torch.equal(R.with_halo64(x, 3, mode), want)


def test_every_listed_case_is_run_and_in_its_regime():
    for c in P.CASES:
        P.check_regime(c)
    assert len(set(P.CASES)) == len(P.CASES)
    for dt in P.DTYPES:
        ns = {c.shape[0] * c.shape[1] * c.shape[2] for c in P.CASES if c.group == "patch" and c.dtype == dt}
        assert ns == {1, 108, 1024, 1083, 9800}
        assert sum(1 for c in P.CASES if c.dtype == dt and c.shape[1] >= 420) == 3          # 725 x 725, 513 x 513, 420 x 420: once per dtype
    assert sum(len(cases) for _, cases in P.WRONG) >= 12 and len(P.WRONG) >= 12
    assert {c.group for _, cases in P.WRONG for c in cases} == {"patch", "l1", "r1", "aug", "pool", "layout"}


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_emulated_family_within_the_derived_bounds(c):
    P.body(make, c)


@pytest.mark.parametrize("wrong,cases", P.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_emulated_family_rejects_a_wrong_reference(wrong, cases):
    P.rejects(make, wrong, cases)


def test_worst_ratios_are_reported():
    P.worst_table()
