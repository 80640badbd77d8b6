"""The fused CycleGAN trainer with spectral-norm discriminators on the MI355X: the reference's two iterations (tests/golden/basic_sn.npz) in
fp32 and bf16, and one iteration at the bench size (BASELINE.json configs[1]) against float64 power iterations."""
import math

import pytest
import torch

from tests import emulator_basic_sn as E

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _ops():
    from gan_variant_research_amd.runtime import HipOps
    return HipOps(torch.device(DEV))


def test_golden_fp32_on_hip():
    E.golden_case(DEV, _ops(), E.TOL["gpu_fp32"])


def test_golden_bf16_iteration0_on_hip():
    """bf16: iteration-0 losses and u / v after iteration 0.  All three power iterations of each discriminator in iteration 0 run before its
    first update, on the initial fp32 weight_orig: bf16 activations do not reach u and v."""
    E.golden_case(DEV, _ops(), E.TOL["gpu_bf16"], amp=True, niter=1, grads=False)


def _power_iterations64(W, u, v, n, eps=1e-12):
    m = W.double().reshape(W.shape[0], -1)
    u, v = u.double(), v.double()
    for _ in range(n):
        v = torch.nn.functional.normalize(m.t() @ u, dim=0, eps=eps)
        u = torch.nn.functional.normalize(m @ v, dim=0, eps=eps)
    return u, v


def test_bench_size_one_iteration():
    """BASELINE.json configs[1] (ngf 64, 9 blocks, ndf 64, 64x64, batch 256, bf16) with spectral_norm_d: one iteration -- finite losses, and u / v
    of the six spectral-norm convolutions within 5e-4 (of max |ref|) of three float64 power iterations from the initial weight_orig / u / v."""
    from gan_variant_research_amd import basic as BG
    cfg = {"training": {"amp": True, "seed": 0}, "optim": {"lr_g": 2e-4, "lr_d": 2e-4, "betas": [0.5, 0.999]},
           "loss": {"gan": "lsgan", "lambda_cycle": 10.0, "lambda_identity": 0.5},
           "model": {"ngf": 64, "ndf": 64, "n_blocks": 9, "spectral_norm_d": True}}
    B, S = 256, 64
    torch.manual_seed(0)
    mods = BG.build_models(cfg, "cpu")
    init = {n: {k: v.clone() for k, v in D.state_dict().items()} for n, D in (("D_A", mods[2]), ("D_B", mods[3]))}
    tr = BG.CycleGANTrainer(*[m.to(DEV) for m in mods], cfg, B, S, device=DEV, amp=True, ops=_ops())
    g = torch.Generator().manual_seed(1234)
    a = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(DEV)
    b = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(DEV)
    losses = tr.train_iteration(a, b)
    torch.cuda.synchronize()
    print("losses:", losses)
    assert all(math.isfinite(v) for v in losses.values()), losses
    errs = {}
    for n, D in (("D_A", mods[2]), ("D_B", mods[3])):
        sd = D.state_dict()
        for key in E.SN_KEYS:
            u64, v64 = _power_iterations64(init[n][key + ".weight_orig"], init[n][key + ".weight_u"], init[n][key + ".weight_v"], 3)
            errs[f"{n}.{key}.u"] = E.rel_err(sd[key + ".weight_u"], u64)
            errs[f"{n}.{key}.v"] = E.rel_err(sd[key + ".weight_v"], v64)
    print("u / v vs three float64 power iterations:", " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
    assert all(e < 5e-4 for e in errs.values()), errs
