"""The optimiser kernels and the fp32 helpers without a GPU: the float64 statement of tests/optim_ref64.py against torch.optim.Adam,
clip_grad_norm_ and torch.amp.GradScaler's own update rule, the regimes the tables of tests/optim_cases.py name, the emulator's statement
inside the derived bounds -- which therefore admit an honest fp32 implementation -- and every deliberately wrong reference outside them.
tests/test_optim_family_gpu.py runs the same bodies on the HIP kernels."""
import math

import numpy as np
import pytest
import torch

from gan_variant_research_amd import BF16
from gan_variant_research_amd import autograd as AG
from gan_variant_research_amd.runtime import Ctx
from tests import optim_cases as P
from tests import optim_ref64 as R
from tests.emulator import EmuOps


def make():
    return Ctx(EmuOps(), "cpu", BF16)


@pytest.fixture(autouse=True)
def _emulated_launches(monkeypatch):
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: EmuOps())          # training.fused_adam_launch builds its own context


@pytest.mark.parametrize("max_norm", [0.0, 0.05, 100.0])
def test_statement_equals_torch_adam_and_clip_grad_norm(max_norm):
    """three steps of torch.optim.Adam + clip_grad_norm_ + the reference's EMA.update on float64 tensors, one of them without a gradient"""
    g = torch.Generator().manual_seed(3)
    shapes = [(5,), (3, 4), (7,)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in shapes]
    lr, b1, b2, eps, decay = 1e-3, 0.4, 0.99, 1e-6, 0.9
    opt = torch.optim.Adam(ps, lr=lr, betas=(b1, b2), eps=eps)
    mine = [dict(p=p.detach().clone().reshape(-1), m=torch.zeros(p.numel(), dtype=torch.float64), v=torch.zeros(p.numel(), dtype=torch.float64),
                 ema=p.detach().clone().reshape(-1), g=None, step=0) for p in ps]
    shadow = [p.detach().clone() for p in ps]
    for s in range(3):
        for i, p in enumerate(ps):
            p.grad = None if (i == 1 and s == 1) else torch.randn(p.shape, generator=g, dtype=torch.float64)
            mine[i]["g"] = None if p.grad is None else p.grad.clone().reshape(-1)
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm) if max_norm > 0 else None
        opt.step()
        for sh, p, t in zip(shadow, ps, mine):
            if t["g"] is not None:
                sh.mul_(decay).add_(p.detach(), alpha=1 - decay)
        norm, coef, found, out = R.step64(mine, lr, b1, b2, eps, max_norm, 1.0, None, decay, False)
        if total is not None:
            assert abs(norm - float(total)) <= 1e-12 * norm
        for t, o_, p, sh in zip(mine, out, ps, shadow):
            t.update(o_)
            torch.testing.assert_close(t["p"], p.detach().reshape(-1), rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(t["ema"], sh.reshape(-1), rtol=1e-12, atol=1e-12)
            if p in opt.state and opt.state[p]:
                torch.testing.assert_close(t["m"], opt.state[p]["exp_avg"].reshape(-1), rtol=1e-12, atol=1e-12)
                torch.testing.assert_close(t["v"], opt.state[p]["exp_avg_sq"].reshape(-1), rtol=1e-12, atol=1e-12)
                assert t["step"] == int(opt.state[p]["step"])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_statement_of_the_non_finite_coefficient_is_torchs(bad):
    """clip_grad_norm_ on this build: one NaN makes every gradient of every tensor NaN; an Inf gives the coefficient 0"""
    ps = [torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(3))]
    ps[0].grad, ps[1].grad = torch.tensor([1.0, bad, 2.0, 3.0]), torch.ones(3)
    total = float(torch.nn.utils.clip_grad_norm_(ps, 10.0))
    coef = R.coef64(total, 10.0)
    if math.isnan(bad):
        assert math.isnan(coef) and all(bool(torch.isnan(p.grad).all()) for p in ps)
    else:
        assert coef == 0.0 and bool((ps[1].grad == 0).all()) and bool(torch.isnan(ps[0].grad[1])) and bool((ps[0].grad[[0, 2, 3]] == 0).all())
    assert R.found_inf64(total)


def test_scaler_statement_equals_torch_gradscaler_update_rule():
    """torch.amp.GradScaler.update -> torch._amp_update_scale_, driven directly"""
    for name, (seq, interval, growth, backoff, s0) in P.SCALER_SEQS.items():
        scale, trk = torch.tensor([s0], dtype=torch.float32), torch.zeros(1, dtype=torch.int32)       # the op takes fp32 only
        mine, mt = float(scale), 0
        for fi in seq:
            torch._amp_update_scale_(scale, trk, torch.tensor([float(fi)]), growth, backoff, interval)
            mine, _, mt = R.scaler_update64(mine, mt, fi, float(np.float32(growth)), float(np.float32(backoff)), interval)
            assert abs(mine - float(scale)) <= 2.0 ** -24 * abs(mine) + 2.0 ** -150 and mt == int(trk), name
            mine = float(scale)           # one rounding per call


def test_every_table_is_in_its_regime():
    for c in P.CASES:
        P.check_regime(c)
    assert len({c.name for c in P.CASES}) == len(P.CASES) and len(P.WRONG) >= 10
    assert all(n in P.BY_NAME for _, names in P.WRONG for n in names)


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_emulated_family_within_the_derived_bounds(c):
    P.body(make, c)


@pytest.mark.parametrize("name", list(P.SCALER_SEQS))
def test_emulated_scaler_update(name):
    P.body_scaler(make, name)


@pytest.mark.parametrize("n", P.HELPER_N)
def test_emulated_fill_and_axpy(n):
    P.body_fill_axpy(make, n)


@pytest.mark.parametrize("wrong,names", P.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_emulated_family_rejects_a_wrong_reference(wrong, names):
    P.rejects(make, wrong, names)


def test_worst_ratios_are_reported_and_no_bound_is_idle():
    for c in P.CASES:          # run alone, this test fills the table itself (results are cached per case)
        P.body(make, c)
    for name in P.SCALER_SEQS:
        P.body_scaler(make, name)
    P.body_fill_axpy(make, 257)
    worst = P.worst_table(False)
    idle = {g: r for g, r in worst.items() if r < 0.01}
    assert not idle, f"bounds too loose to catch anything: {idle}"
