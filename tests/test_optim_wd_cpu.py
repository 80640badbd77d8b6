"""gan_adam_step_wd without a GPU: the float64 statement of tests/optim_wd_ref64.py against torch.optim.Adam(weight_decay), torch.optim.AdamW
and Adam(decoupled_weight_decay=True) behind clip_grad_norm_, the emulator's statement (tests/emulator_optim_wd.py) inside the derived bounds
of tests/optim_wd_cases.py -- which therefore admit an honest fp32 implementation -- and every deliberately wrong reference outside them.
tests/test_optim_wd_gpu.py runs the same bodies on the HIP kernels."""
import pytest
import torch

from gan_variant_research_amd import BF16
from gan_variant_research_amd import autograd as AG
from gan_variant_research_amd.runtime import Ctx
from tests import optim_wd_cases as Q
from tests import optim_wd_ref64 as W
from tests.emulator_optim_wd import WdEmuOps


def make():
    return Ctx(WdEmuOps(), "cpu", BF16)


@pytest.fixture(autouse=True)
def _emulated_launches(monkeypatch):
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: WdEmuOps())          # fused_adam_launch and HipAdam build their own context


@pytest.mark.parametrize("kind", ["adam-l2", "adamw", "adam-decoupled"])
@pytest.mark.parametrize("max_norm", [0.0, 0.05])
def test_statement_equals_torch(kind, max_norm):
    """three steps of torch's optimiser behind clip_grad_norm_ with the reference's EMA.update, on float64 tensors, one step without a
    gradient for one tensor (which torch then leaves alone, decay included)"""
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in [(5,), (3, 4), (7,)]]
    lr, b1, b2, eps, decay, wd = 1e-2, 0.4, 0.99, 1e-6, 0.9, 0.1
    kw = dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    opt = {"adam-l2": lambda: torch.optim.Adam(ps, **kw), "adamw": lambda: torch.optim.AdamW(ps, **kw),
           "adam-decoupled": lambda: torch.optim.Adam(ps, decoupled_weight_decay=True, **kw)}[kind]()
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
        norm, coef, found, out = W.step64_wd(mine, lr, b1, b2, eps, max_norm, 1.0, None, decay, False, wd, kind != "adam-l2")
        if total is not None:
            assert abs(norm - float(total)) <= 1e-12 * norm
        for t, o_, p, sh in zip(mine, out, ps, shadow):
            t.update(o_)
            torch.testing.assert_close(t["p"], p.detach().reshape(-1), rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(t["ema"], sh.reshape(-1), rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(t["m"], opt.state[p]["exp_avg"].reshape(-1), rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(t["v"], opt.state[p]["exp_avg_sq"].reshape(-1), rtol=1e-12, atol=1e-12)
            assert t["step"] == int(opt.state[p]["step"])


def test_every_case_is_listed_once_and_every_wrong_reference_names_cases():
    for c in Q.CASES:
        Q.P.check_regime(c)
    assert len({c.name for c in Q.CASES}) == len(Q.CASES) and len(Q.WRONG) == 9
    assert all(n in Q.BY_NAME for _, names in Q.WRONG for n in names)


@pytest.mark.parametrize("c", Q.CASES, ids=Q.case_id)
def test_emulated_family_within_the_derived_bounds(c):
    Q.body(make, c)


@pytest.mark.parametrize("wrong,names", Q.WRONG, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_emulated_family_rejects_a_wrong_reference(wrong, names):
    Q.rejects(make, wrong, names)


@pytest.mark.parametrize("decoupled", [False, True])
def test_emulated_zero_decay_is_adam_step_bit_for_bit(decoupled):
    Q.body_zero_decay_is_adam_step(make, decoupled)


def test_worst_ratios_are_reported_and_no_bound_is_idle():
    for c in Q.CASES:          # run alone, this test fills the table itself (results are cached per case)
        Q.body(make, c)
    worst = Q.worst_table(False)
    idle = {g: r for g, r in worst.items() if r < 0.01}
    assert not idle, f"bounds too loose to catch anything: {idle}"
