"""TEST INFRASTRUCTURE: the fused CycleGAN trainer (basic.CycleGANTrainer) in the configuration of tests/golden/basic_sn.npz, its launch
recorder and a run-time launch trace.  Never imported by the product package.

  * `basic_sn_config` / `make_trainer`: ngf 16, n_blocks 6, ndf 8, lsgan, lambda 10 / 0.5, Adam 2e-4 (0.5, 0.999); the modules come from
    basic.build_models after torch.manual_seed(0), as tools/make_golden_basic_sn.py builds the reference's.
  * `build_programs`: the trainer built on tests.emulator_fp8wgrad.RecOps -- every launch it plans, in planning order.  This function,
    run on the commit before spectral-norm discriminators existed, recorded tests/golden/basic_parent_launches.json.
  * `RunTrace`: RecOps whose launches also note, when they run, their index in the log: the order in which an iteration launched them.
"""
from __future__ import annotations

import os

import torch

from tests.emulator_fp8wgrad import RecOps

S_SN, B_SN = 64, 2


def basic_sn_config(sn: bool = True, amp: bool = False) -> dict:
    return {"training": {"amp": amp, "seed": 0}, "optim": {"lr_g": 2e-4, "lr_d": 2e-4, "betas": [0.5, 0.999]},
            "loss": {"gan": "lsgan", "lambda_cycle": 10.0, "lambda_identity": 0.5},
            "model": {"ngf": 16, "ndf": 8, "n_blocks": 6, "spectral_norm_d": sn}}


def make_models(cfg):
    from gan_variant_research_amd import basic as BG
    torch.manual_seed(0)
    return BG.build_models(cfg, "cpu")


def make_trainer(device, ops, sn=True, amp=False, S=S_SN, B=B_SN, **kw):
    from gan_variant_research_amd import basic as BG
    cfg = basic_sn_config(sn, amp)
    mods = make_models(cfg)
    tr = BG.CycleGANTrainer(*[m.to(device) for m in mods], cfg, B, S, device=device, amp=amp, ops=ops, **kw)
    return tr, mods


def golden_inputs(S=S_SN, B=B_SN):
    g = torch.Generator().manual_seed(77)
    a = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    b = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    return a, b


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "basic_sn.npz")
SN_KEYS = ("net.2", "net.5", "net.8")

# Tolerances (tests/cases.py:run_basic_iterations for the losses, optional_cases "bsn" for the spectral-norm gradients and buffers; the last
# two relative to max |ref|).  test_basic_sn_cpu.py checks them against the fixture's spread.* and wrong.* figures.
TOL = {"emulator": {"loss0": 2e-4, "loss1": 2e-3, "uv": 2e-4, "grad": 2e-3},
       "gpu_fp32": {"loss0": 1e-3, "loss1": 2e-3, "uv": 5e-4, "grad": 5e-3},
       "gpu_bf16": {"loss0": 4e-2, "uv": 5e-4}}


def rel_err(got, want) -> float:
    got, want = got.detach().double().cpu(), torch.as_tensor(want).double()
    return float((got - want).abs().max() / want.abs().max())


def golden_case(device, ops, tol, amp=False, niter=2, grads=True):
    """tests/golden/basic_sn.npz on the fused trainer: build_models reproduces the initial state, then `niter` iterations -- losses, u / v
    after every iteration and (grads) the iteration-0 D-step gradients of every D parameter, each printed before it is asserted."""
    import numpy as np
    g = np.load(GOLDEN)
    cfg = basic_sn_config(True, amp)
    mods = make_models(cfg)
    for name, m in zip(("G_ab", "G_ba", "D_A", "D_B"), mods):
        sd = m.state_dict()
        keys = [k[len(f"init.{name}."):] for k in g.files if k.startswith(f"init.{name}.")]
        assert list(sd) == keys, name
        for k in keys:
            want = torch.from_numpy(g[f"init.{name}.{k}"])
            got = sd[k].reshape(-1)[:16] if name.startswith("G") else sd[k]
            assert torch.equal(got, want), (name, k)
    from gan_variant_research_amd import basic as BG
    tr = BG.CycleGANTrainer(*[m.to(device) for m in mods], cfg, B_SN, S_SN, device=device, amp=amp, ops=ops)
    a, b = golden_inputs()
    dmods = {"D_A": mods[2], "D_B": mods[3]}
    for it in range(niter):
        got = tr.train_iteration(a.to(device), b.to(device))
        tl = tol["loss0" if it == 0 else "loss1"]
        for k, v in got.items():
            want = float(g[f"it{it}.{k}"])
            print(f"it{it} {k}: got {v:.7g} want {want:.7g} rel {abs(v - want) / abs(want):.3g} (rtol {tl})")
        for k, v in got.items():
            np.testing.assert_allclose(v, float(g[f"it{it}.{k}"]), rtol=tl, atol=1e-5, err_msg=f"it{it} {k}")
        if device != "cpu":
            torch.cuda.synchronize()
        errs = {}
        for name, D in dmods.items():
            sd = D.state_dict()
            for key in SN_KEYS:
                for s in ("u", "v"):
                    k = f"{key}.weight_{s}"
                    errs[f"it{it}.{name}.{k}"] = rel_err(sd[k], g[f"it{it}.{name}.{k}"])
        print("u / v:", " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
        assert all(e < tol["uv"] for e in errs.values()), {k: e for k, e in errs.items() if e >= tol["uv"]}
        if it == 0 and grads:      # the D-steps' gradients stay in the optimisers' blocks until the next D-step
            gerrs = {}
            for name, opt in (("D_A", tr.opt_DA), ("D_B", tr.opt_DB)):
                for k, v in opt.grads.items():
                    gerrs[f"{name}.{k}"] = rel_err(v, g[f"grad0.{name}.{k}"])
            print("iteration-0 D-step gradients:", " ".join(f"{k}={e:.2e}" for k, e in gerrs.items()))
            assert len(gerrs) == 14
            assert all(e < tol["grad"] for e in gerrs.values()), {k: e for k, e in gerrs.items() if e >= tol["grad"]}
    return tr, mods


def build_programs(ops, sn=False, amp=False):
    """Builds the trainer on a recording op layer; nothing is stepped.  -> (trainer, LaunchLog)."""
    rec = RecOps(ops)
    tr, _ = make_trainer("cpu", rec, sn=sn, amp=amp)
    return tr, rec.log


class RunTrace(RecOps):
    """RecOps + the run order: log.ran lists, per executed launch, (index into log.entries, the raw arguments)."""

    def __init__(self, inner, log=None, stream="main"):
        super().__init__(inner, log, stream)
        if not hasattr(self.log, "ran"):
            self.log.ran = []

    def side(self):
        if self._side is None:
            self._side = RunTrace(self._inner.side(), self.log, self._stream + ".side")
        return self._side

    def fork(self):
        return RunTrace(self._inner.fork(), self.log, self._stream + ".fork")

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr):
            return attr
        log = self.log

        def wrap(op, idx, raw):
            def run():
                log.ran.append((idx, raw))
                return op()
            run.__dict__.update(getattr(op, "__dict__", {}))
            return run

        def call(*a, **kw):
            out = attr(*a, **kw)
            islist = isinstance(out, list) and out and all(callable(o) for o in out)
            if callable(out) or islist:
                idx = len(log.entries)
                log.entries.append((self._stream, name, log.summary([list(a), kw])))
                raw = (name, a, kw)
                out = [wrap(o, idx, raw) for o in out] if islist else wrap(out, idx, raw)
            return out
        return call
