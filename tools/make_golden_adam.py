"""Records every optimiser launch training.HipAdam.step and training.fused_adam_launch build BEFORE the three Adam front ends were put on
runtime.AdamPlan, for tests/test_adam_parent_launches.py.

The record was made on the commit before that change (this file copied into its tree) and is never recomputed from the code under test:

  python tools/make_golden_adam.py [--out FILE]      -> tests/golden/adam_parent_launches.json

Each case of CASES runs on tests.emulator_optim_wd.WdEmuOps behind a recording wrapper (RecAdamOps, handed out through
autograd._OPS_FACTORY).  Per adam_step / adam_step_wd call the record holds the entry point, every scalar argument, the contents of
chunk_tensor / chunk_off, the sizes of ws and norm_out, which optional device scalars were given, per table entry (numel, g given, ema
given), and the learning rate the launch found in lr_dev every time it ran.  Per case it also holds how many plans and tables were
built.  The tensors are [1, 5, ADAM_CHUNK, ADAM_CHUNK + 3] long: one chunk, one chunk, an exact fit and a spill-over.

  hipadam-*   three steps: all gradients; the rate halved, all gradients (same plan, table and op); the second parameter's .grad None
              (a plan of its own).  no decay / L2 / decoupled  x  EMA attached or not  x  max_grad_norm given or not
  groups      one step of two param groups, without and with decay
  fused-*     two calls at two rates (one plan, one table, one op).  no decay / L2 / decoupled  x  EMA or not  x  max_norm 0 or 1  x
              inv_scale + skip_nonfinite or neither
"""
from __future__ import annotations

import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_variant_research_amd import autograd as AG  # noqa: E402
from gan_variant_research_amd import training as T  # noqa: E402
from gan_variant_research_amd.runtime import ADAM_CHUNK  # noqa: E402
from tests.emulator_optim_wd import WdEmuOps  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "adam_parent_launches.json")
SIZES = [1, 5, ADAM_CHUNK, ADAM_CHUNK + 3]
LR, BETAS, EPS, WD, EMA_DECAY = 2e-4, (0.5, 0.999), 1e-8, 0.125, 0.75
DECAYS = {"plain": (0.0, False), "l2": (WD, False), "decoupled": (WD, True)}


class RecAdamOps(WdEmuOps):
    """WdEmuOps that appends what each adam_step / adam_step_wd / make_adam_table call was given to a shared log."""

    def __init__(self, log):
        super().__init__()
        self.log = log

    def make_adam_table(self, entries):
        self.log["tables"] += 1
        return super().make_adam_table(entries)

    def _rec(self, entry, build, table, ntensors, chunk_tensor, chunk_off, nchunks, lr, b1, b2, eps, max_norm, grad_scale, ema_decay, norm_out, ws,
             weight_decay=None, decoupled=None, lr_dev=None, inv_scale=None, skip_nonfinite=False):
        rec = {"entry": entry, "ntensors": ntensors, "nchunks": nchunks, "lr": lr, "b1": b1, "b2": b2, "eps": eps, "max_norm": max_norm,
               "grad_scale": grad_scale, "ema_decay": ema_decay, "weight_decay": weight_decay, "decoupled": decoupled,
               "skip_nonfinite": skip_nonfinite, "lr_dev": lr_dev is not None, "inv_scale": inv_scale is not None,
               "chunk_tensor": [chunk_tensor.dtype == torch.int32] + chunk_tensor.tolist(), "chunk_off": [chunk_off.dtype == torch.int64] + chunk_off.tolist(),
               "ws": ws.numel(), "norm_out": norm_out.numel(),
               "table": [[e["p"].numel(), e.get("g") is not None, e.get("ema") is not None] for e in table], "rates": []}
        self.log["calls"].append(rec)
        op = build()

        def run():
            rec["rates"].append(float(lr_dev) if lr_dev is not None else None)
            op()
        return run

    def adam_step(self, *a, **k):
        return self._rec("adam_step", lambda: WdEmuOps.adam_step(self, *a, **k), *a, **k)

    def adam_step_wd(self, *a, **k):
        return self._rec("adam_step_wd", lambda: WdEmuOps.adam_step_wd(self, *a, **k), *a, **k)


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in SIZES]


def _hipadam(log, decay, ema, clip):
    wd, dec = DECAYS[decay]
    ps = [torch.nn.Parameter(t) for t in _tensors(1)]
    opt = T.HipAdam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, decoupled_weight_decay=dec)
    if ema:
        opt.attach_ema({id(p): p.detach().clone() for p in ps}, EMA_DECAY)
    for s, (lr, dead) in enumerate(((LR, None), (LR / 2, None), (LR / 2, 1))):
        opt.param_groups[0]["lr"] = lr
        for i, (p, g) in enumerate(zip(ps, _tensors(2 + s))):
            p.grad = None if i == dead else g
        opt.step(max_grad_norm=1.0 if clip else None)
        log["plans"].append(len(opt._plans))


def _groups(log):
    ps = [torch.nn.Parameter(t) for t in _tensors(1)]
    opt = T.HipAdam([{"params": ps[:2], "weight_decay": 0.0}, {"params": ps[2:], "weight_decay": WD}], lr=LR, betas=BETAS, eps=EPS)
    for p, g in zip(ps, _tensors(2)):
        p.grad = g
    opt.step()
    log["plans"].append(len(opt._plans))


def _fused(log, decay, ema, clip, scaler):
    wd, dec = DECAYS[decay]
    saved, T._FUSED_PLANS = T._FUSED_PLANS, {}
    try:
        ps, m, v = _tensors(1), [torch.zeros(n) for n in SIZES], [torch.zeros(n) for n in SIZES]
        shadow = [p.clone() for p in ps] if ema else []
        steps, inv = torch.zeros(len(SIZES), dtype=torch.int32), torch.tensor([0.5]) if scaler else None
        for s, lr in enumerate((LR, LR / 2)):
            T.fused_adam_launch(ps, _tensors(2 + s), m, v, shadow, steps, lr, BETAS[0], BETAS[1], EPS, 1.0 if clip else 0.0, 2.0, EMA_DECAY, inv, scaler,
                                weight_decay=wd, decoupled=dec)
            log["plans"].append(len(T._FUSED_PLANS))
    finally:
        T._FUSED_PLANS = saved


_ON = lambda tag, on: tag if on else "no-" + tag
CASES = {"groups": (_groups, ())}
for _d, _e, _c in itertools.product(DECAYS, (False, True), (False, True)):
    CASES[f"hipadam-{_d}-{_ON('ema', _e)}-{_ON('clip', _c)}"] = (_hipadam, (_d, _e, _c))
for _d, _e, _c, _s in itertools.product(DECAYS, (False, True), (False, True), (False, True)):
    CASES[f"fused-{_d}-{_ON('ema', _e)}-{_ON('clip', _c)}-{_ON('scaler', _s)}"] = (_fused, (_d, _e, _c, _s))


def record(name):
    """Runs CASES[name] on recording op layers -> {"calls": [...], "tables": n, "plans": [plan count after each step]}."""
    log = {"calls": [], "tables": 0, "plans": []}
    saved, AG._OPS_FACTORY = AG._OPS_FACTORY, lambda device: RecAdamOps(log)
    try:
        fn, args = CASES[name]
        fn(log, *args)
    finally:
        AG._OPS_FACTORY = saved
    return json.loads(json.dumps(log))


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    rec = {name: record(name) for name in CASES}
    with open(out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
    print({k: len(v["calls"]) for k, v in rec.items()}, "->", out)
