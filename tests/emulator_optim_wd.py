"""TEST INFRASTRUCTURE: emulator statement of gan_adam_step_wd.

`WdEmuOps` is tests.emulator.EmuOps plus adam_step_wd, an fp32 restatement of csrc/optim.hip's decaying instantiations in torch, so the host
code that plans a decaying optimiser step (cut.FusedAdam, training.HipAdam, training.fused_adam_launch, cut.CutTrainer) runs on the CPU.
weight_decay == 0 goes to EmuOps.adam_step, as the C entry point launches gan_adam_step's kernels.  Never imported by the product package.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.emulator import EmuOps


class WdEmuOps(EmuOps):
    def adam_step_wd(self, table, ntensors, chunk_tensor, chunk_off, nchunks, lr, b1, b2, eps, max_norm, grad_scale, ema_decay, norm_out, ws,
                     weight_decay, decoupled=False, lr_dev=None, inv_scale=None, skip_nonfinite=False):
        f32 = lambda x: float(np.float32(x))
        if not weight_decay >= 0.0 or decoupled not in (0, 1, False, True):
            raise ValueError("adam_wd: weight_decay must be >= 0 and decoupled 0 or 1")
        if weight_decay == 0.0:
            return self.adam_step(table, ntensors, chunk_tensor, chunk_off, nchunks, lr, b1, b2, eps, max_norm, grad_scale, ema_decay, norm_out, ws,
                                  lr_dev=lr_dev, inv_scale=inv_scale, skip_nonfinite=skip_nonfinite)
        lr, b1, b2, eps, max_norm, grad_scale, ema_decay, wd = (f32(x) for x in (lr, b1, b2, eps, max_norm, grad_scale, ema_decay, weight_decay))

        def op():
            gs = grad_scale * (float(inv_scale) if inv_scale is not None else 1.0)
            rate = float(lr_dev) if lr_dev is not None else lr
            live = [e for e in table if e.get("g") is not None]
            tot = math.sqrt(sum(float(((e["g"] * gs) ** 2).sum()) for e in live))          # the decay is not in the norm
            clip = max_norm / (tot + 1e-6)
            coef = (clip if math.isnan(clip) else min(1.0, clip)) if max_norm > 0 else 1.0
            found = not math.isfinite(tot)
            norm_out[0], norm_out[1], norm_out[2] = tot, coef, float(found)
            if skip_nonfinite and found:
                return
            keep = f32(1.0 - f32(rate * wd))
            for e in live:
                g = e["g"] * f32(gs * coef)
                if decoupled:
                    e["p"].mul_(keep)
                else:
                    g = g + wd * e["p"]
                t = int(e["step"]) + 1
                e["step"].fill_(t)
                e["m"].lerp_(g, 1 - b1)
                e["v"].mul_(b2).addcmul_(g, g, value=1 - b2)
                bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
                denom = (e["v"].sqrt() / math.sqrt(bc2)).add_(eps)
                e["p"].addcdiv_(e["m"], denom, value=-(rate / bc1))
                if e.get("ema") is not None:
                    e["ema"].copy_((1.0 - ema_decay) * e["p"] + ema_decay * e["ema"])
        return op
