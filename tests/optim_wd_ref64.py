"""TEST INFRASTRUCTURE: float64 statement of one gan_adam_step_wd, independent of the emulator; tests/optim_ref64.py with torch's weight decay.

  L2 (decoupled = False)   torch.optim.Adam(weight_decay) -- torch/optim/adam.py, _single_tensor_adam: `grad = grad.add(param, alpha=weight_decay)`.
                           The reference runs scaler.unscale_ -> clip_grad_norm_ -> optimizer.step, so the parameter term joins the gradient
                           after scaling and clipping: g_eff = g gs coef + wd p; m, v and p then follow adam64 on g_eff.
  decoupled                torch.optim.AdamW / Adam(decoupled_weight_decay=True) -- same function: `param.mul_(1 - lr * weight_decay)` before
                           anything else; m and v from the undecayed gradient; p = p (1 - lr wd) - (lr / bc1) m / denom.
  Both: the norm, the coefficient and found_inf see the scaled gradients only; a tensor without a gradient is skipped entirely, decay
  included (torch's _init_group leaves out a parameter whose grad is None); a step that GradScaler skips decays nothing; the EMA reads p_new.

`WdRef` is the true statement; a subclass that overrides one attribute is a deliberately wrong one (tests/optim_wd_cases.py: WRONG).
"""
import math

import torch

from tests import optim_ref64 as R


class WdRef(R.Ref):
    wd_in_norm = False              # the norm is taken over g gs + wd p
    wd_before_clip = False          # (g gs + wd p) coef: the decay is scaled by the clip coefficient
    wd_on_skipped = False           # a tensor without a gradient is decayed all the same (p (1 - lr wd))
    wd_on_nonfinite_skip = False    # a step skipped for a non-finite norm decays all the same
    swap_mode = False               # L2 where decoupled was asked, and the reverse
    decoupled_after = False         # (p - step) (1 - lr wd) instead of p (1 - lr wd) - step
    decoupled_lr_from_arg = False   # the factor 1 - lr wd from the argument `lr` when lr_dev is given
    v_undecayed = False             # L2: v from g gs coef, without wd p
    ema_undecayed_p = False         # the EMA reads the p that the step without decay gives


def sumsq64_wd(tensors, gs, wd, ref=WdRef):
    if not ref.wd_in_norm:
        return R.sumsq64(tensors, gs, ref)
    return sum((float(((t["g"] * gs + wd * t["p"]) ** 2).sum()) for t in tensors if t["g"] is not None), 0.0)


def adam64_wd(t, rate, rate_decay, b1, b2, eps, gs, coef, ema_decay, wd, decoupled, ref=WdRef):
    """-> (p, m, v, ema or None) after one step of a live tensor"""
    decoupled = (not decoupled) if ref.swap_mode else decoupled
    g = t["g"] * (gs * coef)
    g_eff = g
    if not decoupled:
        g_eff = (t["g"] * gs + wd * t["p"]) * coef if ref.wd_before_clip else g + wd * t["p"]
    step = t["step"] + 1
    m = t["m"] + (1.0 - b1) * (g_eff - t["m"])
    gv = g if (ref.v_undecayed and not decoupled) else g_eff
    v = b2 * t["v"] + (1.0 - b2) * gv * gv
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    upd = (rate / bc1) * (m / (torch.sqrt(v) / math.sqrt(bc2) + eps))
    keep = 1.0 - rate_decay * wd
    if decoupled:
        p = (t["p"] - upd) * keep if ref.decoupled_after else t["p"] * keep - upd
    else:
        p = t["p"] - upd
    ema = None
    if t["ema"] is not None:
        src = p
        if ref.ema_undecayed_p:            # the parameter an Adam step without any decay would have written
            m0 = t["m"] + (1.0 - b1) * (g - t["m"])
            v0 = b2 * t["v"] + (1.0 - b2) * g * g
            src = t["p"] - (rate / bc1) * (m0 / (torch.sqrt(v0) / math.sqrt(bc2) + eps))
        ema = ema_decay * t["ema"] + (1.0 - ema_decay) * src
    return p, m, v, ema


def step64_wd(tensors, lr, b1, b2, eps, max_norm, grad_scale, inv_scale, ema_decay, skip_nonfinite, wd, decoupled, lr_dev=None, coef=None, ref=WdRef):
    """One gan_adam_step_wd in float64; arguments and result as optim_ref64.step64, with the decay and its mode."""
    gs = grad_scale * (inv_scale if inv_scale is not None else 1.0)
    total = math.sqrt(sumsq64_wd(tensors, gs, wd, ref))
    own = R.coef64(total, max_norm, ref)
    coef = own if coef is None else coef
    found = R.found_inf64(total)
    rate = lr if lr_dev is None else lr_dev
    rate_decay = lr if (lr_dev is None or ref.decoupled_lr_from_arg) else lr_dev
    out = []
    for t in tensors:
        skipped_step = bool(skip_nonfinite and found)
        if t["g"] is None or skipped_step:
            decay = (ref.wd_on_nonfinite_skip and skipped_step) or (ref.wd_on_skipped and t["g"] is None and not skipped_step)
            out.append(dict(p=t["p"] * (1.0 - rate * wd) if decay else t["p"], m=t["m"], v=t["v"], ema=t["ema"], step=t["step"]))
            continue
        p, m, v, ema = adam64_wd(t, rate, rate_decay, b1, b2, eps, gs, coef, ema_decay, wd, decoupled, ref)
        out.append(dict(p=p, m=m, v=v, ema=ema, step=t["step"] + 1))
    return total, own, found, out
