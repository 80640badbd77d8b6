"""TEST INFRASTRUCTURE: float64 statements of what csrc/optim.hip and the fp32 helpers of csrc/util.hip replace, independent of the emulator.

  clip64 / coef64     torch.nn.utils.clip_grad_norm_: total = ||all live gradients||_2, coef = clamp(max_norm / (total + 1e-6), max = 1).
                      clamp keeps a NaN (torch.clamp(nan, max = 1) is nan), so a NaN gradient makes every gradient NaN; an Inf norm gives 0.
  adam64              one step of torch.optim.Adam's single-tensor path without amsgrad or weight decay (torch/optim/adam.py):
                      step += 1; m.lerp_(g, 1 - b1); v = b2 v + (1 - b2) g g; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
  ema64               EMA.update: shadow = decay shadow + (1 - decay) p_new
  step64              GradScaler.unscale_ (g *= inv_scale) / step (a non-finite norm skips everything) around the three above
  scaler_update64     torch.amp.GradScaler.update: scale *= backoff after an overflow (tracker = 0); otherwise tracker += 1 and, once it
                      reaches growth_interval, scale *= growth (tracker = 0); inv_scale = 1 / scale

`Ref` is the true statement; a subclass that overrides one of its attributes is a deliberately wrong one (tests/optim_cases.py: WRONG).
Scalars are the floats the C ABI receives; 1e-6 is the fp32 constant both torch (an fp32 tensor plus a Python scalar) and the kernel add.
"""
import math

import numpy as np
import torch

CHUNK = 16384
CLIP_EPS = float(np.float32(1e-6))
F32_MAX = 3.4028234663852886e38


class Ref:
    drop_last_chunk = False       # the norm without the last chunk of the grid
    drop_tail = False             # the norm over whole chunks only: without the n % 16384 last elements of every tensor
    bc_offset = 1                 # bias corrections at step + bc_offset
    eps_inside_sqrt = False
    ema_old_p = False
    clip_eps = CLIP_EPS
    scale_after_clip_only = False  # grad_scale left out of the norm (it then meets the gradient only with the coefficient)
    v_unclipped = False
    bump_skipped = False
    lr_from_arg = False


def sumsq64(tensors, gs, ref=Ref):
    """sum of squares of the scaled live gradients; tensors: dicts with g (float64 or None)"""
    live = [t["g"] * (1.0 if ref.scale_after_clip_only else gs) for t in tensors if t["g"] is not None]
    parts = []
    for g in live:
        n = g.numel()
        if ref.drop_tail and n % CHUNK:
            g = g[:n - n % CHUNK]
        parts.append(g)
    if ref.drop_last_chunk and parts:
        n = parts[-1].numel()
        parts[-1] = parts[-1][:((n - 1) // CHUNK) * CHUNK]
    return sum((float((g * g).sum()) for g in parts), 0.0)


def coef64(total, max_norm, ref=Ref):
    """clip_grad_norm_'s coefficient at a given norm; NaN stays NaN, Inf gives 0"""
    if not max_norm > 0:
        return 1.0
    c = max_norm / (total + ref.clip_eps)
    return c if math.isnan(c) else min(1.0, c)


def found_inf64(total):
    return not (abs(total) <= F32_MAX)


def adam64(t, lr, b1, b2, eps, gfac, ema_decay, ref=Ref, gfac_v=None):
    """-> (p, m, v, ema or None) after one step of a live tensor; gfac: the factor on g (scales and clip coefficient)"""
    g = t["g"] * gfac
    step = t["step"] + ref.bc_offset
    m = t["m"] + (1.0 - b1) * (g - t["m"])
    gv = t["g"] * gfac_v if ref.v_unclipped else g
    v = b2 * t["v"] + (1.0 - b2) * gv * gv
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = torch.sqrt(v / bc2 + eps) if ref.eps_inside_sqrt else torch.sqrt(v) / math.sqrt(bc2) + eps
    p = t["p"] - (lr / bc1) * (m / denom)
    ema = None
    if t["ema"] is not None:
        ema = ema_decay * t["ema"] + (1.0 - ema_decay) * (t["p"] if ref.ema_old_p else p)
    return p, m, v, ema


def step64(tensors, lr, b1, b2, eps, max_norm, grad_scale, inv_scale, ema_decay, skip_nonfinite, lr_dev=None, coef=None, ref=Ref):
    """One gan_adam_step in float64.  tensors: dicts p, g (or None), m, v, ema (or None) as float64 tensors and step (int).
    coef: the coefficient to apply (the family passes the one the kernel wrote); None: the statement's own.
    -> (norm, coef, found_inf, list of dicts p, m, v, ema, step)"""
    gs = grad_scale * (inv_scale if inv_scale is not None else 1.0)
    total = math.sqrt(sumsq64(tensors, gs, ref))
    own = coef64(total, max_norm, ref)
    coef = own if coef is None else coef
    found = found_inf64(total)
    rate = lr if (lr_dev is None or ref.lr_from_arg) else lr_dev
    out = []
    for t in tensors:
        if t["g"] is None or (skip_nonfinite and found):
            bump = int(ref.bump_skipped and not (skip_nonfinite and found))
            out.append(dict(p=t["p"], m=t["m"], v=t["v"], ema=t["ema"], step=t["step"] + bump))
            continue
        p, m, v, ema = adam64(t, rate, b1, b2, eps, gs * coef, ema_decay, ref, gfac_v=gs)
        out.append(dict(p=p, m=m, v=v, ema=ema, step=t["step"] + 1))
    return total, own, found, out


def scaler_update64(scale, tracker, found_inf, growth, backoff, interval):
    """-> (scale, inv_scale, tracker) after GradScaler.update"""
    if found_inf != 0.0:
        scale, tracker = scale * backoff, 0
    elif tracker + 1 >= interval:
        scale, tracker = scale * growth, 0
    else:
        tracker += 1
    return scale, 1.0 / scale, tracker
