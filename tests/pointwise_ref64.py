"""TEST INFRASTRUCTURE: float64 statements of the loss, augmentation, pooling and layout entry points (csrc/pointwise.hip and the three
layout entry points of csrc/norm.hip), in plain torch, independent of tests/emulator.py.  Activations are (B, H, W, C real) float64 tensors
(the logical interior of a view); NCHW tensors are named so.  Every closed-form backward here is held to float64 autograd of its own forward
by tests/test_pointwise_family_cpu.py.

`Ref` carries the switches of the deliberately wrong statements of tests/pointwise_cases.py; the class itself is the true statement.
"""
import torch

HALO_NONE, HALO_REFLECT, HALO_REPLICATE = 0, 2, 3


class Ref:
    count_include_pad = False          # AvgPool2d(3, 2, 1, count_include_pad=False)
    pool_t_div9 = False                # the transpose pool divides by the window's own tap count, not by 9
    cut_exclusive = False              # the cutout's bounds are inclusive
    shift_sign = 1                     # y[h, w] reads x[h + tx, w + ty]
    contrast_per_channel = False       # the contrast mean is taken over (c, h, w)
    contrast_mean_raw = False          # ... of the image after the brightness shift
    sign0 = 0.0                        # sign(0) = 0
    kink = 0.0                         # |hinge derivative| at the kink, as relu' in torch
    no_dev_scale = False               # the L1 gradient carries *dev_grad_scale
    r1_factor = 2.0                    # u = scale * 2 / B * g
    n_minus_1 = False                  # means divide by n
    reflect_as_replicate = False


# ------------------------------------------------------------------------------------------------ DiffAugment
def aug_geometry(prm, H, W, ref=Ref):
    """(source row, source column, valid) per output pixel, each (B, H, W); valid = the source lies in the image and the pixel is not cut"""
    p = prm.double()
    B = p.shape[0]
    col = lambda i: p[:, i].long().view(B, 1, 1)
    hh, ww = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    sh, sw = hh + ref.shift_sign * col(3), ww + ref.shift_sign * col(4)
    inr = (sh >= 0) & (sh < H) & (sw >= 0) & (sw < W)
    if ref.cut_exclusive:
        cut = (hh >= col(5)) & (hh < col(6)) & (ww >= col(7)) & (ww < col(8))
    else:
        cut = (hh >= col(5)) & (hh <= col(6)) & (ww >= col(7)) & (ww <= col(8))
    return sh.clamp(0, H - 1).expand(B, H, W), sw.clamp(0, W - 1).expand(B, H, W), (inr & ~cut).expand(B, H, W)


def diffaug_colour64(x, prm, ref=Ref):
    """brightness, saturation about the per-pixel channel mean, contrast about the per-image mean of the saturated image: every source pixel"""
    B = x.shape[0]
    br, sat, con = (prm[:, i].double().view(B, 1, 1, 1) for i in range(3))
    t = x + br
    mc = t.mean(3, keepdim=True)
    s = (t - mc) * sat + mc
    if ref.contrast_per_channel:
        mu = s.mean((1, 2), keepdim=True)
    elif ref.contrast_mean_raw:
        mu = x.mean((1, 2, 3), keepdim=True)
    else:
        mu = s.mean((1, 2, 3), keepdim=True)
    return (s - mu) * con + mu


def diffaug_fwd64(x, prm, ref=Ref):
    B, H, W, C = x.shape
    sh, sw, valid = aug_geometry(prm, H, W, ref)
    bb = torch.arange(B).view(B, 1, 1).expand(B, H, W)
    col = diffaug_colour64(x, prm, ref)
    return torch.where(valid.unsqueeze(-1), col[bb, sh, sw], torch.zeros((), dtype=torch.float64))


def diffaug_bwd64(gy, prm, ref=Ref):
    """closed form: the masked gradient moved back to its source pixel, then the transposes of the contrast and saturation lines"""
    B, H, W, C = gy.shape
    sh, sw, valid = aug_geometry(prm, H, W, ref)
    bb = torch.arange(B).view(B, 1, 1).expand(B, H, W)
    g = torch.where(valid.unsqueeze(-1), gy, torch.zeros((), dtype=torch.float64))
    gsum = g.sum((1, 2, 3), keepdim=True)
    gs = torch.zeros_like(gy)
    gs.index_put_((bb[valid], sh[valid], sw[valid]), g[valid], accumulate=True)        # a shift: every source pixel is read at most once
    sat, con = (prm[:, i].double().view(B, 1, 1, 1) for i in (1, 2))
    gm = gsum / (C * H * W)
    if ref.contrast_per_channel:
        gm = g.sum((1, 2), keepdim=True) / (H * W)
    gc = con * gs + (1 - con) * gm
    return sat * gc + (1 - sat) * gc.mean(3, keepdim=True)


# ------------------------------------------------------------------------------------------------ losses
def patch_f64(v, mode, target):
    """the summand of mode 0..4 and its derivative away from the kink"""
    if mode == 0:
        return torch.relu(1 - v), -(v < 1).double()
    if mode == 1:
        return torch.relu(1 + v), (v > -1).double()
    if mode == 2:
        return -v, -torch.ones_like(v)
    if mode == 3:
        return (v - target) ** 2, 2 * (v - target)
    return torch.relu(v) - v * target + torch.log1p(torch.exp(-v.abs())), torch.sigmoid(v) - target          # BCE, the stable form


def patch_loss64(v, mode, target, scale, ref=Ref):
    """v: channel 0 of the logits (B, H, W).  -> (scale * mean f, scale / n * f')"""
    n = v.numel()
    f, d = patch_f64(v, mode, target)
    if ref.kink and mode in (0, 1):
        d = torch.where(v == (1.0 if mode == 0 else -1.0), torch.full_like(v, -ref.kink if mode == 0 else ref.kink), d)
    den = n - 1 if ref.n_minus_1 else n
    return scale * f.sum() / den, scale / n * d


def l1_loss64(x, t_nchw, scale, dev_scale, ref=Ref):
    d = x - t_nchw.permute(0, 2, 3, 1)
    n = d.numel()
    sg = torch.sign(d)
    sg = torch.where(d == 0, torch.full_like(d, ref.sign0), sg)
    gs = scale / n * (1.0 if dev_scale is None or ref.no_dev_scale else dev_scale)
    return scale * d.abs().sum() / (n - 1 if ref.n_minus_1 else n), gs * sg


def r1_reduce64(g, scale, ref=Ref):
    B = g.shape[0]
    return (g * g).sum() / B, scale * ref.r1_factor / B * g


# ------------------------------------------------------------------------------------------------ AvgPool2d(3, 2, 1, count_include_pad=False)
def pool_size(n):
    return (n - 1) // 2 + 1


def _pool_taps(x):
    """the nine strided taps of a zero-padded x (B, H, W, C), each (B, Ho, Wo, C)"""
    B, H, W, C = x.shape
    Ho, Wo = pool_size(H), pool_size(W)
    xp = torch.zeros(B, 2 * Ho + 1, 2 * Wo + 1, C, dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    return [xp[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2] for dy in range(3) for dx in range(3)]


def pool_counts(H, W, ref=Ref):
    """taps of each window that lie in the image, (1, Ho, Wo, 1)"""
    if ref.count_include_pad:
        return torch.full((1, pool_size(H), pool_size(W), 1), 9.0, dtype=torch.float64)
    return sum(_pool_taps(torch.ones(1, H, W, 1, dtype=torch.float64)))


def avgpool_fwd64(x, ref=Ref):
    """-> (mean of the taps inside the image, sum of their absolute values)"""
    cnt = pool_counts(x.shape[1], x.shape[2], ref)
    return sum(_pool_taps(x)) / cnt, sum(_pool_taps(x.abs()))


def avgpool_bwd64(gy, H, W, ref=Ref):
    """pool^T gy -> (value, sum of the absolute terms, their number), each (B, H, W, C)"""
    B, Ho, Wo, C = gy.shape
    cnt = torch.full((1, Ho, Wo, 1), 9.0, dtype=torch.float64) if ref.pool_t_div9 else pool_counts(H, W)
    q = gy / cnt
    out, mag, num = (torch.zeros(B, 2 * Ho + 1, 2 * Wo + 1, C, dtype=torch.float64) for _ in range(3))
    for dy in range(3):
        for dx in range(3):
            out[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2] += q
            mag[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2] += q.abs()
            num[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2] += 1
    return tuple(t[:, 1:H + 1, 1:W + 1] for t in (out, mag, num))


# ------------------------------------------------------------------------------------------------ layout
def halo_index(n, halo, mode, ref=Ref):
    """source index of every padded position -halo .. n + halo - 1"""
    i = torch.arange(-halo, n + halo)
    if mode == HALO_REPLICATE or (mode == HALO_REFLECT and ref.reflect_as_replicate):
        return i.clamp(0, n - 1)
    assert mode == HALO_REFLECT and halo < n
    i = i.abs()
    return torch.where(i >= n, 2 * (n - 1) - i, i)


def with_halo64(x, halo, mode, ref=Ref):
    """(B, H, W, C) -> (B, H + 2 halo, W + 2 halo, C): what a REFLECT or REPLICATE call leaves in the padded extent"""
    return x[:, halo_index(x.shape[1], halo, mode, ref)][:, :, halo_index(x.shape[2], halo, mode, ref)]


def nchw_to_nhwc64(src, C):
    """(B, Cr, H, W) -> (B, H, W, C), zero pad channels"""
    B, Cr, H, W = src.shape
    out = torch.zeros(B, H, W, C, dtype=torch.float64)
    out[..., :Cr] = src.double().permute(0, 2, 3, 1)
    return out
