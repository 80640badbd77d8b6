"""TEST INFRASTRUCTURE: float64 statements of the InstanceNorm kernel family (csrc/norm.hip), written from the definitions of the operations
and independent of tests/emulator.py.  tests/test_norm_family_cpu.py checks each of them against float64 autograd (F.instance_norm,
F.pad(mode="reflect" / "replicate") and the activation functions) at rtol = atol = 1e-12.

The family is split the way the kernels split it:
  * producers turn x into (mean, rstd): `sums64` + `stats_from_sums64` are float64 sums of the stored operand values;
  * consumers take (mean, rstd) AS AN INPUT -- the tests hand them the floats the producer itself wrote, so `x > mean` is the same exact
    comparison in kernel and reference and a ReLU / LeakyReLU mask can never differ between the two: `apply64`, `halo64`, `bwd64`,
    `fold_full64`, `act_bwd64`.
Tensors are (B, H, W, C) float64 unless a docstring says otherwise; a "view" is a gan_variant_research_amd.runtime.View.
"""
import numpy as np
import torch

EPS = 1e-5
EPS64 = float(np.float32(EPS))          # the float the C ABI receives
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
HALO_NONE, HALO_ZERO, HALO_REFLECT, HALO_REPLICATE = 0, 1, 2, 3


def reflect_index(i: torch.Tensor, n: int) -> torch.Tensor:
    """source index of position i of a reflect-padded axis of length n (no edge repeat: -1 -> 1, n -> n - 2)"""
    i = i.abs()
    return torch.where(i >= n, 2 * (n - 1) - i, i)


def pad_index(n: int, p: int, mode: int) -> torch.Tensor:
    """for each of the n + 2p padded positions of an axis, the interior index the padding copies from"""
    i = torch.arange(-p, n + p)
    return reflect_index(i, n) if mode == HALO_REFLECT else i.clamp(0, n - 1)


# ------------------------------------------------------------------------------------------------ producers
def sums64(v: torch.Tensor):
    """(sum, sum of squares) over the pixels: (B, C) each"""
    return v.sum((1, 2)), (v * v).sum((1, 2))


def stats_from_sums64(S, Q, HW, eps=EPS64):
    """(mean, var, rstd) of the biased estimator from whole-image sums; var is clamped at 0 like the kernels'"""
    mean = S / HW
    var = (Q / HW - mean * mean).clamp_min(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def stats64(v: torch.Tensor, eps=EPS64):
    S, Q = sums64(v)
    return stats_from_sums64(S, Q, v.shape[1] * v.shape[2], eps)


# ------------------------------------------------------------------------------------------------ consumers: forward
def act64(v, act, slope=0.2):
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_LRELU:
        return torch.where(v > 0, v, slope * v)
    if act == ACT_TANH:
        return torch.tanh(v)
    return v


def apply64(v, mean, rstd, act, residual=None, slope=0.2, residual_first=False):
    """act((v - mean) * rstd) + residual; mean, rstd: (B, C)"""
    xh = (v - mean[:, None, None, :]) * rstd[:, None, None, :]
    if residual is not None and residual_first:
        return act64(xh + residual, act, slope)
    out = act64(xh, act, slope)
    return out if residual is None else out + residual


def halo64(v, p, mode):
    """the (B, H + 2p, W + 2p, C) buffer a reflect / replicate halo fill of v makes"""
    ys, xs = pad_index(v.shape[1], p, mode), pad_index(v.shape[2], p, mode)
    return v[:, ys][:, :, xs]


# ------------------------------------------------------------------------------------------------ consumers: backward
def fold_full64(full, p, mode=HALO_REFLECT, corners=True, pad=None):
    """Gradient of a padding layer.  full: (B, H + 2p, W + 2p, C), the gradient on the padded domain; returns (B, H, W, C): every interior
    pixel collects the padded positions that the padding copied from it.  pad < p folds only the innermost `pad` halo pixels;
    corners=False folds rows and columns separately and leaves out the positions that are in the halo of both."""
    pad = p if pad is None else pad
    B, Hp, Wp, C = full.shape
    H, W = Hp - 2 * p, Wp - 2 * p
    full = full[:, p - pad:Hp - p + pad, p - pad:Wp - p + pad]
    ys, xs = pad_index(H, pad, mode), pad_index(W, pad, mode)
    if not corners:
        inner = full[:, pad:pad + H, pad:pad + W]
        rows = torch.zeros(B, H, W, C, dtype=full.dtype).index_add_(1, ys, full[:, :, pad:pad + W])
        cols = torch.zeros(B, H, W, C, dtype=full.dtype).index_add_(2, xs, full[:, pad:pad + H])
        return rows + cols - inner
    tmp = torch.zeros(B, H, full.shape[2], C, dtype=full.dtype).index_add_(1, ys, full)
    return torch.zeros(B, H, W, C, dtype=full.dtype).index_add_(2, xs, tmp)


def act_mask64(g, v, mean, act, slope=0.2):
    """g * act'(xhat) for relu / lrelu, the sign of xhat being that of v - mean"""
    pos = v > mean[:, None, None, :]
    if act == ACT_RELU:
        return g * pos
    if act == ACT_LRELU:
        return torch.where(pos, g, slope * g)
    return g


def bwd64(v, mean, rstd, gm, m1=None, m2=None):
    """InstanceNorm backward for an (already masked) gradient gm: rstd * (gm - mean(gm) - xhat * mean(gm * xhat)).  m1, m2 (B, C) replace
    the two means (gan_in_bwd_parts takes them from its caller's partial sums)."""
    xh = (v - mean[:, None, None, :]) * rstd[:, None, None, :]
    m1 = gm.mean((1, 2)) if m1 is None else m1
    m2 = (gm * xh).mean((1, 2)) if m2 is None else m2
    return rstd[:, None, None, :] * (gm - m1[:, None, None, :] - xh * m2[:, None, None, :])


def act_grad_from_out64(y, act, slope=0.2):
    """act' expressed through the activation's OUTPUT y"""
    if act == ACT_RELU:
        return (y > 0).double()
    if act == ACT_LRELU:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    if act == ACT_TANH:
        return 1 - y * y
    return torch.ones_like(y)


# ------------------------------------------------------------------------------------------------ on views (tests/fp8_producer_cases.py)
def norm_ref64(x, act, residual):
    """float64 InstanceNorm of the interior of view x: mean and variance from float64 sums of x, activation, residual"""
    v = x.nhwc().double()
    mean, _, rstd = stats64(v)
    out = apply64(v, mean, rstd, act, None if residual is None else residual.nhwc().double())
    return out, mean[:, None, None, :], rstd[:, None, None, :]


def fold64(g, fold):
    full = g.padded().double()
    p, H, W = g.halo, g.H, g.W
    if not fold:
        return full[:, p:p + H, p:p + W].clone()
    return fold_full64(full.cpu(), p).to(full.device)


def bwd_ref64(x, act, gy, fold):
    v = x.nhwc().double()
    mean, _, rstd = stats64(v)
    return bwd64(v, mean, rstd, act_mask64(fold64(gy, fold), v, mean, act))
