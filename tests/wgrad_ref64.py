"""TEST INFRASTRUCTURE: float64 statements of the weight-gradient family (csrc/conv_wgrad.hip, wgrad_patch.hip, conv_win7.hip):
the partial slabs of gan_conv_wgrad at the level of its descriptor, the layer's weight gradient, gan_wgrad_reduce's index formula and
gan_bias_grad's column sums.  Plain indexing and matmul in float64, on whatever device the operands are on; used by tests/wgrad_cases.py."""
from collections import namedtuple

import torch

from tests.cases import conv_ref64

# what gan_wgrad_desc says about addressing: rows m = (b, ho, wo) of g against the taps of x
Desc = namedtuple("Desc", "B Ho Wo Cx N ntaps x_Wp x_y0 x_x0 x_sy x_sx g_y0 g_x0 g_sy g_sx tapoff")


def desc_of(c):
    """the addressing of a planned runtime.WgradCall"""
    return Desc(c.B, c.Ho, c.Wo, c.Cx, c.N, c.ntaps, c.x.Wp, c.x_y0, c.x_x0, c.x_sy, c.x_sx, c.g_y0, c.g_x0, c.g_sy, c.g_sx,
                tuple(int(v) for v in c.tapoff.tolist()))


def slab_rows(M, nsplit):
    """rows per split of the generic kernel, as gan_conv_wgrad computes them: ceil(ceil(M / nsplit) / 64) * 64"""
    return -(-(-(-M // nsplit)) // 64) * 64


def desc64(d, xpad, gpad, ranges=None, absolute=False, shift_first_row=False, swap_taps=False):
    """part[n][t][c] = sum_m g[row m][n] * x[row m + tap t][c] over the pixel ranges [(m0, m1), ...] (default: all pixels), one result per
    range: (len(ranges), N, ntaps, Cx) float64.  xpad / gpad: the padded buffers (B, Hp, Wp, C) as float64.  Taps go through tapoff, pixels
    through the strides and origins of the descriptor; the halo of g is never indexed.
    shift_first_row (a wrong statement): the first row of every range but the first is counted in the range before it.
    swap_taps (a wrong statement): tap (kh, kw) reads the pixel of tap (kw, kh)."""
    M = d.B * d.Ho * d.Wo
    ranges = [(0, M)] if ranges is None else list(ranges)
    if shift_first_row:
        ranges = [(m0 + (1 if i else 0), min(M, m1 + 1) if i + 1 < len(ranges) else m1) for i, (m0, m1) in enumerate(ranges)]
    if absolute:
        xpad, gpad = xpad.abs(), gpad.abs()
    dev = xpad.device
    m = torch.arange(M, device=dev)
    b, r = m // (d.Ho * d.Wo), m % (d.Ho * d.Wo)
    ho, wo = r // d.Wo, r % d.Wo
    gm = gpad[b, d.g_y0 + ho * d.g_sy, d.g_x0 + wo * d.g_sx, :d.N]
    out = torch.zeros(len(ranges), d.N, d.ntaps, d.Cx, dtype=torch.float64, device=dev)
    k = int(round(d.ntaps ** 0.5))
    for t, off in enumerate(d.tapoff):
        assert off % d.Cx == 0
        dy, dx = divmod(off // d.Cx, d.x_Wp)
        if swap_taps:
            assert k * k == d.ntaps
            dy, dx = dx, dy
        xm = xpad[b, d.x_y0 + ho * d.x_sy + dy, d.x_x0 + wo * d.x_sx + dx, :]
        for i, (m0, m1) in enumerate(ranges):
            out[i, :, t, :] = gm[m0:m1].t() @ xm[m0:m1]
    return out


def layer64(k, s, p, tr, reflect, x, dy, wshape, swap_taps=False, zero_pad=False, wrong_stride=False):
    """(ref, A, K) of the layer's weight gradient in the layer's own weight layout: tests/cases.conv_ref64('wgrad').
    wrong statements: swap_taps (kh and kw exchanged), zero_pad (zero padding where the layer reflects), wrong_stride (transposed layer:
    the stride thins out dy instead of stepping the window over it)."""
    w = torch.zeros(wshape, dtype=torch.float64, device=x.device)
    if wrong_stride and tr:
        from tests.cases import _c_bwd_w
        import torch.nn.functional as F
        f = lambda xv, dyv: _c_bwd_w(F.pad(dyv[:, :, ::2, ::2], (1, 1, 1, 1)), xv, 3, 1)
        ref, A, K = f(x, dy), f(x.abs(), dy.abs()), x.shape[0] * x.shape[2] * x.shape[3]
    else:
        ref, A, K = conv_ref64("wgrad", k, s, p, tr, reflect and not zero_pad, w, x=x, dy=dy)
    if swap_taps:
        ref, A = ref.transpose(2, 3).contiguous(), A.transpose(2, 3).contiguous()
    return ref, A, K


def bias64(dy_view_padded, halo, H, W, cout, with_halo=False):
    """(ref, A, K): column sums of the logical pixels of dy (B, Hp, Wp, C) float64.  with_halo (a wrong statement): the halo is summed too."""
    v = dy_view_padded if with_halo else dy_view_padded[:, halo:halo + H, halo:halo + W]
    v = v[..., :cout]
    return v.sum((0, 1, 2)), v.abs().sum((0, 1, 2)), dy_view_padded.shape[0] * H * W


def reduce_index(N_real, C_real, swap, I2, KK, k, device="cpu"):
    """element of grad that (n, c) of a tap with khw = k lands on: ((c * I2 + n) if swap else (n * I2 + c)) * KK + k"""
    n = torch.arange(N_real, device=device)[:, None]
    c = torch.arange(C_real, device=device)[None, :]
    return (((c * I2 + n) if swap else (n * I2 + c)) * KK + k).reshape(-1)


def reduce64(part, nsplit, N, ntaps, Cx, N_real, C_real, swap, I2, KK, khw, n_grad):
    """(ref, bound, touched) over the n_grad elements of grad: the float64 sum of the slabs scattered by the index formula (0 elsewhere),
    the worst-case bound nsplit * 2^-24 * sum_s |part[s]| of any fp32 summation order, and the mask of the elements the launch writes."""
    p = part[:nsplit * N * ntaps * Cx].double().view(nsplit, N, ntaps, Cx)
    s, a = p.sum(0), p.abs().sum(0)
    ref = torch.zeros(n_grad, dtype=torch.float64, device=p.device)
    bound = torch.zeros_like(ref)
    touched = torch.zeros(n_grad, dtype=torch.bool, device=p.device)
    for t, k in enumerate(khw):
        if k < 0:
            continue
        o = reduce_index(N_real, C_real, swap, I2, KK, k, p.device)
        ref[o] = s[:N_real, t, :C_real].reshape(-1)
        bound[o] = nsplit * 2.0 ** -24 * a[:N_real, t, :C_real].reshape(-1)
        touched[o] = True
    return ref, bound, touched
