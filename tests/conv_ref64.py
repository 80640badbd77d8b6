"""TEST INFRASTRUCTURE: the float64 statement of what one gan_conv_igemm launch leaves behind -- result, fused partials, chain sums --
and of gan_pack_weight, with the bounds a result is held to.  The convolution itself is tests/cases.conv_ref64 (unfold + matmul, checked
against float64 F.conv2d / F.conv_transpose2d / autograd by tests/test_conv_family_cpu.py); this module adds the epilogue.

EPILOGUE STATEMENT (include/mi355x_gan.h, gan_conv_desc).  With t = sum over taps and channels + bias[n] (the bias is added BEFORE the
activation; no bias: t is the sum):
    result = act(t) * f,      act in {identity, max(t, 0) with NaN kept, t > 0 ? t : 0.2 t, tanh},
    f = 1 without a mask, else (m > 0 ? 1 : 0.2) with m the mask element at the OUTPUT pixel, read through the mask's own halo:
        m = mask.padded[b, mask.halo + oy, mask.halo + ox, n], (oy, ox) the pixel of the output's interior -- for a phased store
        (oy, ox) = (2a + ry, 2b + rx).  m = 0 and m = -0.0 both give 0.2.
    stats_mode 0 (fused InstanceNorm partials): per (image, channel) sum t and sum t^2 of the UNROUNDED t over the image's output pixels
        (summed over all partials of the image: the tiling does not enter the statement);
    stats_mode 1 (backward chain): with g = the result ROUNDED to the output type (what the consumer reads) and y the operand at the
        output pixel of the padded domain, sum g [y > 0] and sum g y; the mask factor is then not applied.

BOUNDS (conventions of tests/cases.py: BOUND_C = 4, u = 2^-24).  Before the activation the error of t is the convolution's,
    e_t = BOUND_C sqrt(K) u A  (+ u |t| for the bias addition),    A = the same sum over |operands| (+ |bias|).
The activations are 1-Lipschitz, so e_t passes unchanged; LeakyReLU's product with the float 0.2f adds 2u |act| (the constant and the
product), tanhf is within 2 ulp (4u |tanh|, as tests/norm_cases.py grants it); the mask factor f scales all of that and, as the float 0.2f, adds 2u |ref|;
then the store, with |ref| = |act(t) f| the stored value's size:
    tol = e + u_out (|ref| + e),         e = f (e_t [+ 2u |act| | + 4u |act|]) [+ 2u |ref|]
The plain epilogue (no activation, no mask) is held to cases.derived_bound itself, u_out |ref| + BOUND_C sqrt(K) u A with the bias in A.
A sum over the n pixels of an image: every addend is off by at most its element bound, and n fp32 additions in any order add
BOUND_C sqrt(n) u sum|addend| (the form of dS in tests/norm_cases.py):
    tol(sum t)   = sum e_t          + BOUND_C sqrt(n) u sum|t|
    tol(sum t^2) = sum (2|t| e_t + e_t^2) + BOUND_C sqrt(n) u sum t^2          (t^2 is rounded once: inside the margin)
The chain sums are sums of the gradient the launch itself STORED (the statement is about the rounded gradient), read back bit for bit:
only the summation and the one product rounding remain,
    tol(sum g [y>0]) = BOUND_C sqrt(n) u sum|g| [y>0],      tol(sum g y) = (BOUND_C sqrt(n) + 1) u sum|g y|.
None of these is fitted to a result.
"""
import math

import torch

from tests.cases import BOUND_C, U_BF16, U_F32, conv_ref64, derived_bound

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
U = U_F32


def act64(t, act, slope=0.2):
    if act == ACT_RELU:
        return torch.where(t < 0, torch.zeros_like(t), t)           # a NaN passes, as torch.relu lets it
    if act == ACT_LRELU:
        return torch.where(t > 0, t, slope * t)
    if act == ACT_TANH:
        return torch.tanh(t)
    return t


def mask_factor64(m, slope=0.2):
    """LeakyReLU' from the saved activation: 1 where m > 0, else the slope (0 and -0.0 included)"""
    return torch.where(m > 0, torch.ones_like(m), torch.full_like(m, slope))


def layer64(op, g, w64, b64, src64, padded_domain=False):
    """(t, A, K): the pre-activation result of one direction of the layer `g` (tests/conv_cases.Geom) in float64 from the rounded operands,
    NCHW; b64: the bias (forward only) or None."""
    if op == "fwd":
        t, A, K = conv_ref64("fwd", g.k, g.s, g.p, g.tr, g.reflect, w64, x=src64)
        if b64 is not None:
            t, A = t + b64.view(1, -1, 1, 1), A + b64.abs().view(1, -1, 1, 1)
        return t, A, K
    assert b64 is None
    return conv_ref64("dgrad", g.k, g.s, g.p, g.tr, g.reflect, w64, dy=src64, x_hw=(g.H, g.W), padded_domain=padded_domain)


def epilogue64(t, act, mf=None, slope=0.2):
    r = act64(t, act, slope)
    return r if mf is None else r * mf


def elem_tol(t, A, K, act, mf, u_out, bias):
    """(tol of the stored result, e_t) per element; mf: the mask factor per element or None.  The plain epilogue gets
    cases.derived_bound unchanged.  |ref| is the stored value's, |act(t) mf|: the store term and the mask term are 0.2 of the unmasked
    ones where the mask is not positive, and the error of t reaches the result through the factor."""
    et = BOUND_C * math.sqrt(K) * U * A
    if act == ACT_NONE and mf is None:
        return derived_bound(t, A, K, u_out), et
    if bias:
        et = et + U * t.abs()
    r = act64(t, act).abs()
    e = et + (2 * U * r if act == ACT_LRELU else 4 * U * r if act == ACT_TANH else 0.0)
    if mf is not None:
        r = r * mf.abs()
        e = e * mf.abs() + 2 * U * r
    return e + u_out * (r + e), et


def sums_tol(t, et):
    """tolerances of (sum t, sum t^2) over the pixels of each (image, channel); t, et: (B, C, H, W)"""
    n = t.shape[2] * t.shape[3]
    k = BOUND_C * math.sqrt(n) * U
    return (et.sum((2, 3)) + k * t.abs().sum((2, 3)),
            (2 * t.abs() * et + et * et).sum((2, 3)) + k * (t * t).sum((2, 3)))


def chain_sums64(g, y):
    """(sum g [y > 0], sum g y) and their tolerances from the stored gradient g and the operand y, both (B, C, H, W) float64"""
    n = g.shape[2] * g.shape[3]
    k = BOUND_C * math.sqrt(n) * U
    pos = (y > 0).double()
    return ((g * pos).sum((2, 3)), (g * y).sum((2, 3)),
            k * (g.abs() * pos).sum((2, 3)), (k + U) * (g * y).abs().sum((2, 3)))


# ------------------------------------------------------------------------------------------------ gan_pack_weight
def pack64(src, Nw, ntaps, Cin, N_real, C_real, swap, I2, KK, khw, layout, scale=None):
    """dst[n][t][c] = src[(a * I2 + b) * KK + khw[t]] / scale, (a, b) = swap ? (c, n) : (n, c); 0 where n >= N_real, c >= C_real or
    khw[t] < 0.  layout 1: element (n, k = t * Cin + c) at (((n / 16) * (ntaps * Cin / 32) + k / 32) * 64 + ((k % 32) / 8) * 16 + n % 16) * 8 + k % 8.
    Returns the flat float64 copy in the destination's element order (the caller rounds it once to the destination type)."""
    s = src.reshape(-1).double()
    out = torch.zeros(Nw, ntaps, Cin, dtype=torch.float64)
    n_idx, c_idx = torch.arange(N_real)[:, None], torch.arange(C_real)[None, :]
    for t, k in enumerate(khw):
        if k < 0:
            continue
        o = ((c_idx * I2 + n_idx) if swap else (n_idx * I2 + c_idx)) * KK + k
        out[:N_real, t, :C_real] = s[o]
    if scale is not None:
        out = (out.float() / torch.tensor(scale, dtype=torch.float32)).double()     # one fp32 division, as W_sn = W / sigma rounds
    flat = out.reshape(-1)
    if layout == 1:
        K = ntaps * Cin
        n = torch.arange(Nw)[:, None].expand(Nw, K)
        k = torch.arange(K)[None, :].expand(Nw, K)
        pos = (((n // 16) * (K // 32) + k // 32) * 64 + ((k % 32) // 8) * 16 + n % 16) * 8 + k % 8
        res = torch.zeros(Nw * K, dtype=torch.float64)
        res[pos.reshape(-1)] = out.reshape(-1)
        flat = res
    return flat
