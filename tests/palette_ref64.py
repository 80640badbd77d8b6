"""TEST INFRASTRUCTURE: the palette prior (csrc/palette.hip) stated in float64 (or, with dtype=torch.float32, the same statement in
fp32: the yardstick of the tolerance in tests/palette_cases.py).

Statistic (the reference's, GAN_Variant1/dataio/transforms.py:52-119): v = clamp(x / 2 + 1 / 2, 0, 1); sRGB linearisation; XYZ with the
reference's matrix over its white point; f(t); L, a, b; adaptive average pooling to T x T; mean and unbiased standard deviation of the
T*T cells per image and channel.  Loss (this project's): mean over images and channels of (|m - m_prior| + |s - s_prior|) / 100.
Gradient: analytic, with the derivative of the branch taken at every `where` and clamp passing on [0, 1] inclusive -- never autograd
through torch.where, whose untaken branch contributes 0 * inf at a saturated pixel.
"""
import torch

M = ((0.4124, 0.3576, 0.1805), (0.2126, 0.7152, 0.0722), (0.0193, 0.1192, 0.9505))
WHITE = (0.95047, 1.0, 1.08883)
EPS, KAPPA, LIN_T = 0.008856, 903.3, 0.04045


def pool_matrix(n, T, dtype=torch.float64):
    """(T, n): row i averages pixels floor(i n / T) .. ceil((i + 1) n / T) - 1."""
    P = torch.zeros(T, n, dtype=dtype)
    for i in range(T):
        lo, hi = (i * n) // T, -((-(i + 1) * n) // T)
        P[i, lo:hi] = 1.0 / (hi - lo)
    return P


def _chain(x, dtype):
    """-> Lab (B,3,H,W) and the pieces the gradient needs"""
    x = x.to(dtype)
    t = x * 0.5 + 0.5
    inside = (t >= 0) & (t <= 1)
    v = torch.where(t < 0, torch.zeros_like(t), torch.where(t > 1, torch.ones_like(t), t))      # keeps a NaN
    hi = v > LIN_T
    u = (v + 0.055) / 1.055
    lin = torch.where(hi, u.clamp_min(0.05) ** 2.4, v / 12.92)
    lin = torch.where(torch.isnan(v), v, lin)
    dlin = torch.where(hi, 2.4 / 1.055 * u.clamp_min(0.05) ** 1.4, torch.full_like(v, 1 / 12.92))
    mat = torch.tensor(M, dtype=dtype)
    white = torch.tensor(WHITE, dtype=dtype).view(1, 3, 1, 1)
    xyz = torch.einsum("kc,bchw->bkhw", mat, lin) / white
    big = xyz > EPS
    cb = xyz.clamp_min(EPS).pow(1.0 / 3.0)
    f = torch.where(big, cb, (KAPPA * xyz + 16.0) / 116.0)
    f = torch.where(torch.isnan(xyz), xyz, f)
    df = torch.where(big, 1.0 / (3.0 * cb * cb), torch.full_like(xyz, KAPPA / 116.0))
    lab = torch.stack([116.0 * f[:, 1] - 16.0, 500.0 * (f[:, 0] - f[:, 1]), 200.0 * (f[:, 1] - f[:, 2])], 1)
    return lab, inside, dlin, df, mat, white


def lab(x, dtype=torch.float64):
    return _chain(x, dtype)[0]


def cells(x, T, dtype=torch.float64):
    """(B, 3, T, T)"""
    L = lab(x, dtype)
    return torch.einsum("ih,bchw,jw->bcij", pool_matrix(x.shape[2], T, dtype), L, pool_matrix(x.shape[3], T, dtype))


def stats(x, T, dtype=torch.float64):
    """-> mean (B,3), std (B,3) (unbiased)"""
    if T < 2:
        raise ValueError("low_freq_size must be >= 2")
    c = cells(x, T, dtype).flatten(2)
    m = c.mean(2)
    s = ((c - m.unsqueeze(2)) ** 2).sum(2).div(c.shape[2] - 1).sqrt()
    return m, s


def loss_from_stats(m, s, pm, ps):
    return ((m - pm).abs() + (s - ps).abs()).sum() / (100.0 * m.numel())


def loss(x, T, pm, ps, dtype=torch.float64):
    m, s = stats(x, T, dtype)
    return loss_from_stats(m, s, pm.to(dtype), ps.to(dtype))


def grad(x, T, pm, ps, dtype=torch.float64):
    """dLoss/dx (B,3,H,W), analytic"""
    L, inside, dlin, df, mat, white = _chain(x, dtype)
    Ph, Pw = pool_matrix(x.shape[2], T, dtype), pool_matrix(x.shape[3], T, dtype)
    c = torch.einsum("ih,bchw,jw->bcij", Ph, L, Pw)
    N = T * T
    m = c.flatten(2).mean(2)
    s = ((c.flatten(2) - m.unsqueeze(2)) ** 2).sum(2).div(N - 1).sqrt()
    k = 1.0 / (100.0 * m.numel())
    gm, gs = torch.sign(m - pm.to(dtype)) * k, torch.sign(s - ps.to(dtype)) * k
    coef = torch.where(s > 0, gs / ((N - 1) * torch.where(s > 0, s, torch.ones_like(s))), torch.zeros_like(s))
    gc = gm.view(*gm.shape, 1, 1) / N + coef.view(*coef.shape, 1, 1) * (c - m.view(*m.shape, 1, 1))
    gl = torch.einsum("ih,bcij,jw->bchw", Ph, gc, Pw)                       # every cell's gradient over its pixels, / area
    gf = torch.stack([500.0 * gl[:, 1], 116.0 * gl[:, 0] - 500.0 * gl[:, 1] + 200.0 * gl[:, 2], -200.0 * gl[:, 2]], 1)
    gxyz = gf * df / white
    glin = torch.einsum("kc,bkhw->bchw", mat, gxyz)
    return 0.5 * inside.to(dtype) * dlin * glin


def batch_prior(monets, T, dtype=torch.float64):
    """The six batch means (mean[3], std[3]) of a Monet batch."""
    m, s = stats(monets, T, dtype)
    return m.mean(0), s.mean(0)


def ema(prior, batch, first, use_ema, decay):
    return batch if (first or not use_ema) else decay * prior + (1 - decay) * batch
