"""TEST INFRASTRUCTURE: float64 statement of torch.nn.utils.spectral_norm as csrc/spectral.hip applies it (one power iteration, sigma, the
weight gradient with u and v held constant), independent of the emulator.

Every quantity is stated from what it is computed from, so that a test can hold each kernel output to the statement AT THE VALUES THE
KERNEL WROTE for the quantities before it:  v = normalize(W^T u_in);  u = normalize(W v);  sigma = u . (W v);
dW = (G - (<G, W> / sigma) u v^T) / sigma  (single-matrix path: <G, W_sn> in place of <G, W> / sigma).  normalize(x) = x / max(||x||, eps).

`Ref` is the true statement; a subclass that overrides one of its attributes is a deliberately wrong one (tests/spectral_cases.py: WRONG).
"""
import torch

SN_RB, SN_CB = 32, 256          # the batched path's tile: rows, columns


class Ref:
    u_before_v = False            # u <- normalize(W v_in) first, v from that u
    sigma_old_u = False           # sigma = u_in . (W v)
    no_div_sigma = False          # dW = G - k u v^T
    swap_uv = False               # the projection on v u^T (square matrices)
    drop_last_tile = False        # <G, W> without the last tile of the batched grid
    drop_last_row_tile = False    # <G, W> without the last row of tiles
    acc_overwrites = False        # accumulate = 1 overwrites
    v_unnormalised = False        # v = W^T u
    eps_added = False             # x / (||x|| + eps)
    stale_snap = False            # the snapshots hold the u, v from before the power iteration


def normalize64(x, eps, ref=Ref):
    n = float(x.norm())
    return x / (n + eps) if ref.eps_added else x / max(n, eps)


def v64(W, u_in, v_in, eps, ref=Ref):
    if ref.u_before_v:
        return normalize64(W.t() @ normalize64(W @ v_in, eps, ref), eps, ref)
    t = W.t() @ u_in
    return t if ref.v_unnormalised else normalize64(t, eps, ref)


def u64(W, v, eps, ref=Ref):
    return normalize64(W @ v, eps, ref)


def sigma64(W, u_in, u, v, ref=Ref):
    return float(torch.dot(u_in if ref.sigma_old_u else u, W @ v))


def snap64(before, written, ref=Ref):
    return before if ref.stale_snap else written


def gw64(G, W, ref=Ref):
    """<G, W>"""
    P = G * W
    h, w = P.shape
    if ref.drop_last_row_tile:
        P = P[:((h - 1) // SN_RB) * SN_RB]
    elif ref.drop_last_tile:
        P = P.clone()
        P[((h - 1) // SN_RB) * SN_RB:, ((w - 1) // SN_CB) * SN_CB:] = 0
    return float(P.sum())


def dW64(G, k, u, v, sigma, prior=None, ref=Ref):
    """(G - k u v^T) / sigma (+ prior); k = <G, W> / sigma (batched) or <G, W_sn> (single matrix)"""
    outer = torch.outer(v, u) if ref.swap_uv else torch.outer(u, v)
    val = G - k * outer
    if not ref.no_div_sigma:
        val = val / sigma
    return val if (prior is None or ref.acc_overwrites) else prior + val


def module_step64(W, u, v, G, power_iter=True, eps=1e-12):
    """torch.nn.utils.spectral_norm's training-mode step and its weight gradient through float64 autograd -> (u, v, sigma, dW)"""
    W, u, v, G = (t.double() for t in (W, u, v, G))
    if power_iter:
        v = torch.nn.functional.normalize(W.t() @ u, dim=0, eps=eps)
        u = torch.nn.functional.normalize(W @ v, dim=0, eps=eps)
    sigma = torch.dot(u, W @ v)
    Wr = W.clone().requires_grad_(True)
    (Wr / torch.dot(u, Wr @ v) * G).sum().backward()        # u, v are constants of the backward
    return u, v, sigma, Wr.grad
