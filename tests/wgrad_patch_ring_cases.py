"""Shapes, seeded operands and runners shared by tools/make_golden_wgrad_patch.py (run once on the commit before the stage ring) and
tests/test_wgrad_patch_ring_gpu.py: the range-patch weight gradient (csrc/wgrad_patch.hip, csrc/wgrad_patch_fp8.hip) through
ConvLayer.wgrad / wgrad8, its partial slabs `part` [nsplit][N][9][Cx] and the reduced gradient [N][Cx][3][3]."""
import hashlib

import torch

from gan_variant_research_amd import BF16, FP8
from gan_variant_research_amd.convplan import ConvLayer
from gan_variant_research_amd.runtime import Ctx, HipOps

DEV = "cuda:0"

# (B, H, W, Cx, N): what each one reaches
SHAPES = [
    (2, 64, 64, 64, 128),      # 16 splits per image, 2 KM-pixel ranges per split
    (1, 64, 64, 256, 256),     # full tile grid, XCD remap
    (3, 32, 32, 64, 128),      # Wo = 32
    (4, 16, 16, 64, 128),      # Wo = 16
    (2, 20, 16, 64, 128),      # tail range, HoWo = 320
    (64, 16, 16, 256, 256),    # 2 images per split
    (1, 8, 128, 64, 128),      # the 128-pixel-wide kernel
]
FP8_SHAPES = [SHAPES[0], SHAPES[3], SHAPES[5]]
CASES = [("bf16", s) for s in SHAPES] + [("e4m3", s) for s in FP8_SHAPES]


def case_id(kind, shape):
    return kind + "-" + "x".join(str(v) for v in shape)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def operands(shape):
    """Seeded N(0,1): the padded input [B][H+2][W+2][Cx] (halo included) and the output gradient [B][H][W][N], as bf16 on the device."""
    B, H, W, Cx, N = shape
    g = torch.Generator().manual_seed(1000 + B + 3 * H + 5 * W + 7 * Cx + 11 * N)
    xp = torch.randn(B, H + 2, W + 2, Cx, generator=g).to(torch.bfloat16)
    dy = torch.randn(B, H, W, N, generator=g).to(torch.bfloat16)
    return xp.to(DEV), dy.to(DEV)


def run(kind, shape):
    """Runs the weight gradient of a 3x3 Cx -> N convolution once.  Returns a dict: part (fp32 [nsplit][N][9][Cx], a copy), grad (the reduced
    gradient, a copy), nsplit, and the operands the kernel multiplied as float64-exact tensors: xp [B][H+2][W+2][Cx], g [B][H][W][N] and the
    per-image scale [B] (ones for bf16)."""
    B, H, W, Cx, N = shape
    dev = torch.device(DEV)
    ctx = Ctx(HipOps(dev), dev, BF16)
    w = torch.zeros(N, Cx, 3, 3, device=dev)
    layer = ConvLayer(ctx, w, None, torch.zeros_like(w), None, 3, 1, 1)
    xp, g = operands(shape)
    x, dy = ctx.view(B, H, W, Cx, 1), ctx.view(B, H, W, N, 2)
    x.padded().copy_(xp)
    dy.nhwc().copy_(g)
    scale = torch.ones(B, device=dev)
    if kind == "bf16":
        ops = layer.wgrad(x, dy, False, bias_too=False)
    else:
        x8, dy8 = ctx.view(B, H, W, Cx, 1, dtype=FP8), ctx.view(B, H, W, N, 2, dtype=FP8)
        amax, scale = dy.nhwc().float().abs().amax((1, 2, 3)), torch.zeros(B, device=dev)
        for o in (ctx.ops.quantize_fp8(x, x8), ctx.ops.quantize_fp8_pow2(dy, dy8, amax, scale)):
            o()
        ops = layer.wgrad8(x8, dy8, scale, False, pow2=True)
        xp, g = x8.padded().view(torch.float8_e4m3fn).float(), dy8.nhwc().view(torch.float8_e4m3fn).float()
    call = ops[0].wgrad
    assert call.variant == 1, (kind, shape, call.variant)
    n = call.nsplit * N * 9 * Cx
    call.part[:n].fill_(float("nan"))          # every element of every slab must be written by the launch
    for o in ops:
        o()
    torch.cuda.synchronize()
    return {"part": call.part[:n].view(call.nsplit, N, 9, Cx).clone(), "grad": layer.grad_w.clone(), "nsplit": call.nsplit,
            "xp": xp.double(), "g": g.double(), "scale": scale.double()}


def ref64(r, absolute=False):
    """float64 on the device: out[n][kh*3+kw][c] = sum_b scale[b] sum_yx g[b,y,x,n] xp[b,y+kh,x+kw,c] (or the sum of the |products|)."""
    xp, g = r["xp"], r["g"]
    B, H, W, N = g.shape
    if absolute:
        xp, g = xp.abs(), g.abs()
    gs = (g * r["scale"].view(B, 1, 1, 1)).reshape(B * H * W, N)
    out = torch.empty(N, 9, xp.shape[-1], dtype=torch.float64, device=g.device)
    for kh in range(3):
        for kw in range(3):
            out[:, kh * 3 + kw, :] = gs.t() @ xp[:, kh:kh + H, kw:kw + W, :].reshape(B * H * W, -1)
    return out
