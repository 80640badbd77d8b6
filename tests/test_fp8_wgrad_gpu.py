"""e4m3 weight gradient of the residual convolutions (gan_conv_wgrad with dtype GAN_FP8, csrc/wgrad_patch_fp8.hip) on the GPU: the kernel
through the C ABI with e4m3 bytes and scales written by the test, then the fused CUT step with fp8_wgrad=True."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from gan_variant_research_amd import BF16, FP8                                     # noqa: E402
from gan_variant_research_amd._lib import GanError                                 # noqa: E402
from gan_variant_research_amd.convplan import ConvLayer                            # noqa: E402
from gan_variant_research_amd.runtime import HALO_REFLECT, HALO_ZERO, Ctx, HipOps  # noqa: E402
from tests import cases                                                            # noqa: E402
from tests import emulator_fp8wgrad as E                                           # noqa: E402

# (B, H = W, C): 16-pixel-wide maps (two image rows per 32-pixel read), 64-wide (256x256 images), 128-wide (512x512 images: row ring)
GEOMS = [(2, 16, 256), (16, 64, 256), (1, 128, 256), (8, 128, 256), (2, 16, 128)]


def hip_ctx():
    return Ctx(HipOps(torch.device(DEV)), DEV, BF16)


def e4m3_bytes(v):
    return v.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_values(b):
    return b.view(torch.float8_e4m3fn).float()


def setup(ctx, xb, gb, scale):
    """xb: uint8 [B][H+2][W+2][C] e4m3 bytes of the padded input; gb: uint8 [B][H][W][C] e4m3 bytes of the output gradient;
    scale: float [B] or None.  Returns (layer, ops, call)."""
    B, H, W, C_ = gb.shape
    w = torch.zeros(C_, C_, 3, 3, device=DEV)
    layer = ConvLayer(ctx, w, None, torch.full_like(w, 7.0), None, 3, 1, 1)
    x8 = ctx.view(B, H, W, C_, 1, dtype=FP8)
    g8 = ctx.view(B, H, W, C_, 2, dtype=FP8)
    x8.padded().copy_(xb.to(DEV))
    g8.t.zero_()
    g8.nhwc().copy_(gb.to(DEV))
    sc = None if scale is None else scale.float().to(DEV)
    ops = layer.wgrad8(x8, g8, sc, False)
    return layer, ops, ops[0].wgrad


def run(ops):
    for o in ops:
        o()
    torch.cuda.synchronize()


def ref64(xp, g, scale, absolute=False):
    """float64 on the device: out[n][c][kh][kw] = sum_b scale[b] sum_yx g[b,y,x,n] xp[b,y+kh,x+kw,c] (or the sum of |products|)."""
    B, H, W, N = g.shape
    xp, g = xp.to(DEV).double(), g.to(DEV).double()
    if absolute:
        xp, g = xp.abs(), g.abs()
    gs = (g * scale.to(DEV).double().view(B, 1, 1, 1)).reshape(B * H * W, N)
    out = torch.empty(N, xp.shape[-1], 3, 3, dtype=torch.float64, device=DEV)
    for kh in range(3):
        for kw in range(3):
            out[:, :, kh, kw] = gs.t() @ xp[:, kh:kh + H, kw:kw + W, :].reshape(B * H * W, -1)
    return out.cpu()


@pytest.mark.parametrize("geom", GEOMS)
def test_exact_small_integers(geom):
    """Operands from {0, +-0.5, +-1, +-2}, power-of-two image scales at most two bits apart: every partial and the reduced sum fit fp32's
    significand, so the result is independent of the summation order and must EQUAL the float64 one bit for bit."""
    B, H, C_ = geom
    g = torch.Generator().manual_seed(100 + B + H + C_)
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    xv = vals[torch.randint(0, 7, (B, H + 2, H + 2, C_), generator=g)]
    gv = vals[torch.randint(0, 7, (B, H, H, C_), generator=g)]
    scale = 2.0 ** -(3.0 + torch.arange(B) % 3)
    ctx = hip_ctx()
    layer, ops, call = setup(ctx, e4m3_bytes(xv), e4m3_bytes(gv), scale)
    assert call.x.dtype == FP8 and call.variant == 1 and call.nsplit % B == 0
    run(ops)
    want = ref64(xv, gv, scale)
    got = layer.grad_w.cpu().double()
    assert float(want.abs().max()) > 0
    assert torch.equal(got, want), (float((got - want).abs().max()), int((got != want).sum()))


@pytest.mark.parametrize("geom", GEOMS)
def test_random_e4m3_operands_fp32_accumulation_bound(geom):
    """Rounded Gaussians (ReLU'd for x), image scales 1e-3 / 3e-5: against float64 on the same dequantised operands, elementwise
    |got - ref| <= (K + nsplit) * 2^-24 * sum |products| -- products of two e4m3 values are exact in fp32, only the accumulation rounds."""
    B, H, C_ = geom
    g = torch.Generator().manual_seed(200 + B + H + C_)
    xb = e4m3_bytes(torch.randn(B, H + 2, H + 2, C_, generator=g).relu())
    gb = e4m3_bytes(torch.randn(B, H, H, C_, generator=g))
    scale = torch.tensor([1e-3, 3e-5]).repeat((B + 1) // 2)[:B]
    ctx = hip_ctx()
    layer, ops, call = setup(ctx, xb, gb, scale)
    run(ops)
    scale32 = scale.float()         # the kernel multiplies by the fp32 value
    want = ref64(e4m3_values(xb), e4m3_values(gb), scale32)
    bound = (B * H * H + call.nsplit) * 2.0 ** -24 * ref64(e4m3_values(xb), e4m3_values(gb), scale32, absolute=True)
    err = (layer.grad_w.cpu().double() - want).abs()
    print(f"geom {geom}: nsplit {call.nsplit}, max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3e}, rms of ref {float(want.pow(2).mean().sqrt()):.3e}")
    assert bool((err <= bound).all()), (float(err.max()), float(bound.min()))


@pytest.mark.parametrize("geom,relu", [((2, 16, 256), False), ((2, 16, 256), True), ((2, 64, 256), True), ((1, 128, 256), True)])
def test_against_unrounded_gradient(geom, relu):
    """bf16 x and dy through gan_quantize_fp8 (per-image amax for dy), e4m3 weight gradient against torch.nn.grad.conv2d_weight in float64
    on the UNROUNDED operands: rms error < 0.05 rms and max error < 0.3 rms of the exact gradient (the bounds cases.run_conv_fp8 states
    for the forward; exact arithmetic on e4m3-rounded operands gives 0.037-0.038 / 0.17-0.20)."""
    B, H, C_ = geom
    g = torch.Generator().manual_seed(300 + H)
    x = torch.randn(B, C_, H, H, generator=g)
    x = (x.relu() if relu else x).bfloat16().float()
    dy = (torch.randn(B, C_, H, H, generator=g) * torch.tensor([1e-3, 3e-5])[:B].view(B, 1, 1, 1)).bfloat16().float()
    ctx = hip_ctx()
    w = torch.zeros(C_, C_, 3, 3, device=DEV)
    layer = ConvLayer(ctx, w, None, torch.zeros_like(w), None, 3, 1, 1)
    xv, dyv = cases.to_view(ctx, x, 1, HALO_REFLECT), cases.to_view(ctx, dy, 2, HALO_ZERO)
    x8, dy8 = ctx.view(B, H, H, C_, 1, dtype=FP8), ctx.view(B, H, H, C_, 2, dtype=FP8)
    amax, scale = dy.abs().amax((1, 2, 3)).to(DEV), torch.zeros(B, device=DEV)
    run([ctx.ops.quantize_fp8(xv, x8), ctx.ops.quantize_fp8(dyv, dy8, amax, scale)] + layer.wgrad8(x8, dy8, scale, False))
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect").double()
    want = torch.nn.grad.conv2d_weight(xp, (C_, C_, 3, 3), dy.double())
    got = layer.grad_w.cpu().double()
    rms = float(want.pow(2).mean().sqrt())
    e_rms, e_max = float((got - want).pow(2).mean().sqrt()) / rms, float((got - want).abs().max()) / rms
    print(f"geom {geom} relu {relu}: rms error {e_rms:.4f} rms, max error {e_max:.4f} rms")
    assert e_rms < 0.05 and e_max < 0.3, (e_rms, e_max)


@pytest.mark.parametrize("geom", [(2, 16, 256), (16, 64, 256), (1, 128, 256)])
def test_two_runs_bit_identical(geom):
    B, H, C_ = geom
    g = torch.Generator().manual_seed(400 + H)
    xb = e4m3_bytes(torch.randn(B, H + 2, H + 2, C_, generator=g).relu())
    gb = e4m3_bytes(torch.randn(B, H, H, C_, generator=g))
    ctx = hip_ctx()
    layer, ops, call = setup(ctx, xb, gb, torch.tensor([1e-3, 3e-5]).repeat((B + 1) // 2)[:B])
    n = call.nsplit * call.N * call.ntaps * call.Cx
    run(ops)
    first = call.part[:n].clone()
    call.part[:n].fill_(float("nan"))
    run(ops)
    assert bool(torch.isfinite(first).all()) and torch.equal(first.view(torch.int32), call.part[:n].view(torch.int32))


def test_wrong_variant_or_split_count_is_an_error_and_launches_nothing():
    B, H, C_ = 2, 16, 256
    g = torch.Generator().manual_seed(5)
    xb = e4m3_bytes(torch.randn(B, H + 2, H + 2, C_, generator=g))
    gb = e4m3_bytes(torch.randn(B, H, H, C_, generator=g))
    ctx = hip_ctx()
    layer, ops, call = setup(ctx, xb, gb, None)
    good = (call.variant, call.nsplit)
    assert good[0] == 1 and good[1] == B * ctx.ops.wgrad_patch_splits(call)
    for variant, nsplit in ((0, good[1]), (2, good[1]), (1, good[1] + B), (1, 1)):
        call.variant, call.nsplit = variant, nsplit
        call.part = torch.full((max(nsplit, good[1]) * call.N * call.ntaps * call.Cx,), -3.0, device=DEV)
        with pytest.raises(GanError):
            ctx.ops.conv_wgrad(call)()
        torch.cuda.synchronize()
        assert bool((call.part == -3.0).all()), (variant, nsplit)
    call.variant, call.nsplit = good


# ---------------------------------------------------------------------- the fused CUT step
@pytest.mark.parametrize("S,B", [(64, 2), (512, 1)])
def test_cut_step_fp8_wgrad_vs_oracle(S, B):
    """One CUT step with fp8=True, fp8_wgrad=True against the fp32 oracle with the tolerances of the fp8 step tests (step-0 losses within
    8 %, every parameter within 2 lr + 5e-5 after the update).  At 512x512 the residual maps are 128 pixels wide: every e4m3 weight
    gradient is the row-ring instantiation (the only one that takes 128-wide maps)."""
    ops = HipOps(torch.device(DEV))
    tr, img, ref_img = E.run_cut_steps_fp8_wgrad(DEV, ops, S=S, B=B, nsteps=1, tol0=8e-2, ptol=4.5e-4, threads=16)
    assert tr.fp8 and tr.fp8_wgrad and tr.G.fp8_wgrad
    passes = [p for p in tr.G.passes if getattr(p, "wgrad8_layers", None)]      # the passes whose backward was planned
    assert sum(p.B for p in passes) == 3 * B       # G(photos), G(monets) (one merged pass of 2B or two of B) and the PatchNCE feature pass
    for p in passes:
        took = p.wgrad8_layers
        assert len(took) == 2 * min(9, p.last - 2) and all(took.values()), took
    if S == 512:
        for p in passes:
            for call in p.wgrad8_calls:
                assert call.Wo == 128 and call.variant == 1 and call.x.dtype == FP8      # 128-wide maps: the row-ring kernel
    assert float((img - ref_img).abs().max()) < 0.3 and float((img - ref_img).pow(2).mean().sqrt()) < 0.06


def test_block_gradients_vs_bf16_weight_gradient_within_the_format_error():
    """Residual-block weight gradients after one 64x64 step: fp8 + fp8_wgrad against fp8 (bf16 weight gradient), relative Frobenius
    difference per layer, on the GPU and on the emulator (exact arithmetic on the e4m3 bytes: what the number format alone causes).  The
    GPU's value may exceed the emulator's by at most half."""
    from tests.emulator_fp8wgrad import Fp8WgradEmuOps
    torch.set_num_threads(16)
    diffs = {}
    for name, dev, mk in (("gpu", DEV, lambda: HipOps(torch.device(DEV))), ("emu", "cpu", Fp8WgradEmuOps)):
        grads = []
        for w8 in (False, True):
            tr = E.make_trainer(dev, mk(), 64, 2, True, w8)
            E.run_steps(tr, 64, 2, 1, dev)
            if dev != "cpu":
                torch.cuda.synchronize()
            grads.append(E.block_grads(tr))
        diffs[name] = [E.rel_frobenius(a, b) for a, b in zip(grads[1], grads[0])]
    for i, (dg, de) in enumerate(zip(diffs["gpu"], diffs["emu"])):
        print(f"block {i // 2} conv {'ab'[i % 2]}: gpu {dg:.4f} emulator {de:.4f} ratio {dg / de:.3f}")
    assert len(diffs["gpu"]) == 18
    for i, (dg, de) in enumerate(zip(diffs["gpu"], diffs["emu"])):
        assert dg <= 1.5 * de, (i, dg, de)


def test_twenty_steps_stay_finite():
    """Twenty steps at 64x64, batch 2, fp8 + fp8_wgrad: every loss finite (the curves are printed next to the fp8 ones)."""
    curves = {}
    for w8 in (False, True):
        tr = E.make_trainer(DEV, HipOps(torch.device(DEV)), 64, 2, True, w8)
        curves[w8] = E.run_steps(tr, 64, 2, 20, DEV)
    for s, (a, b) in enumerate(zip(curves[False], curves[True])):
        print(f"step {s:2d} fp8 " + " ".join(f"{k}={v:.4f}" for k, v in a.items()) + " | fp8+wgrad " + " ".join(f"{k}={v:.4f}" for k, v in b.items()))
    assert all(np.isfinite(v) for l in curves[True] for v in l.values())
