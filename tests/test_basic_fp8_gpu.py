"""fp8 mode of the fused CycleGAN trainer on the GPU: the e4m3 weight gradient over several images per split (gan_conv_wgrad with dtype
GAN_FP8 and g_scale_pow2, csrc/wgrad_patch_fp8.hip) through the C ABI, the power-of-two quantiser (gan_quantize_fp8_pow2) against its
emulator statement, iterations of basic.CycleGANTrainer(fp8=True, fp8_wgrad=True), and the bit-equality of the trainer with the switches
off to the commit before they existed."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from gan_variant_research_amd import BF16, F32, FP8                                # noqa: E402
from gan_variant_research_amd._lib import GanError                                 # noqa: E402
from gan_variant_research_amd.convplan import ConvLayer                            # noqa: E402
from gan_variant_research_amd.runtime import Ctx, HipOps                           # noqa: E402
from tests import emulator_basic_fp8 as E                                          # noqa: E402
from tests.emulator_basic_fp8 import BasicFp8EmuOps                                # noqa: E402

PARENT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "basic_fp8_parent_gpu.json")

# (B, H = W, C), all with the promise set.  The set the feature was specified with named (48, 16, 256) and (64, 16, 128); neither groups
# images (48 * 8 blocks / 256 and 64 * 2 blocks / 256 round down to one image per split), so they are replaced by the nearest geometries of
# the same kind that do: a batch that is no power of two, (96, 16, 256) -> 3 images per split, and 128 channels, (512, 16, 128) -> 4.
GEOMS = [(64, 16, 256), (256, 16, 256), (96, 16, 256), (512, 16, 128)]
IMAGES_PER_SPLIT = {(64, 16, 256): 2, (256, 16, 256): 8, (96, 16, 256): 3, (512, 16, 128): 4}


def hip_ctx(dtype=BF16):
    return Ctx(HipOps(torch.device(DEV)), DEV, dtype)


def e4m3_bytes(v):
    return v.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_values(b):
    return b.view(torch.float8_e4m3fn).float()


def setup(ctx, xb, gb, scale, pow2=True):
    """xb: uint8 [B][H+2][W+2][C] e4m3 bytes of the padded input; gb: uint8 [B][H][W][C] e4m3 bytes of the output gradient; scale: float [B].
    Returns (layer, ops, call) of ConvLayer.wgrad8 with the power-of-two promise."""
    B, H, W, C_ = gb.shape
    w = torch.zeros(C_, C_, 3, 3, device=DEV)
    layer = ConvLayer(ctx, w, None, torch.full_like(w, 7.0), None, 3, 1, 1)
    x8 = ctx.view(B, H, W, C_, 1, dtype=FP8)
    g8 = ctx.view(B, H, W, C_, 2, dtype=FP8)
    x8.padded().copy_(xb.to(DEV))
    g8.t.zero_()
    g8.nhwc().copy_(gb.to(DEV))
    ops = layer.wgrad8(x8, g8, scale.float().to(DEV), False, pow2=pow2)
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


def random_operands(geom, seed):
    B, H, C_ = geom
    g = torch.Generator().manual_seed(seed + B + H + C_)
    xb = e4m3_bytes(torch.randn(B, H + 2, H + 2, C_, generator=g).relu())
    gb = e4m3_bytes(torch.randn(B, H, H, C_, generator=g))
    scale = 2.0 ** -(10.0 + torch.arange(B) % 6)            # powers of two spread over 2^-10 .. 2^-15, different inside every split
    return xb, gb, scale


# ---------------------------------------------------------------------- the kernel through the C ABI
@pytest.mark.parametrize("geom", GEOMS)
def test_every_geometry_groups_images(geom):
    """The planner answers -(images per split) for every geometry of the set, and wgrad8 plans nsplit = B / that < B."""
    B, H, C_ = geom
    ctx = hip_ctx()
    xb, gb, scale = random_operands(geom, 0)
    layer, ops, call = setup(ctx, xb, gb, scale)
    k = IMAGES_PER_SPLIT[geom]
    assert ctx.ops.wgrad_patch_splits(call) == -k == BasicFp8EmuOps().wgrad_patch_splits(call)
    assert call.nsplit == B // k < B and call.variant == 1 and call.x.dtype == FP8 and call.g_scale_pow2 is True
    call.g_scale_pow2 = None
    assert ctx.ops.wgrad_patch_splits(call) == 0          # without the promise: the bf16 kernel keeps the launch
    call.g_scale_pow2 = True


@pytest.mark.parametrize("geom", GEOMS)
def test_exact_small_integers_scales_differ_inside_a_split(geom):
    """Operands from {0, +-0.5, +-1, +-2}; power-of-two image scales 2^-3, 2^-4, 2^-5 by image index modulo 3, so the images of one split
    (2, 8, 3 or 4 consecutive ones) carry different scales, at most two bits apart.  Every partial and the reduced sum fit fp32's
    significand, so the result must EQUAL the float64 one bit for bit; a scale applied per split instead of per image cannot."""
    B, H, C_ = geom
    g = torch.Generator().manual_seed(100 + B + H + C_)
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    xv = vals[torch.randint(0, 7, (B, H + 2, H + 2, C_), generator=g)]
    gv = vals[torch.randint(0, 7, (B, H, H, C_), generator=g)]
    scale = 2.0 ** -(3.0 + torch.arange(B) % 3)
    ctx = hip_ctx()
    layer, ops, call = setup(ctx, e4m3_bytes(xv), e4m3_bytes(gv), scale)
    k = B // call.nsplit
    assert k == IMAGES_PER_SPLIT[geom] and all(len(set(scale[s * k:(s + 1) * k].tolist())) > 1 for s in range(call.nsplit))
    run(ops)
    want = ref64(xv, gv, scale)
    got = layer.grad_w.cpu().double()
    assert float(want.abs().max()) > 0
    assert torch.equal(got, want), (float((got - want).abs().max()), int((got != want).sum()))
    # the same data with one scale per SPLIT (its first image's) is a different result: the check above can tell the two apart
    per_split = scale.view(call.nsplit, k)[:, :1].expand(call.nsplit, k).reshape(B)
    assert not torch.equal(ref64(xv, gv, per_split), want)


@pytest.mark.parametrize("geom", GEOMS)
def test_random_e4m3_operands_fp32_accumulation_bound(geom):
    """Rounded Gaussians (ReLU'd for x), power-of-two image scales spread over 2^-10 .. 2^-15: against float64 on the same dequantised
    operands, elementwise |got - ref| <= (K + nsplit) * 2^-24 * sum |products| (the bound of test_fp8_wgrad_gpu's test of the same name:
    products of two e4m3 values and their power-of-two scaling are exact in fp32, only the accumulation rounds)."""
    B, H, C_ = geom
    xb, gb, scale = random_operands(geom, 200)
    ctx = hip_ctx()
    layer, ops, call = setup(ctx, xb, gb, scale)
    run(ops)
    want = ref64(e4m3_values(xb), e4m3_values(gb), scale)
    bound = (B * H * H + call.nsplit) * 2.0 ** -24 * ref64(e4m3_values(xb), e4m3_values(gb), scale, absolute=True)
    err = (layer.grad_w.cpu().double() - want).abs()
    print(f"geom {geom}: nsplit {call.nsplit}, max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3e}, rms of ref {float(want.pow(2).mean().sqrt()):.3e}")
    assert bool((err <= bound).all()), (float(err.max()), float(bound.min()))


@pytest.mark.parametrize("geom", GEOMS)
def test_two_runs_bit_identical(geom):
    xb, gb, scale = random_operands(geom, 400)
    ctx = hip_ctx()
    layer, ops, call = setup(ctx, xb, gb, scale)
    n = call.nsplit * call.N * call.ntaps * call.Cx
    run(ops)
    first = call.part[:n].clone()
    call.part[:n].fill_(float("nan"))
    run(ops)
    assert bool(torch.isfinite(first).all()) and torch.equal(first.view(torch.int32), call.part[:n].view(torch.int32))


def test_wrong_split_count_or_missing_promise_is_an_error_and_launches_nothing():
    geom = (64, 16, 256)
    B = geom[0]
    xb, gb, scale = random_operands(geom, 5)
    ctx = hip_ctx()
    layer, ops, call = setup(ctx, xb, gb, scale)
    good = call.nsplit
    assert good == B // 2 and call.g_scale_pow2 is True
    for nsplit, pow2 in ((B, True), (good // 2, True), (good + 1, True), (0, True), (good, None), (good, False)):
        call.nsplit, call.g_scale_pow2 = nsplit, pow2
        call.part = torch.full((max(nsplit, good) * call.N * call.ntaps * call.Cx,), -3.0, device=DEV)
        with pytest.raises(GanError):
            ctx.ops.conv_wgrad(call)()
        torch.cuda.synchronize()
        assert bool((call.part == -3.0).all()), (nsplit, pow2)
    call.nsplit, call.g_scale_pow2 = good, True


# ---------------------------------------------------------------------- the quantiser
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_pow2_quantiser_equals_its_emulator_statement(dtype):
    """gan_quantize_fp8_pow2 on a bf16 and on an fp32 source: scales and e4m3 bytes equal BasicFp8EmuOps.quantize_fp8_pow2's bit for bit
    (amax values around the 1.75 * 2^e boundary, tiny, large and zero images included)."""
    B, H, C_ = 12, 16, 64
    g = torch.Generator().manual_seed(11)
    mag = torch.tensor([1.0, 448.0, 447.0, 449.0, 1.75, 1.7578125, 3e-5, 7e-9, 6e4, 0.0, 2.0 ** -20, 0.013])
    v = torch.randn(B, H + 4, H + 4, C_, generator=g).clamp(-1, 1) * mag.view(B, 1, 1, 1)
    v[:, 3, 3, 0] = mag                                      # the image's amax is exactly `mag`
    tdt = torch.bfloat16 if dtype == BF16 else torch.float32
    v = v.to(tdt)
    out = {}
    for name, dev, ops in (("gpu", DEV, HipOps(torch.device(DEV))), ("emu", "cpu", BasicFp8EmuOps())):
        ctx = Ctx(ops, dev if name == "gpu" else torch.device("cpu"), dtype)
        src, dst = ctx.view(B, H, H, C_, 2), ctx.view(B, H, H, C_, 2, dtype=FP8)
        src.padded().copy_(v.to(dev))
        amax = src.padded().float().abs().amax((1, 2, 3)).contiguous()
        sc = ctx.f32(B)
        ops.quantize_fp8_pow2(src, dst, amax, sc)()
        if name == "gpu":
            torch.cuda.synchronize()
        out[name] = (amax.cpu(), sc.cpu(), dst.padded().cpu().clone())
    assert torch.equal(out["gpu"][0], out["emu"][0])
    print("amax:", out["gpu"][0].tolist(), "\nscale:", out["gpu"][1].tolist())
    assert torch.equal(out["gpu"][1].view(torch.int32), out["emu"][1].view(torch.int32))
    assert torch.equal(out["gpu"][2], out["emu"][2]), int((out["gpu"][2] != out["emu"][2]).sum())
    sc, am = out["gpu"][1].double(), out["gpu"][0].double()
    nz = am > 0
    assert bool((torch.frexp(sc)[0] == 0.5).all()) and bool((am[nz] / 448 <= sc[nz]).all()) and bool((sc[nz] < 2 * am[nz] / 448).all())
    assert float(sc[9]) == 1.0


# ---------------------------------------------------------------------- the fused CycleGAN iteration
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_switches_off_iteration_equals_the_parents_to_the_bit(mode):
    """One iteration at 32x32, batch 2 with both switches off: the three losses and every optimiser's parameter block equal, bit for bit,
    what the commit before the switches existed computed -- tests/golden/basic_fp8_parent_gpu.json, recorded ON that commit on an MI355X
    by tools/make_golden_basic_fp8.py (float.hex() of the losses, SHA-256 of the parameter blocks)."""
    want = json.load(open(PARENT))[mode]
    tr = E.make_trainer(DEV, HipOps(torch.device(DEV)), 32, 2, amp=mode == "bf16")
    a, b = E.inputs(32, 2)
    losses = tr.train_iteration(a.to(DEV), b.to(DEV))
    torch.cuda.synchronize()
    got = E.state_digest(tr, losses)
    print(mode, {k: float.fromhex(v) for k, v in got["losses"].items()}, {k: float.fromhex(v) for k, v in want["losses"].items()})
    assert got == want


@pytest.mark.parametrize("S,B", [(64, 2), (256, 1)])
def test_iteration_fp8_wgrad_vs_oracle(S, B):
    """One iteration with fp8=True, fp8_wgrad=True against the fp32 oracle with the tolerances of the project's fp8 step tests
    (iteration-0 losses within 8 %, every parameter within 2 lr + 5e-5 after the update); all 18 residual layers of all six passes on
    the e4m3 weight gradient."""
    tr, got, ref = E.run_iteration_vs_oracle(DEV, HipOps(torch.device(DEV)), S, B, True, True, tol0=8e-2, ptol=4.5e-4, threads=16)
    assert tr.fp8 and tr.fp8_wgrad
    for name, p in E.generator_passes(tr):
        assert len(p.wgrad8_layers) == 18 and all(p.wgrad8_layers.values()), (name, p.wgrad8_layers)
        assert all(c.x.dtype == FP8 and c.variant == 1 and c.g_scale_pow2 for c in p.wgrad8_calls)


def test_block_gradients_vs_bf16_weight_gradient_within_the_format_error():
    """Residual weight gradients of both generators after one 64x64, batch 2 iteration: fp8 + fp8_wgrad against fp8 (bf16 weight
    gradient), relative Frobenius difference per layer, on the GPU and on the emulator (exact arithmetic on the e4m3 bytes: what the number
    format alone causes).  The GPU's value may exceed the emulator's by at most half (the margin of the CUT trainer's test)."""
    torch.set_num_threads(16)
    diffs = {}
    a, b = E.inputs(64, 2)
    for name, dev, mk in (("gpu", DEV, lambda: HipOps(torch.device(DEV))), ("emu", "cpu", BasicFp8EmuOps)):
        grads = []
        for w8 in (False, True):
            tr = E.make_trainer(dev, mk(), 64, 2, True, True, w8)
            tr.train_iteration(a.to(dev), b.to(dev))
            if dev != "cpu":
                torch.cuda.synchronize()
            grads.append(E.block_grads(tr))
        diffs[name] = [E.rel_frobenius(x, y) for x, y in zip(grads[1], grads[0])]
    for i, (dg, de) in enumerate(zip(diffs["gpu"], diffs["emu"])):
        print(f"{'G_A2B' if i < 18 else 'G_B2A'} block {i % 18 // 2} conv {'ab'[i % 2]}: gpu {dg:.4f} emulator {de:.4f} ratio {dg / de:.3f}")
    assert len(diffs["gpu"]) == 36
    for i, (dg, de) in enumerate(zip(diffs["gpu"], diffs["emu"])):
        assert 0 < dg <= 1.5 * de, (i, dg, de)


def test_batch_64_every_residual_weight_gradient_is_a_multi_image_e4m3_launch():
    """One iteration at 64x64, batch 64 -- the smallest batch whose 16x16 residual maps group images (2 per split): every residual weight
    gradient of the six passes is an e4m3 launch with nsplit = 32 < B, the losses are finite, and every parameter is within
    2 lr + 5e-5 of the bf16 trainer's after the update (both are this project's own paths on the same data; after one Adam step from
    zero moments a parameter moves by at most lr, so two paths differ by at most 2 lr plus rounding)."""
    S, B = 64, 64
    a, b = E.inputs(S, B)
    res = {}
    for name, fp8 in (("bf16", False), ("fp8", True)):
        tr = E.make_trainer(DEV, HipOps(torch.device(DEV)), S, B, True, fp8, fp8)
        losses = tr.train_iteration(a.to(DEV), b.to(DEV))
        torch.cuda.synchronize()
        res[name] = (losses, [o.flat_p.detach().cpu().clone() for o in (tr.opt_G, tr.opt_DA, tr.opt_DB)])
        print(name, losses)
        if fp8:
            for pname, p in E.generator_passes(tr):
                assert len(p.wgrad8_layers) == 18 and all(p.wgrad8_layers.values()), (pname, p.wgrad8_layers)
                assert len(p.wgrad8_calls) == 18
                for c in p.wgrad8_calls:
                    assert c.x.dtype == FP8 and c.variant == 1 and c.g_scale_pow2 and c.B == B and c.nsplit == B // 2
        del tr
    assert all(np.isfinite(v) for v in res["fp8"][0].values()), res["fp8"][0]
    worst = [float((x - y).abs().max()) for x, y in zip(res["fp8"][1], res["bf16"][1])]
    print("max |parameter(fp8 + fp8_wgrad) - parameter(bf16)| after the update: G %.3e D_A %.3e D_B %.3e (tol 4.5e-4)" % tuple(worst))
    assert all(w <= 4.5e-4 for w in worst), worst


def test_batch_256_the_benchmark_configuration_runs_8_images_per_split():
    """BASELINE configs[1], 64x64 at batch 256, with fp8 + fp8_wgrad: the trainer builds (the e4m3 input gradient's 18x18 padded domain
    qualifies for the e4m3 convolution kernel at any batch), every residual weight gradient of the six passes is an e4m3 launch of 8 images
    per split, and two iterations give finite losses."""
    S, B = 64, 256
    tr = E.make_trainer(DEV, HipOps(torch.device(DEV)), S, B, True, True, True)
    for pname, p in E.generator_passes(tr):
        assert len(p.wgrad8_layers) == 18 and all(p.wgrad8_layers.values()), (pname, p.wgrad8_layers)
        assert all(c.x.dtype == FP8 and c.variant == 1 and c.g_scale_pow2 and c.B == B and c.nsplit == B // 8 for c in p.wgrad8_calls)
    a, b = E.inputs(S, B)
    for _ in range(2):
        losses = tr.train_iteration(a.to(DEV), b.to(DEV))
        print("64x64 batch 256 fp8 + fp8_wgrad:", losses)
        assert all(np.isfinite(v) for v in losses.values()), losses


def test_twenty_iterations_stay_finite():
    """Twenty iterations at 64x64, batch 2, fp8 + fp8_wgrad: every loss finite (the curves are printed next to the fp8 ones)."""
    curves = {}
    a, b = E.inputs(64, 2)
    for w8 in (False, True):
        tr = E.make_trainer(DEV, HipOps(torch.device(DEV)), 64, 2, True, True, w8)
        curves[w8] = [tr.train_iteration(a.to(DEV), b.to(DEV)) for _ in range(20)]
    for s, (x, y) in enumerate(zip(curves[False], curves[True])):
        print(f"iteration {s:2d} fp8 " + " ".join(f"{k}={v:.4f}" for k, v in x.items()) + " | fp8+wgrad " + " ".join(f"{k}={v:.4f}" for k, v in y.items()))
    assert all(np.isfinite(v) for l in curves[True] for v in l.values())
