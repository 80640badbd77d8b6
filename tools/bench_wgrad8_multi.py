"""bf16 vs e4m3 weight gradient of the residual 3x3 256->256 convolution on many small maps (Basic_GAN at 64x64: 16x16 maps), where a
split covers several whole images: python tools/bench_wgrad8_multi.py [B] [H] [iters].  One launch each per iteration on real (random,
non-zero) operands; the e4m3 copy of the output gradient carries power-of-two scales (quantize_fp8_pow2) and the call the promise.  Prints
HIP-event times; under `rocprofv3 --kernel-trace --stats -- python ...` the kernel table gives the per-launch durations of
wgrad_patch_kernel<4> (bf16, several images per split) and wgrad_patch_fp8_kernel<false, true>."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_variant_research_amd import BF16, FP8
from gan_variant_research_amd.convplan import ConvLayer
from gan_variant_research_amd.runtime import Ctx, HipOps

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
H = int(sys.argv[2]) if len(sys.argv) > 2 else 16
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ctx = Ctx(HipOps(dev), dev, BF16)
w = torch.zeros(256, 256, 3, 3, device=dev)
layer = ConvLayer(ctx, w, None, torch.zeros_like(w), None, 3, 1, 1)
x = ctx.view(B, H, H, 256, 1); x.t.normal_().relu_()
dy = ctx.view(B, H, H, 256, 2); dy.nhwc().normal_()
dy.nhwc().mul_(torch.logspace(-5, -3, B, device=dev).view(B, 1, 1, 1).to(dy.t.dtype))      # per-image magnitudes as in a backward pass
x8, dy8 = ctx.view(B, H, H, 256, 1, dtype=FP8), ctx.view(B, H, H, 256, 2, dtype=FP8)
amax, scale = dy.nhwc().float().abs().amax((1, 2, 3)).contiguous(), torch.zeros(B, device=dev)
for o in (ctx.ops.quantize_fp8(x, x8), ctx.ops.quantize_fp8_pow2(dy, dy8, amax, scale)):
    o()
w16, w8 = layer.wgrad(x, dy, False, bias_too=False), layer.wgrad8(x8, dy8, scale, False, pow2=True)
flop = 2.0 * B * H * H * 256 * 256 * 9
print(f"wgrad 3x3 256->256, B={B}, {H}x{H}: {flop/1e9:.1f} GFLOP; splits bf16 {w16[0].wgrad.nsplit}, e4m3 {w8[0].wgrad.nsplit}")
for name, ops in (("bf16 wgrad_patch", w16[:1]), ("e4m3 wgrad_patch_fp8 multi", w8[:1]), ("wgrad_reduce (shared)", w8[1:])):
    for _ in range(3):
        for o in ops: o()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        for o in ops: o()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / iters * 1e3
    print(f"{name:28s} {us:8.1f} us" + (f"  {flop/us/1e6:8.1f} TFLOP/s" if "reduce" not in name else ""))
