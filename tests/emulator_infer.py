"""TEST INFRASTRUCTURE: emulator statement of the inference epilogue.

`InferEmuOps` is tests.emulator.EmuOps plus gan_view_to_u8_hwc in torch, so `ResNetGenerator.forward_u8` / `inference.stylize_hwc`
run on the CPU.  Never imported by the product package.
"""
from __future__ import annotations

import torch

from tests.emulator import EmuOps


class InferEmuOps(EmuOps):
    def view_to_u8_hwc(self, src, Cr, dst):
        assert dst.dtype == torch.uint8 and tuple(dst.shape) == (src.B, src.H, src.W, Cr) and 1 <= Cr <= 4

        def op():
            v = src.nhwc().float()[..., :Cr]
            v = torch.where(torch.isnan(v), torch.full_like(v, -1.0), v)          # the library's contract: a NaN gives byte 0
            dst.copy_(v.clamp(-1, 1).mul(0.5).add(0.5).mul(255).round().byte())
        return op
