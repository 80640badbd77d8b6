"""TEST INFRASTRUCTURE: emulator statements of the fused trainer's discriminator-family entry points.

`DFamilyEmuOps` is tests.emulator.EmuOps plus gan_spectral_norm_batch_fwd / _bwd and the bf16 / fp32 operand copy packed with a
scale (gan_pack_desc.scale: dst = src / *scale), so the fused CutTrainer with several discriminator scales and spectral norm runs
on the CPU.  Never imported by the product package.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.emulator import EmuOps


class DFamilyEmuOps(EmuOps):
    def spectral_norm_batch_ws_floats(self, h, w):
        return 1

    def spectral_norm_batch_fwd(self, entries, power_iter, eps):
        entries = list(entries)

        def op():
            for e in entries:
                W, u, v = e["W"], e["u"], e["v"]
                m = W.reshape(W.shape[0], -1)
                if power_iter:
                    v.copy_(F.normalize(torch.mv(m.t(), u), dim=0, eps=eps))
                    u.copy_(F.normalize(torch.mv(m, v), dim=0, eps=eps))
                e["sigma"].fill_(float(torch.dot(u, torch.mv(m, v))))
                e["u_snap"].copy_(u)
                e["v_snap"].copy_(v)
        return op

    def spectral_norm_batch_bwd(self, entries, accumulate):
        entries = list(entries)

        def op():
            for e in entries:
                G, W, sg = e["G"], e["W"], e["sigma"]
                k = (G * W).sum() / sg
                val = (G.reshape(G.shape[0], -1) - k * torch.outer(e["u_snap"], e["v_snap"])).reshape(G.shape) / sg
                if accumulate:
                    e["dW"].add_(val)
                else:
                    e["dW"].copy_(val)
        return op

    def pack_weight(self, src, dst, dtype, Nw, ntaps, Cin, N_real, C_real, swap, I2, KK, khw, layout=0, scale=None):
        if scale is None or dtype == 2:
            return super().pack_weight(src, dst, dtype, Nw, ntaps, Cin, N_real, C_real, swap, I2, KK, khw, layout, scale)
        tmp = torch.zeros_like(src)
        inner = super().pack_weight(tmp, dst, dtype, Nw, ntaps, Cin, N_real, C_real, swap, I2, KK, khw, layout, None)

        def op():
            tmp.copy_(src / scale)
            inner()
        op.pack_args = (src, dst, dtype, Nw, ntaps, Cin, N_real, C_real, int(swap), I2, KK, khw, int(layout), scale)
        return op
