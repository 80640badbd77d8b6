"""TEST INFRASTRUCTURE: emulator statement of the device JPEG encoder and of the inference input pipeline.

`JpegEmuOps` is tests.emulator_infer.InferEmuOps plus the three encoder ops as the stages of tests.jpeg_ref, so `inference.JpegEncoder`
and `stylize_folder(device_jpeg=True)` run on the CPU; `EmuInputPipeline` stands in for dataio.InputPipeline with PIL's own resize (which
the device pipeline equals bit for bit).  Never imported by the product package.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import jpeg_ref as R
from tests.emulator_infer import InferEmuOps


class JpegEmuOps(InferEmuOps):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._jpeg = {}          # workspace pointer -> per-image symbol lists (what the kernels keep as coefficients)

    def jpeg_bounds(self, B, H, W):
        assert B >= 1 and 1 <= H <= 65535 and 1 <= W <= 65535
        nblk = 3 * -(-H // 8) * -(-W // 8)
        return 256, 2 * B * nblk * 216

    def jpeg_blocks(self, rgb, quality, ws, hist):
        def op():
            syms = [R.block_symbols(R.coefficients(im.numpy(), quality)) for im in rgb]
            self._jpeg[ws.data_ptr()] = syms
            for b, s in enumerate(syms):
                hist[b].copy_(torch.from_numpy(R.histograms(s).astype(np.int32)))
        return op

    def jpeg_tables(self, hist, n, dht, codes):
        def op():
            h, d, c = hist.view(-1, 256), dht.view(-1, 272), codes.view(-1, 256)
            for t in range(n):
                bits, vals = R.optimal_table(h[t].tolist())
                code, size = R.canonical_codes(bits, vals)
                row = np.zeros(272, np.uint8)
                row[:16], row[16:16 + len(vals)] = bits[1:17], vals
                d[t].copy_(torch.from_numpy(row))
                c[t].copy_(torch.from_numpy(((size << 16) | code).astype(np.int32)))
        return op

    def jpeg_scan(self, ws, B, H, W, codes, out, offsets):
        def op():
            c = codes.view(-1, 4, 256).numpy().astype(np.int64)
            pos = 0
            for b, syms in enumerate(self._jpeg[ws.data_ptr()][:B]):
                scan = R.pad_and_stuff(*R.bit_string(syms, [(c[b, t] & 0xFFFF, c[b, t] >> 16) for t in range(4)]))
                offsets[b] = pos
                out[pos:pos + len(scan)] = torch.frombuffer(bytearray(scan), dtype=torch.uint8)
                pos += len(scan)
            offsets[B] = pos
        return op


class EmuInputPipeline:
    """dataio.InputPipeline for inference jobs (whole image -> S x S, no flip, no jitter) with PIL's resize and the host path's
    normalisation."""

    def __init__(self, image_size, device, max_batch=64, max_rows=1024, filter=2):
        self.S, self.device, self.max_batch, self.filter = image_size, torch.device(device), max_batch, filter

    def run(self, images, jobs, out=None):
        from PIL import Image
        S = self.S
        arr = np.stack([np.asarray(Image.fromarray(im.cpu().numpy()).resize((S, S), self.filter), dtype=np.float32) for im in images])
        return torch.from_numpy(arr).permute(0, 3, 1, 2).div(255.0).sub(0.5).div(0.5).contiguous()
