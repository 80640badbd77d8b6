"""TEST INFRASTRUCTURE: emulator statement of csrc/zip.hip.

`ZipEmuOps` is tests.emulator_jpeg.JpegEmuOps plus `jpeg_files_bounds`, `jpeg_files` and `crc32_ranges`, with zlib for the checksum and the
file layout written out from include/mi355x_gan.h, so that `inference.JpegEncoder.encode_block` and `stylize_folder(zip_path=...)` run on
the CPU.  Never imported by the product package."""
from __future__ import annotations

import zlib

import numpy as np
import torch

from tests.emulator_jpeg import JpegEmuOps


class ZipEmuOps(JpegEmuOps):
    def crc32_ranges(self, buf, offsets, crc, flag):
        def op():
            off, raw = offsets.tolist(), buf.numpy()
            for i in range(len(off) - 1):
                lo, hi = off[i], off[i + 1]
                if not 0 <= lo <= hi <= raw.size:
                    crc[i] = 0
                    flag[0] |= 1
                    continue
                crc[i] = int(np.uint32(zlib.crc32(raw[lo:hi].tobytes())).astype(np.int32))
        return op

    def jpeg_files_bounds(self, B, H, W, head_bytes, sos_bytes=14):
        return self.jpeg_bounds(B, H, W)[1] + B * (head_bytes + 4 * (5 + 16 + 256) + sos_bytes + 2)

    def jpeg_files(self, head, sos, dht, scan, scan_offsets, B, files, file_offsets, crc, flag):
        def op():
            h, s, d, sc, so = head.numpy().tobytes(), sos.numpy().tobytes(), dht.numpy().reshape(-1, 4, 272), scan.numpy(), scan_offsets.tolist()
            pos, bits = 0, 0
            for b in range(B):
                data = h
                for t, tc in enumerate((0x00, 0x10, 0x01, 0x11)):
                    n = min(int(d[b, t, :16].sum()), 256)
                    data += b"\xff\xc4" + (2 + 1 + 16 + n).to_bytes(2, "big") + bytes([tc]) + d[b, t, :16 + n].tobytes()
                lo, hi = so[b], so[b + 1]
                if not 0 <= lo <= hi <= sc.size:
                    bits |= 1
                    lo = hi = 0
                data += s + sc[lo:hi].tobytes() + b"\xff\xd9"
                if pos + len(data) > files.numel():
                    bits |= 2
                    data = data[:max(files.numel() - pos, 0)]
                file_offsets[b] = pos
                files[pos:pos + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8) if data else files[:0]
                crc[b] = int(np.uint32(zlib.crc32(data)).astype(np.int32))
                pos += len(data)
            file_offsets[B] = pos
            flag[0] = bits
        return op
