"""TEST INFRASTRUCTURE: emulator statement of the device PNG decoder's entries (csrc/pngdec.hip) as the stages of tests.pngdec_ref, over
the same upload block and the same workspace layout, so that dataio.PngDecoder, DeviceDecoder, ImageStore(device_png=True) and
stylize_folder(device_png=True) run on the CPU.  Never imported by the product package."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import torch

from gan_variant_research_amd import _lib
from tests import pngdec_ref as R
from tests.emulator_jpegdec import JpegDecEmuOps

IMG_BYTES, PAL_BYTES = C.sizeof(_lib.GanPngdecImage), 768
up256 = lambda v: -(-v // 256) * 256


def block_offsets(n: int):
    return n * IMG_BYTES, n * (IMG_BYTES + PAL_BYTES)


def read_block(blk: np.ndarray, n: int):
    """The descriptors of an upload block."""
    return (_lib.GanPngdecImage * n).from_buffer_copy(blk[:n * IMG_BYTES].tobytes())


def raw_bytes(im) -> int:
    return im.H * (1 + im.rowbytes)


class PngDecEmuOps(JpegDecEmuOps):
    def pngdec_block_offsets(self, n):
        assert 1 <= n <= 65535
        return block_offsets(n)

    def pngdec_bounds(self, imgs) -> int:
        o = up256(4 * len(imgs))
        for im in imgs:
            assert im.H >= 1 and im.W >= 1 and im.rowbytes <= _lib.PNGDEC_MAX_ROWBYTES and (im.color == 3 or im.depth == 8)
            im.raw_off, o = o, o + up256(raw_bytes(im))
        return o

    def _open_png(self, blk_dev, nbytes, n, ws):
        blk = blk_dev[:nbytes].numpy()
        imgs = read_block(blk, n)
        assert nbytes % 16 == 0 and ws.numel() >= imgs[n - 1].raw_off + raw_bytes(imgs[n - 1])
        return blk, imgs, ws.numpy(), ws.numpy()[:4 * n].view(np.int32)

    def pngdec_inflate(self, blk_dev, blk_host, nbytes, n, ws):
        blk, imgs, w, err = self._open_png(blk_dev, nbytes, n, ws)
        for i, im in enumerate(imgs):
            assert im.stream_off % 16 == 0 and im.stream_off + im.stream_len <= nbytes
            err[i] = 0
            try:
                raw = R.inflate(blk[im.stream_off:im.stream_off + im.stream_len].tobytes(), raw_bytes(im), im.wbits)
            except R.Flag as e:
                err[i] = e.bits
                continue
            w[im.raw_off:im.raw_off + len(raw)] = np.frombuffer(raw, np.uint8)

    def pngdec_pixels(self, blk_dev, blk_host, nbytes, n, ws, out, err_out):
        blk, imgs, w, err = self._open_png(blk_dev, nbytes, n, ws)
        o, o_pal = out.numpy(), block_offsets(n)[0]
        for i, im in enumerate(imgs):
            if err[i]:
                continue
            raw = w[im.raw_off:im.raw_off + raw_bytes(im)].tobytes()
            try:
                rows = R.unfilter(raw, im.H, im.rowbytes, im.bpp)
                if zlib.adler32(raw) != int.from_bytes(blk[im.stream_off + im.stream_len - 4:im.stream_off + im.stream_len].tobytes(), "big"):
                    raise R.Flag(R.ADLER)
            except R.Flag as e:
                err[i] = e.bits
                continue
            pal = blk[o_pal + PAL_BYTES * i:o_pal + PAL_BYTES * i + 3 * im.pal_count].tobytes()
            assert 0 <= im.out_off and im.out_off + im.H * im.W * 3 <= o.size
            o[im.out_off:im.out_off + im.H * im.W * 3] = R.to_rgb(rows, im.W, im.color, im.depth, pal).reshape(-1)
        err_out[:n] = torch.from_numpy(err.copy())
