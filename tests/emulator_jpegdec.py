"""TEST INFRASTRUCTURE: emulator statement of the device JPEG decoder's entries (csrc/jpegdec.hip) as the stages of tests.jpegdec_ref,
over the same upload block and the same workspace layout, so that dataio.JpegDecoder, ImageStore(device_decode=True) and
stylize_folder(device_decode=True) run on the CPU.  Never imported by the product package."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from gan_variant_research_amd import _lib
from tests import jpegdec_ref as R
from tests.emulator_jpeg import JpegEmuOps

TABLE_BYTES, IMG_BYTES, SEG_BYTES = 1424, C.sizeof(_lib.GanJpegdecImage), C.sizeof(_lib.GanJpegdecSegment)
ERR_BITS = {"no code within 16 bits": 1, "DC category": 1, "run past coefficient 63": 2, "bits beyond the segment": 4, "DC outside int16": 8,
            "bytes left over": 16, "wrong RSTn": 32, "marker inside a segment": 64}
up256 = lambda v: -(-v // 256) * 256


def blocks(im) -> int:
    return im.mcux * im.mcuy * (im.hmax * im.vmax + (2 if im.ncomp == 3 else 0))


def comp_shapes(im):
    """(blocks down, blocks across) per component."""
    return [(im.mcuy * (im.vmax if c == 0 else 1), im.mcux * (im.hmax if c == 0 else 1)) for c in range(im.ncomp)]


def block_offsets(n: int, nseg: int):
    o_seg = n * IMG_BYTES
    o_dht = o_seg + nseg * SEG_BYTES
    o_qt = -(-(o_dht + n * 4 * 272) // 16) * 16
    return o_seg, o_dht, o_qt, -(-(o_qt + n * 512) // 16) * 16


def read_block(blk: np.ndarray, n: int, nseg: int):
    """The descriptors of an upload block -> (images, segments (nseg, 5), offsets)."""
    o_seg, o_dht, o_qt, o_scan = block_offsets(n, nseg)
    imgs = (_lib.GanJpegdecImage * n).from_buffer_copy(blk[:o_seg].tobytes())
    segs = blk[o_seg:o_dht].view(np.int32).reshape(nseg, 5)
    return imgs, segs, (o_seg, o_dht, o_qt, o_scan)


def ref_plan(blk: np.ndarray, i: int, im, segs, offs) -> SimpleNamespace:
    """Image i of the block as a tests.jpegdec_ref plan."""
    _, o_dht, o_qt, _ = offs
    dht = lambda t: (lambda raw: (raw[:16].tolist(), raw[16:16 + int(raw[:16].sum())].tolist()))(blk[o_dht + (4 * i + t) * 272:][:272])
    qt = lambda t: blk[o_qt + (4 * i + t) * 128:][:128].view(np.uint16).astype(np.int64)
    comps = [(im.hmax if c == 0 else 1, im.vmax if c == 0 else 1, qt(im.q_tab[c]), dht(im.dc_tab[c]), dht(im.ac_tab[c])) for c in range(im.ncomp)]
    mine = segs[im.seg_first:im.seg_first + im.seg_count]
    return SimpleNamespace(H=im.H, W=im.W, comps=comps, hmax=im.hmax, vmax=im.vmax, mcux=im.mcux, mcuy=im.mcuy, per=int(mine[0, 2]),
                           segments=[(int(b), int(e)) for b, e in mine[:, 3:5]], data=blk.tobytes())


class JpegDecEmuOps(JpegEmuOps):
    def jpegdec_block_offsets(self, n, nseg):
        assert 1 <= n <= 65535 and nseg >= 1
        return block_offsets(n, nseg)

    def jpegdec_bounds(self, imgs) -> int:
        n = len(imgs)
        o = up256(n * 4 * TABLE_BYTES) + up256(4 * n)
        for im in imgs:
            assert im.ncomp in (1, 3) and 1 <= im.H <= 65535 and 1 <= im.W <= 65535
            im.coef_off, o = o, o + up256(blocks(im) * 128)
        for im in imgs:
            im.plane_off, o = o, o + up256(blocks(im) * 64)
        return o

    def _open(self, blk_dev, nbytes, n, nseg, ws):
        blk = blk_dev[:nbytes].numpy()
        imgs, segs, offs = read_block(blk, n, nseg)
        assert ws.numel() >= imgs[n - 1].plane_off + blocks(imgs[n - 1]) * 64
        err = ws.numpy()[up256(n * 4 * TABLE_BYTES):][:4 * n].view(np.int32)
        return blk, imgs, segs, offs, ws.numpy(), err

    def jpegdec_tables(self, blk_dev, blk_host, nbytes, n, nseg, ws):
        blk, imgs, segs, offs, w, err = self._open(blk_dev, nbytes, n, nseg, ws)
        w[up256(n * 4 * TABLE_BYTES):imgs[0].plane_off] = 0

    def jpegdec_entropy(self, blk_dev, blk_host, nbytes, n, nseg, ws):
        blk, imgs, segs, offs, w, err = self._open(blk_dev, nbytes, n, nseg, ws)
        for i, im in enumerate(imgs):
            try:
                co = R.coefficients(ref_plan(blk, i, im, segs, offs))
            except R.Corrupt as e:
                err[i] |= ERR_BITS[str(e)]
                continue
            flat = np.concatenate([c.reshape(-1) for c in co])
            w[im.coef_off:im.coef_off + flat.size * 2].view(np.int16)[:] = flat

    def jpegdec_idct(self, blk_dev, blk_host, nbytes, n, nseg, ws):
        blk, imgs, segs, offs, w, err = self._open(blk_dev, nbytes, n, nseg, ws)
        for i, im in enumerate(imgs):
            co, at = [], im.coef_off
            for bh, bw in comp_shapes(im):
                co.append(w[at:at + bh * bw * 128].view(np.int16).reshape(bh, bw, 64))
                at += bh * bw * 128
            pl, extreme = R.planes(ref_plan(blk, i, im, segs, offs), co)
            if extreme:
                err[i] |= 128
            flat = np.concatenate([p.reshape(-1) for p in pl])
            w[im.plane_off:im.plane_off + flat.size] = flat

    def jpegdec_pixels(self, blk_dev, blk_host, nbytes, n, nseg, ws, out, err_out):
        blk, imgs, segs, offs, w, err = self._open(blk_dev, nbytes, n, nseg, ws)
        o = out.numpy()
        for i, im in enumerate(imgs):
            pl, at = [], im.plane_off
            for bh, bw in comp_shapes(im):
                pl.append(w[at:at + bh * bw * 64].reshape(bh * 8, bw * 8))
                at += bh * bw * 64
            assert 0 <= im.out_off and im.out_off + im.H * im.W * 3 <= o.size
            o[im.out_off:im.out_off + im.H * im.W * 3] = R.pixels(ref_plan(blk, i, im, segs, offs), pl).reshape(-1)
        err_out[:n] = torch.from_numpy(err.copy())
