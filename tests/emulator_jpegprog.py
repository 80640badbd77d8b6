"""TEST INFRASTRUCTURE: emulator statement of the progressive JPEG decoder's entries (csrc/jpegprog.hip): the entropy stage of
tests.jpegprog_ref and the later stages of tests.jpegdec_ref over the same upload block and the same workspace layout, with the same
refusals, so that dataio.JpegDecoder(progressive=True) and everything above it run on the CPU.  Never imported by the product package."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from gan_variant_research_amd import _lib
from tests import jpegdec_ref as R, jpegprog_ref as P
from tests.emulator_jpegdec import TABLE_BYTES, blocks, comp_shapes, up256
from tests.emulator_pngdec import PngDecEmuOps

IMG_BYTES = C.sizeof(_lib.GanJpegdecImage)
MAX_SCANS = MAX_TABLES = 64
up16 = lambda v: -(-v // 16) * 16


def block_offsets(n: int, nscan: int, nseg: int, nver: int):
    o_pimg = up16(n * IMG_BYTES)
    o_scan = o_pimg + 32 * n
    o_seg = o_scan + 64 * nscan
    o_dht = o_seg + 32 * nseg
    o_qt = up16(o_dht + 272 * nver)
    return o_pimg, o_scan, o_seg, o_dht, o_qt, up16(o_qt + 512 * n)


def read_block(blk: np.ndarray, counts):
    """The descriptors of an upload block -> (images, progressive images (n, 8), scans (nscan, 16), segments (nseg, 8), offsets)."""
    n, nscan, nseg, nver = counts
    offs = block_offsets(*counts)
    imgs = (_lib.GanJpegdecImage * n).from_buffer_copy(blk[:n * IMG_BYTES].tobytes())
    view = lambda a, b, w: blk[a:b].view(np.int32).reshape(-1, w)
    return imgs, view(offs[0], offs[1], 8), view(offs[1], offs[2], 16), view(offs[2], offs[3], 8), offs


def ref_plan(blk: np.ndarray, i: int, im, pimg, scans, segs, offs) -> SimpleNamespace:
    """Image i of the block as a tests.jpegprog_ref plan."""
    o_dht, o_qt = offs[3], offs[4]
    c0, nsc, s0, nsg, v0, nv, _, _ = (int(v) for v in pimg[i])
    dht = lambda t: (lambda raw: (raw[:16].tolist(), raw[16:16 + int(raw[:16].sum())].tolist()))(blk[o_dht + (v0 + t) * 272:][:272])
    qt = lambda t: blk[o_qt + (4 * i + t) * 128:][:128].view(np.uint16).astype(np.int64)
    comps = [(im.hmax if c == 0 else 1, im.vmax if c == 0 else 1, qt(im.q_tab[c])) for c in range(im.ncomp)]
    mine = segs[s0:s0 + nsg]
    out = []
    for j in range(nsc):
        _, comp, Ss, Se, Ah, Al, t0, t1, t2, dep, level = (int(v) for v in scans[c0 + j, :11])
        rows = mine[mine[:, 1] == c0 + j]
        rows = rows[np.argsort(rows[:, 2])]
        tables = {c: dht(t) for c, t in enumerate((t0, t1, t2)) if t >= 0 and (comp < 0 or comp == c)}
        out.append(SimpleNamespace(comp=comp, Ss=Ss, Se=Se, Ah=Ah, Al=Al, tables=tables, per=int(rows[0, 4]), segments=[(int(b), int(e)) for b, e in rows[:, 5:7]],
                                   units=int(rows[-1, 3] + rows[-1, 4])))
    return SimpleNamespace(H=im.H, W=im.W, comps=comps, hmax=im.hmax, vmax=im.vmax, mcux=im.mcux, mcuy=im.mcuy, scans=out, data=blk.tobytes())


class JpegProgEmuOps(PngDecEmuOps):
    def jpegprog_block_offsets(self, n, nscan, nseg, nver):
        assert 1 <= n <= 65535 and 1 <= nscan <= MAX_SCANS * n and nseg >= 1 and 1 <= nver <= MAX_TABLES * n
        return block_offsets(n, nscan, nseg, nver)

    def jpegprog_bounds(self, imgs, nver) -> int:
        n = len(imgs)
        o = up256(nver * TABLE_BYTES) + up256(4 * n)
        for im in imgs:
            assert im.ncomp in (1, 3) and 1 <= im.H <= 65535 and 1 <= im.W <= 65535
            im.coef_off, o = o, o + up256(blocks(im) * 128)
        for im in imgs:
            im.plane_off, o = o, o + up256(blocks(im) * 64)
        return o

    def _prog_open(self, blk_dev, nbytes, counts, ws):
        n, nscan, nseg, nver = counts
        blk = blk_dev[:nbytes].numpy()
        imgs, pimg, scans, segs, offs = read_block(blk, counts)
        assert ws.numel() >= imgs[n - 1].plane_off + blocks(imgs[n - 1]) * 64
        for i in range(n):                       # the refusals of the library
            c0, nsc, s0, nsg, v0, nv, nlevel, _ = (int(v) for v in pimg[i])
            assert 1 <= nsc <= MAX_SCANS and 0 <= c0 and c0 + nsc <= nscan and 1 <= nv <= MAX_TABLES and 0 <= v0 and v0 + nv <= nver and 0 <= s0 and s0 + nsg <= nseg
            for j in range(nsc):
                a = scans[c0 + j]
                assert a[0] == i and -1 <= a[9] < j and 0 <= a[10] < nlevel and all(-1 <= t < nv for t in a[6:9])
                for e in scans[c0:c0 + j]:
                    if (a[1] < 0 or e[1] < 0 or a[1] == e[1]) and a[2] <= e[3] and e[2] <= a[3]:
                        assert e[10] < a[10], "scans of one level touch the same coefficients"
            assert (np.diff(scans[segs[s0:s0 + nsg, 1], 10]) >= 0).all(), "segments not ordered by level"
            for j in range(nsc):                 # a scan's segments come in order and tile its units
                rows = segs[s0:s0 + nsg][segs[s0:s0 + nsg, 1] == c0 + j]
                assert len(rows) and (rows[:, 2] == np.arange(len(rows))).all() and (rows[:, 3] == np.cumsum(rows[:, 4]) - rows[:, 4]).all(), "segments do not tile their scan"
        err = ws.numpy()[up256(nver * TABLE_BYTES):][:4 * n].view(np.int32)
        return blk, imgs, pimg, scans, segs, offs, ws.numpy(), err

    def jpegprog_tables(self, blk_dev, blk_host, nbytes, counts, ws):
        blk, imgs, pimg, scans, segs, offs, w, err = self._prog_open(blk_dev, nbytes, counts, ws)
        w[up256(counts[3] * TABLE_BYTES):imgs[0].plane_off] = 0

    def jpegprog_entropy(self, blk_dev, blk_host, nbytes, counts, ws):
        blk, imgs, pimg, scans, segs, offs, w, err = self._prog_open(blk_dev, nbytes, counts, ws)
        for i, im in enumerate(imgs):
            co, word = P.decode_all(ref_plan(blk, i, im, pimg, scans, segs, offs))      # a flagged file leaves what its lanes stored, as on the device
            err[i] |= word
            flat = np.concatenate([c.reshape(-1) for c in co])
            w[im.coef_off:im.coef_off + flat.size * 2].view(np.int16)[:] = flat

    def jpegprog_idct(self, blk_dev, blk_host, nbytes, counts, ws):
        blk, imgs, pimg, scans, segs, offs, w, err = self._prog_open(blk_dev, nbytes, counts, ws)
        for i, im in enumerate(imgs):
            co, at = [], im.coef_off
            for bh, bw in comp_shapes(im):
                co.append(w[at:at + bh * bw * 128].view(np.int16).reshape(bh, bw, 64))
                at += bh * bw * 128
            pl, extreme = R.planes(ref_plan(blk, i, im, pimg, scans, segs, offs), co)
            if extreme:
                err[i] |= 128
            flat = np.concatenate([p.reshape(-1) for p in pl])
            w[im.plane_off:im.plane_off + flat.size] = flat

    def jpegprog_pixels(self, blk_dev, blk_host, nbytes, counts, ws, out, err_out):
        blk, imgs, pimg, scans, segs, offs, w, err = self._prog_open(blk_dev, nbytes, counts, ws)
        o = out.numpy()
        for i, im in enumerate(imgs):
            pl, at = [], im.plane_off
            for bh, bw in comp_shapes(im):
                pl.append(w[at:at + bh * bw * 64].reshape(bh * 8, bw * 8))
                at += bh * bw * 64
            assert 0 <= im.out_off and im.out_off + im.H * im.W * 3 <= o.size
            o[im.out_off:im.out_off + im.H * im.W * 3] = R.pixels(ref_plan(blk, i, im, pimg, scans, segs, offs), pl).reshape(-1)
        err_out[:counts[0]] = torch.from_numpy(err.copy())
