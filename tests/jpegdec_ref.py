"""TEST INFRASTRUCTURE: the baseline JPEG decoder restated in numpy, by stages, as Pillow (libjpeg-turbo) runs it for
Image.open(p).convert("RGB"): parse -> coefficients (Huffman decode, natural order) -> planes (dequantise + jidctint.c's
jpeg_idct_islow) -> pixels (jdsample.c's fancy h2v1 / h2v2 upsampling, jdcolor.c's fixed-point YCbCr -> RGB).  The device decoder
(csrc/jpegdec.hip) is held to it stage by stage; it is itself held to the golden pixels and to live Pillow.  Independent of the product's
parser.  Never imported by the product package."""
from __future__ import annotations

import io
from types import SimpleNamespace

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class NotBaseline(Exception):
    """The file is outside the class the device decoder takes."""


class Corrupt(Exception):
    """The scan is irregular: the device decoder flags the file."""


def pillow_pixels(data: bytes) -> np.ndarray:
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))


def markers(data: bytes):
    """(marker, body) of every segment up to and including SOS, then the position of the first scan byte."""
    assert data[:2] == b"\xff\xd8"
    pos, out = 2, []
    while True:
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise NotBaseline("marker expected")
        m, L = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        out.append((m, data[pos + 4:pos + 2 + L]))
        pos += 2 + L
        if m == 0xDA:
            return out, pos


def parse(data: bytes) -> SimpleNamespace:
    """H, W, comps [(h, v, quant table (64,) natural order, (DC counts, symbols), (AC counts, symbols))], restart interval and the
    restart segments of the scan as (first byte, end) pairs."""
    segs, sb = markers(data)
    qt, dht, sof, ri = {}, {}, None, 0
    for m, body in segs:
        if m == 0xDB:
            while body:
                if body[0] >> 4:
                    raise NotBaseline("16-bit quantisation table")
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = list(body[1:65])
                qt[body[0] & 15], body = q, body[65:]
        elif m == 0xC4:
            while body:
                n = sum(body[1:17])
                dht[body[0]], body = (list(body[1:17]), list(body[17:17 + n])), body[17 + n:]
        elif m == 0xC0:
            if sof is not None:
                raise NotBaseline("two frames")
            sof = body
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC, 0xDC):
            raise NotBaseline(f"marker {m:#x}")
        elif m == 0xDD:
            ri = int.from_bytes(body[:2], "big")
        elif m == 0xEE and body[:5] == b"Adobe":
            raise NotBaseline("Adobe marker")
        elif m == 0xDA:
            sos = body
    if sof is None or sof[0] != 8:
        raise NotBaseline("no 8-bit SOF0")
    H, W, nc = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    samp = [(sof[7 + 3 * c] >> 4, sof[7 + 3 * c] & 15) for c in range(nc)]
    if not ((nc == 1 and samp == [(1, 1)]) or (nc == 3 and samp[1:] == [(1, 1), (1, 1)] and samp[0] in ((1, 1), (2, 1), (2, 2))
                                                and [sof[6 + 3 * c] for c in range(3)] == [1, 2, 3])):
        raise NotBaseline(f"components {samp}")
    if sos[0] != nc or tuple(sos[-3:]) != (0, 63, 0):
        raise NotBaseline("not one sequential scan of all components")
    comps = []
    for c in range(nc):
        assert sos[1 + 2 * c] == sof[6 + 3 * c]
        td, ta = sos[2 + 2 * c] >> 4, sos[2 + 2 * c] & 15
        comps.append((samp[c][0], samp[c][1], qt[sof[8 + 3 * c]], dht[td], dht[0x10 | ta]))
    # the scan: up to the first marker that is neither a stuffed byte nor RSTn, which must be EOI
    pos, cuts = sb, []
    while True:
        pos = data.find(b"\xff", pos)
        if pos < 0 or pos + 1 >= len(data):
            raise NotBaseline("no EOI")
        m = data[pos + 1]
        if m == 0:
            pos += 2
        elif 0xD0 <= m <= 0xD7:
            cuts.append(pos)
            pos += 2
        elif m == 0xD9:
            break
        else:
            raise NotBaseline(f"marker {m:#x} in the scan")
    hmax, vmax = samp[0]
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    per = ri or mcux * mcuy
    if len(cuts) != -(-mcux * mcuy // per) - 1:
        raise NotBaseline("restart markers do not match the interval")
    segments = list(zip([sb] + [c + 2 for c in cuts], cuts + [pos]))
    return SimpleNamespace(H=H, W=W, comps=comps, hmax=hmax, vmax=vmax, mcux=mcux, mcuy=mcuy, per=per, segments=segments, data=data)


def _codes(counts, symbols):
    """{(length, code): symbol}."""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[(l, code)] = symbols[k]
            code, k = code + 1, k + 1
        code <<= 1
    return out


class _Bits:
    def __init__(self, raw: bytes):
        if b"\xff" in raw.replace(b"\xff\x00", b""):
            raise Corrupt("marker inside a segment")
        self.bits = "".join(f"{b:08b}" for b in raw.replace(b"\xff\x00", b"\xff"))
        self.pos = 0

    def symbol(self, table):
        for l in range(1, 17):
            if self.pos + l > len(self.bits):
                raise Corrupt("bits beyond the segment")
            s = table.get((l, int(self.bits[self.pos:self.pos + l], 2)))
            if s is not None:
                self.pos += l
                return s
        raise Corrupt("no code within 16 bits")

    def extend(self, s):
        if s == 0:
            return 0
        if self.pos + s > len(self.bits):
            raise Corrupt("bits beyond the segment")
        v = int(self.bits[self.pos:self.pos + s], 2)
        self.pos += s
        return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def coefficients(p) -> list:
    """Per component an int16 array (blocks down, blocks across, 64) in natural order over the MCU-padded component."""
    out = [np.zeros((p.mcuy * v, p.mcux * h, 64), np.int16) for h, v, *_ in p.comps]
    tables = [(_codes(*dc), _codes(*ac)) for *_, dc, ac in p.comps]
    for j, (b, e) in enumerate(p.segments):
        if j and p.data[b - 2:b] != bytes((0xFF, 0xD0 + (j - 1) % 8)):
            raise Corrupt("wrong RSTn")
        bits, pred = _Bits(p.data[b:e]), [0] * len(p.comps)
        for mcu in range(j * p.per, min((j + 1) * p.per, p.mcux * p.mcuy)):
            my, mx = divmod(mcu, p.mcux)
            for c, (h, v, *_) in enumerate(p.comps):
                for u in range(h * v):
                    blk = out[c][my * v + u // h, mx * h + u % h]
                    s = bits.symbol(tables[c][0])
                    if s > 15:
                        raise Corrupt("DC category")
                    pred[c] += bits.extend(s)
                    if not -32768 <= pred[c] <= 32767:
                        raise Corrupt("DC outside int16")
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = bits.symbol(tables[c][1])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            raise Corrupt("run past coefficient 63")
                        blk[ZIGZAG[k]] = bits.extend(s)
                        k += 1
        if len(bits.bits) - bits.pos >= 8:
            raise Corrupt("bytes left over")
    return out


def _pass(d, axis, shift):
    """One 1-D pass of jpeg_idct_islow along `axis` of an int64 array whose `axis` has length 8."""
    x = np.moveaxis(d, axis, 0)
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 - z3 * 15137, z1 + z2 * 6270
    tmp0, tmp1 = (x[0] + x[4]) << 13, (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    rows = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.moveaxis((np.stack(rows) + (1 << (shift - 1))) >> shift, 0, axis)


def planes(p, coefs):
    """Per component the uint8 plane over the MCU-padded component, and whether any intermediate left the range in which libjpeg's C
    and SIMD code agree (dequantised products and pass-1 values in int16, descaled row values in -512 .. 511)."""
    out, extreme = [], False
    for (h, v, q, *_), c in zip(p.comps, coefs):
        d = c.astype(np.int64).reshape(c.shape[0], c.shape[1], 8, 8) * q.reshape(8, 8)
        extreme |= bool((np.abs(d + 0.5) > 32768).any())
        d = _pass(d, 2, 11)
        extreme |= bool((np.abs(d + 0.5) > 32768).any())
        d = _pass(d, 3, 18)
        extreme |= bool((np.abs(d + 0.5) > 512).any())
        out.append(np.clip(d + 128, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(c.shape[0] * 8, c.shape[1] * 8))
    return out, extreme


def _upsample(p, pl):
    H, W = p.H, p.W
    if p.hmax == 1:
        return pl[:H, :W].astype(np.int64)
    cw = -(-W // 2)
    if p.vmax == 1:
        s = pl[:H, :cw].astype(np.int64)
        if cw <= 2:
            return np.repeat(s, 2, 1)[:, :W]
        prev, nxt = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        even, odd = (3 * s + prev + 1) >> 2, (3 * s + nxt + 2) >> 2
        even[:, 0], odd[:, -1] = s[:, 0], s[:, -1]
        return np.stack([even, odd], 2).reshape(H, 2 * cw)[:, :W]
    ch = -(-H // 2)
    s = pl[:ch, :cw].astype(np.int64)
    if cw <= 2:
        return np.repeat(np.repeat(s, 2, 0), 2, 1)[:H, :W]
    above, below = np.concatenate([s[:1], s[:-1]]), np.concatenate([s[1:], s[-1:]])
    rows = np.stack([3 * s + above, 3 * s + below], 1).reshape(2 * ch, cw)
    prev, nxt = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    even, odd = (3 * rows + prev + 8) >> 4, (3 * rows + nxt + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * rows[:, 0] + 8) >> 4, (4 * rows[:, -1] + 7) >> 4
    return np.stack([even, odd], 2).reshape(2 * ch, 2 * cw)[:H, :W]


def pixels(p, pls) -> np.ndarray:
    Y = pls[0][:p.H, :p.W].astype(np.int64)
    if len(pls) == 1:
        return np.repeat(Y[..., None], 3, 2).astype(np.uint8)
    cb, cr = _upsample(p, pls[1]) - 128, _upsample(p, pls[2]) - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], 2), 0, 255).astype(np.uint8)


def stages(data: bytes) -> SimpleNamespace:
    p = parse(data)
    co = coefficients(p)
    pl, extreme = planes(p, co)
    return SimpleNamespace(plan=p, coefs=co, planes=pl, extreme=extreme, pixels=pixels(p, pl))


def decode(data: bytes) -> np.ndarray:
    return stages(data).pixels
