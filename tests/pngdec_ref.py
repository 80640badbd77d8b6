"""TEST INFRASTRUCTURE: a plain Python statement of the device PNG decoder's stages -- inflate with the kernels' error bits, unfilter,
to-RGB -- which the kernels (csrc/pngdec.hip) are held to stage by stage; it is itself held to zlib, the golden pixels and live Pillow.
Independent of the product's parser: `parse` below reads the chunks on its own (and checks no CRC)."""
from __future__ import annotations

import io
import zlib
from types import SimpleNamespace

import numpy as np

BTYPE, STORED, COUNTS, REPEAT, OVER, INCOMPLETE, NOEOB, SYMBOL, DIST, END, MORE, LESS, LEFT, FILTER, ADLER = (1 << i for i in range(15))
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


class Flag(Exception):
    """The stream is one the device flags; .bits: the error word."""

    def __init__(self, bits: int):
        super().__init__(bits)
        self.bits = bits


def length_code(s: int):
    """Literal/length symbol 257 .. 285 -> (base, extra bits)."""
    if s < 265:
        return s - 254, 0
    if s == 285:
        return 258, 0
    x = (s - 261) >> 2
    return ((4 + ((s - 265) & 3)) << x) + 3, x


def distance_code(s: int):
    if s < 4:
        return s + 1, 0
    x = (s >> 1) - 1
    return ((2 + (s & 1)) << x) + 1, x


class _Code:
    """A canonical code from its lengths; raises Flag as the device's table builder returns its bits."""

    def __init__(self, lens, codes: bool):
        count = [0] * 16
        for l in lens:
            count[l] += 1
        left, code, self.first, self.count, self.offs, p = 1, 0, [0] * 16, count, [0] * 16, 0
        for l in range(1, 16):
            left = (left << 1) - count[l]
            if left < 0:
                raise Flag(OVER)
            self.first[l], self.offs[l] = code, p
            p, code = p + count[l], (code + count[l]) << 1
        maxlen = max((l for l in range(1, 16) if count[l]), default=0)
        if left > 0 and (codes or maxlen > 1):
            raise Flag(INCOMPLETE)
        self.sym = [s for l in range(1, 16) for s, k in enumerate(lens) if k == l]


class _Bits:
    def __init__(self, data: bytes):
        self.data, self.pos, self.buf, self.n = data, 0, 0, 0

    def _fill(self, k):
        while self.n < k and self.pos < len(self.data):
            self.buf |= self.data[self.pos] << self.n
            self.pos, self.n = self.pos + 1, self.n + 8

    def take(self, k: int) -> int:
        self._fill(k)
        if k > self.n:
            raise Flag(END)
        v = self.buf & ((1 << k) - 1)
        self.buf, self.n = self.buf >> k, self.n - k
        return v

    def symbol(self, c: _Code) -> int:
        self._fill(15)
        code = 0
        for l in range(1, 16):                   # bits past the end read as zeros; a code that needs them is END, no code at all is SYMBOL
            code = code << 1 | (self.buf >> (l - 1) & 1)
            if c.count[l] and code - c.first[l] < c.count[l]:
                if l > self.n:
                    raise Flag(END)
                self.buf, self.n = self.buf >> l, self.n - l
                return c.sym[c.offs[l] + code - c.first[l]]
        raise Flag(SYMBOL)


def inflate(stream: bytes, raw_bytes: int, wbits: int = 15) -> bytes:
    """The zlib stream (2 header bytes, deflate data, Adler-32) -> exactly raw_bytes bytes, or Flag with the device's error bits."""
    b = _Bits(stream[2:len(stream) - 4])
    out = bytearray()
    fixed = None
    while True:
        final, kind = b.take(1), b.take(2)
        if kind == 3:
            raise Flag(BTYPE)
        if kind == 0:
            b.take(b.n & 7)
            n, inv = b.take(16), b.take(16)
            if n != (~inv & 0xFFFF):
                raise Flag(STORED)
            pos = b.pos - b.n // 8
            if pos + n > len(b.data):
                raise Flag(END)
            if len(out) + n > raw_bytes:
                raise Flag(MORE)
            out += b.data[pos:pos + n]
            b.pos, b.buf, b.n = pos + n, 0, 0
        else:
            if kind == 1:
                fixed = fixed or (_Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False), _Code([5] * 32, False))
                lit, dist = fixed
            else:
                hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                if hlit > 286 or hdist > 30:
                    raise Flag(COUNTS)
                cl = [0] * 19
                for k in range(hclen):
                    cl[ORDER[k]] = b.take(3)
                cc = _Code(cl, True)
                lens = []
                while len(lens) < hlit + hdist:
                    s = b.symbol(cc)
                    if s < 16:
                        rep, v = 1, s
                    elif s == 16:
                        if not lens:
                            raise Flag(REPEAT)
                        rep, v = 3 + b.take(2), lens[-1]
                    else:
                        rep, v = (3 + b.take(3), 0) if s == 17 else (11 + b.take(7), 0)
                    if len(lens) + rep > hlit + hdist:
                        raise Flag(REPEAT)
                    lens += [v] * rep
                if lens[256] == 0:
                    raise Flag(NOEOB)
                lit, dist = _Code(lens[:hlit], False), _Code(lens[hlit:], False)
            while True:
                s = b.symbol(lit)
                if s == 256:
                    break
                if s < 256:
                    if len(out) >= raw_bytes:
                        raise Flag(MORE)
                    out.append(s)
                    continue
                if s > 285:
                    raise Flag(SYMBOL)
                base, x = length_code(s)
                n = base + b.take(x)
                ds = b.symbol(dist)
                if ds > 29:
                    raise Flag(SYMBOL)
                base, x = distance_code(ds)
                d = base + b.take(x)
                if d > len(out) or d > 1 << wbits:
                    raise Flag(DIST)
                if len(out) + n > raw_bytes:
                    raise Flag(MORE)
                if d >= n:
                    out += out[len(out) - d:len(out) - d + n]
                else:
                    out += (bytes(out[-d:]) * (n // d + 1))[:n]
        if final:
            break
    if len(out) < raw_bytes:
        raise Flag(LESS)
    if len(b.data) - b.pos + b.n // 8 > 0:
        raise Flag(LEFT)
    return bytes(out)


def unfilter(raw: bytes, H: int, rowbytes: int, bpp: int) -> np.ndarray:
    """The H rows of (filter byte, rowbytes bytes) -> (H, rowbytes) uint8; Flag(FILTER) for a filter byte above 4."""
    rows = np.zeros((H, rowbytes), np.uint8)
    prev = [0] * rowbytes
    for y in range(H):
        line = raw[y * (1 + rowbytes):(y + 1) * (1 + rowbytes)]
        ft, cur = line[0], list(line[1:])
        if ft > 4:
            raise Flag(FILTER)
        for i in range(rowbytes):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) >> 1
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
            cur[i] = (cur[i] + pred) & 255
        rows[y] = cur
        prev = cur
    return rows


def to_rgb(rows: np.ndarray, W: int, color: int, depth: int, palette: bytes) -> np.ndarray:
    H = rows.shape[0]
    if color == 3:
        bits = np.unpackbits(rows, axis=1)[:, :W * depth].reshape(H, W, depth)           # most significant bit first; the padding bits dropped
        idx = (bits.astype(np.int64) << np.arange(depth - 1, -1, -1)).sum(-1)
        pal = np.zeros((256, 3), np.uint8)
        pal[:len(palette) // 3] = np.frombuffer(palette, np.uint8).reshape(-1, 3)
        return pal[idx]
    ch = CHANNELS[color]
    px = rows[:, :W * ch].reshape(H, W, ch)
    return np.ascontiguousarray(px[:, :, :3] if color in (2, 6) else np.repeat(px[:, :, :1], 3, axis=2))


def parse(data: bytes) -> SimpleNamespace:
    """Header, palette and the concatenated IDAT payloads of a PNG file (no CRC check, no refusals beyond the signature)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out, idat = 8, SimpleNamespace(palette=b""), []
    while pos + 12 <= len(data):
        L, typ = int.from_bytes(data[pos:pos + 4], "big"), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + L]
        if typ == b"IHDR":
            out.W, out.H = int.from_bytes(body[:4], "big"), int.from_bytes(body[4:8], "big")
            out.depth, out.color, _, _, out.interlace = body[8:13]
        elif typ == b"PLTE":
            out.palette = bytes(body)
        elif typ == b"IDAT":
            idat.append(bytes(body))
        pos += 12 + L
    out.stream = b"".join(idat)
    ch = CHANNELS[out.color]
    out.rowbytes, out.bpp = (out.W * ch * out.depth + 7) // 8, max(1, ch * out.depth // 8)
    out.raw_bytes = out.H * (1 + out.rowbytes)
    out.wbits = (out.stream[0] >> 4) + 8
    return out


def stages(data: bytes) -> SimpleNamespace:
    """raw (after inflate), rows (unfiltered), pixels of a file of the accepted class; Flag where the device flags."""
    p = parse(data)
    raw = inflate(p.stream, p.raw_bytes, p.wbits)
    rows = unfilter(raw, p.H, p.rowbytes, p.bpp)
    if zlib.adler32(raw) != int.from_bytes(p.stream[-4:], "big"):
        raise Flag(ADLER)
    return SimpleNamespace(plan=p, raw=raw, rows=rows, pixels=to_rgb(rows, p.W, p.color, p.depth, p.palette))


def decode(data: bytes) -> np.ndarray:
    return stages(data).pixels


def pillow_pixels(data: bytes) -> np.ndarray:
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))
