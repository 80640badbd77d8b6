"""TEST INFRASTRUCTURE: the PNG decoder's test cases, read from tests/golden/pngdec_cases.npz (written by tools/make_golden_pngdec.py with
Pillow 12.2.0 and zlib 1.2.11): per case the file's bytes and the pixels np.array(Image.open(..).convert("RGB")) gave (or the text of
the error Pillow raised).  Also the tests' own PNG writer and deflate writer, which make the files Pillow and zlib cannot be asked for,
and `build()`, which makes every file (the golden tool calls it; the tests read the stored bytes)."""
from __future__ import annotations

import hashlib
import io
import os
import zlib
from functools import lru_cache

import numpy as np

from tests import pngdec_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pngdec_cases.npz")

FORMATS = ["pixel", "grey", "la", "rgb", "rgba", "pal1.w7", "pal2.w5", "pal4.w3", "pal8.w9", "pal.trns", "rgb.trns"]
FILTERS = ["filter.0", "filter.1", "filter.2", "filter.3", "filter.4", "filter.all", "paeth.ties", "avg.carry", "sub.wide"]
DEFLATE = ["stored", "stored.multi", "fixed", "dynamic", "flush.full", "mixed", "const", "period32768", "bits15", "clsyms", "single.dist", "literals.only"]
FRAMING = ["idat.bytes", "idat.empty", "idat.header"]
CASES = FORMATS + FILTERS + DEFLATE + FRAMING + ["long"]           # the device decodes these
HASHED = ["long", "period32768"]                                   # pixels kept as a SHA-256
PIXEL_CASES = [n for n in CASES if n not in HASHED]
BATCH = ["rgba", "pal2.w5", "filter.all", "grey", "mixed", "pixel", "la", "pal8.w9"]      # formats, sizes and block types all differ
FALLBACK = ["rgb16", "grey2", "interlaced", "badcrc", "jpeg"]      # Pillow decodes these (or raises), the device must not see them
FLAGGED = {                                                        # the parser takes these, the kernels flag them: name -> error bits
    "bad.btype": R.BTYPE, "bad.stored": R.STORED, "bad.hlit": R.COUNTS, "bad.hdist": R.COUNTS, "bad.repeat.first": R.REPEAT, "bad.repeat.past": R.REPEAT,
    "bad.over": R.OVER, "bad.incomplete": R.INCOMPLETE, "bad.noeob": R.NOEOB, "bad.sym286": R.SYMBOL, "bad.dist30": R.SYMBOL, "bad.far": R.DIST,
    "bad.end": R.END, "bad.less": R.LESS, "bad.filter": R.FILTER, "bad.adler": R.ADLER, "bad.cut": None, "surplus": R.MORE,
}


@lru_cache(maxsize=None)
def _npz():
    return dict(np.load(GOLDEN))


def file(name: str) -> bytes:
    return _npz()[f"{name}.file"].tobytes()


def pixels(name: str) -> np.ndarray:
    """Pillow's (H, W, 3) uint8 for the case (not kept for HASHED: see pixels_sha256)."""
    return _npz()[f"{name}.rgb"]


def pillow_error(name: str):
    """The text of the error Pillow raised for the file, None when it gave pixels."""
    z = _npz()
    return z[f"{name}.error"].tobytes().decode() if f"{name}.error" in z else None


def shape(name: str):
    z = _npz()
    return tuple(int(v) for v in z[f"{name}.shape"]) if f"{name}.shape" in z else tuple(z[f"{name}.rgb"].shape)


def pixels_sha256(name: str) -> bytes:
    z = _npz()
    return z[f"{name}.sha256"].tobytes() if f"{name}.sha256" in z else hashlib.sha256(np.ascontiguousarray(z[f"{name}.rgb"]).tobytes()).digest()


# ------------------------------------------------------------------------------------------------ the tests' own PNG writer
def chunk(typ: bytes, body: bytes = b"") -> bytes:
    return len(body).to_bytes(4, "big") + typ + body + zlib.crc32(typ + body).to_bytes(4, "big")


def write_png(W: int, H: int, color: int, depth: int, stream: bytes, palette: bytes = None, trns: bytes = None, interlace: int = 0, split=None) -> bytes:
    """A PNG file around a finished zlib stream.  split: the sizes of the IDAT chunks (the last takes the rest); None: one IDAT."""
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([depth, color, 0, 0, interlace]))
    if palette is not None:
        out += chunk(b"PLTE", palette)
    if trns is not None:
        out += chunk(b"tRNS", trns)
    at = 0
    for n in list(split or []):
        out += chunk(b"IDAT", stream[at:at + n])
        at += n
    return out + chunk(b"IDAT", stream[at:]) + chunk(b"IEND")


def filtered(rows: np.ndarray, bpp: int, filters) -> bytes:
    """The rows (H, rowbytes) uint8 as scanlines with the given filter per row."""
    H, rb = rows.shape
    out = bytearray()
    for y in range(H):
        cur = rows[y].astype(int).tolist()
        prev = rows[y - 1].astype(int).tolist() if y else [0] * rb
        ft = filters[y % len(filters)]
        out.append(ft)
        for i in range(rb):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if ft == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
            else:
                pred = (0, a, b, (a + b) >> 1)[ft]
            out.append((cur[i] - pred) & 255)
    return bytes(out)


def zwrap(deflate: bytes, raw: bytes, cmf: int = 0x78) -> bytes:
    flg = next(f for f in range(0, 32) if (cmf << 8 | f) % 31 == 0)
    return bytes([cmf, flg]) + deflate + zlib.adler32(raw).to_bytes(4, "big")


# ------------------------------------------------------------------------------------------------ the tests' own deflate writer
class Bits:
    """Least significant bit first, as RFC 1951 packs them."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value: int, k: int):
        self.v |= (value & ((1 << k) - 1)) << self.n
        self.n += k

    def code(self, code_len):                     # a Huffman code goes in most significant bit first
        code, l = code_len
        self.put(int(f"{code:0{l}b}"[::-1], 2), l)

    def align(self):
        self.n = -(-self.n // 8) * 8

    def bytes(self) -> bytes:
        return self.v.to_bytes(-(-self.n // 8), "little")


def canonical(lens):
    """symbol -> (code, length) of the canonical code with these lengths (not checked for completeness: the bad files need that)."""
    out, code = {}, 0
    for l in range(1, 16):
        for s, k in enumerate(lens):
            if k == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def complete_lengths(symbols, size: int):
    """A complete code over the given symbols (at least two): lengths m - 1 and m."""
    k = len(symbols)
    m = max(1, (k - 1).bit_length())
    short = (1 << m) - k
    lens = [0] * size
    for i, s in enumerate(sorted(symbols)):
        lens[s] = m - 1 if i < short else m
    return lens


FIXED_LIT, FIXED_DIST = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32


def put_tokens(b: Bits, tokens, lit, dist):
    """tokens: ints (literals) and (length, distance) pairs; then the end-of-block code.  lit / dist: symbol -> (code, length)."""
    for t in tokens:
        if isinstance(t, int):
            b.code(lit[t])
            continue
        n, d = t
        s = max(s for s in range(257, 286) if R.length_code(s)[0] <= n and (s != 285 or n == 258))
        base, x = R.length_code(s)
        b.code(lit[s])
        b.put(n - base, x)
        s = max(s for s in range(30) if R.distance_code(s)[0] <= d)
        base, x = R.distance_code(s)
        b.code(dist[s])
        b.put(d - base, x)
    b.code(lit[256])


def run_lengths(lens):
    """Code lengths -> code-length symbols [(symbol, extra value, extra bits)] with 16 / 17 / 18 wherever they fit."""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            n = min(run, 138)
            out.append((18, n - 11, 7) if n >= 11 else (17, n - 3, 3))
            i += n
        elif v and run >= 4:
            out.append((v, 0, 0))
            n = min(run - 1, 6)
            out.append((16, n - 3, 2))
            i += 1 + n
        else:
            out.append((v, 0, 0))
            i += 1
    return out


def put_dynamic_header(b: Bits, hlit: int, hdist: int, cl_symbols, cl_lens=None):
    """HLIT / HDIST / HCLEN, the code-length code and the given code-length symbols."""
    cl_lens = cl_lens or complete_lengths({s for s, _, _ in cl_symbols} | ({0, 1} if len({s for s, _, _ in cl_symbols}) < 2 else set()), 19)
    hclen = max(i for i, s in enumerate(R.ORDER) if cl_lens[s]) + 1
    hclen = max(hclen, 4)
    b.put(hlit - 257, 5), b.put(hdist - 1, 5), b.put(hclen - 4, 4)
    for i in range(hclen):
        b.put(cl_lens[R.ORDER[i]], 3)
    cc = canonical(cl_lens)
    for s, v, x in cl_symbols:
        b.code(cc[s])
        b.put(v, x)


def put_block(b: Bits, final: bool, kind: str, tokens=(), lit_lens=None, dist_lens=None, data: bytes = b""):
    b.put(int(final), 1)
    if kind == "stored":
        b.put(0, 2), b.align()
        b.put(len(data), 16), b.put(~len(data), 16)
        for v in data:
            b.put(v, 8)
    elif kind == "fixed":
        b.put(1, 2)
        put_tokens(b, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))
    else:
        b.put(2, 2)
        put_dynamic_header(b, len(lit_lens), len(dist_lens), run_lengths(list(lit_lens) + list(dist_lens)))
        put_tokens(b, tokens, canonical(lit_lens), canonical(dist_lens))


def tokens_of(raw: bytes):
    """A greedy tokeniser good enough for tests: a match (at most 258 long, any distance) where the last 3 bytes were seen before."""
    out, i, seen = [], 0, {}
    while i < len(raw):
        key = raw[i:i + 3]
        j = seen.get(key)
        if j is not None and len(key) == 3:
            n = 3
            while n < 258 and i + n < len(raw) and raw[j + n] == raw[i + n]:
                n += 1
            out.append((n, i - j))
            for k in range(i, i + n):
                seen[raw[k:k + 3]] = k
            i += n
        else:
            out.append(raw[i])
            seen[key] = i
            i += 1
    return out


# ------------------------------------------------------------------------------------------------ every file
def _adam7(px: np.ndarray) -> bytes:
    """(H, W, 3) uint8 -> the unfiltered scanlines of the seven passes."""
    out = bytearray()
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = px[y0::dy, x0::dx]
        if sub.size:
            for row in sub:
                out += b"\x00" + row.tobytes()
    return bytes(out)


def build() -> dict:
    """name -> file bytes, for CASES, FALLBACK and FLAGGED."""
    from PIL import Image
    rng = np.random.default_rng(2024)
    f = {}

    def pil(arr, **kw):
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, "PNG", **kw)
        return buf.getvalue()

    rnd = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
    z = lambda raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY: (lambda c: c.compress(raw) + c.flush())(zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy))
    # formats
    f["pixel"] = pil(rnd(1, 1, 3))
    f["grey"], f["la"], f["rgb"], f["rgba"] = pil(rnd(5, 7)), pil(rnd(5, 7, 2)), pil(rnd(5, 7, 3)), pil(rnd(5, 7, 4))
    for depth, W in ((1, 7), (2, 5), (4, 3), (8, 9)):
        rows = rnd(4, (W * depth + 7) // 8)                      # the padding bits of the rows are random, not zero
        f[f"pal{depth}.w{W}"] = write_png(W, 4, 3, depth, z(filtered(rows, 1, [0, 1, 2, 4])), palette=rnd(3 << depth).tobytes())
    rows = rnd(3, 3)
    f["pal.trns"] = write_png(5, 3, 3, 4, z(filtered(rows, 1, [0])), palette=rnd(48).tobytes(), trns=rnd(16).tobytes())
    rgb = rnd(4, 6 * 3)
    f["rgb.trns"] = write_png(6, 4, 2, 8, z(filtered(rgb, 3, [1])), trns=b"\x00" + bytes(rgb[0, :1]) + b"\x00" + bytes(rgb[0, 1:2]) + b"\x00" + bytes(rgb[0, 2:3]))
    # filters
    rows = rnd(3, 5 * 3)
    for ft in range(5):
        f[f"filter.{ft}"] = write_png(5, 3, 2, 8, z(filtered(rows, 3, [ft])))
    f["filter.all"] = write_png(5, 7, 6, 8, z(filtered(rnd(7, 5 * 4), 4, [4, 3, 2, 1, 0, 4, 3])))
    f["paeth.ties"] = write_png(8, 8, 0, 8, z(filtered(rng.integers(0, 4, (8, 8), dtype=np.uint8), 1, [4])))
    f["avg.carry"] = write_png(6, 4, 4, 8, z(filtered(rng.integers(200, 256, (4, 12), dtype=np.uint8), 2, [3])))
    # deflate
    few = lambda H, W: rng.integers(0, 5, (H, W * 3), dtype=np.uint8)
    raw = filtered(rnd(4, 6 * 3), 3, [0, 2])
    f["stored"] = write_png(6, 4, 2, 8, z(raw, 0))
    c = zlib.compressobj(0)
    f["stored.multi"] = write_png(6, 4, 2, 8, c.compress(raw[:30]) + c.flush(zlib.Z_FULL_FLUSH) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(raw[30:]) + c.flush())
    raw = filtered(few(16, 16), 3, [0])                            # values 0 .. 4 only: the own blocks below code nothing else
    f["fixed"] = write_png(16, 16, 2, 8, z(raw, 9, zlib.Z_FIXED))
    f["dynamic"] = write_png(16, 16, 2, 8, z(raw, 9))
    c = zlib.compressobj(9)
    f["flush.full"] = write_png(16, 16, 2, 8, c.compress(raw[:300]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(raw[300:]) + c.flush())
    b = Bits()
    lit = complete_lengths(set(range(5)) | {256, 257, 258}, 259)
    put_block(b, False, "fixed", tokens_of(raw[:200]))             # ends inside a byte: the next block does not start on a byte boundary
    put_block(b, False, "stored", data=raw[200:260])
    put_block(b, False, "stored", data=b"")
    put_block(b, True, "dynamic", list(raw[260:]), lit_lens=lit, dist_lens=[1, 1])
    f["mixed"] = write_png(16, 16, 2, 8, zwrap(b.bytes(), raw))
    f["const"] = write_png(20, 20, 2, 8, z(bytes(20 * 61), 9))
    first = bytearray(b"\x00" + rng.integers(0, 256, 255, dtype=np.uint8).tobytes())
    tokens = list(first)
    for j in range(1, 128):
        tokens += [0, j, (254, 256)]
    tokens += [(258, 32768)] * 130 + [(252, 32768)]               # the largest distance, over more than one turn of the ring
    b = Bits()
    put_block(b, True, "fixed", tokens)
    raw = R.inflate(b"\x78\x01" + b.bytes() + bytes(4), 260 * 256)
    f["period32768"] = write_png(255, 260, 0, 8, zwrap(b.bytes(), raw))
    lit = list(range(1, 16)) + [0] * 241 + [15]                    # literal v has a code of v + 1 bits; the end of block 15
    raw = filtered(np.array([[0, 1, 0, 2, 3, 4, 14], [13, 12, 11, 10, 9, 8, 7], [6, 5, 4, 3, 2, 1, 0], [14, 14, 13, 0, 0, 1, 5]], np.uint8), 1, [0, 1, 2, 0])
    raw = bytes(min(v, 14) for v in raw)
    b = Bits()
    put_block(b, True, "dynamic", list(raw), lit_lens=lit, dist_lens=[1, 1])
    f["bits15"] = write_png(7, 4, 0, 8, zwrap(b.bytes(), raw))
    lit = [4] * 7 + [0] * 5 + [4] + [0] * 242 + [5, 5, 3, 2, 5, 5]    # 17 for the short run of zeros, 18 for the long one, 16 from 259 into the distances
    dist = [5, 5, 5, 5, 3, 3, 3, 2, 2]
    vals = np.array([0, 1, 2, 3, 4, 5, 6, 12, 255], np.uint8)
    rows = vals[rng.integers(0, 9, (4, 7))]
    rows[2] = rows[1]
    raw = filtered(rows, 1, [0])
    b = Bits()
    put_block(b, True, "dynamic", list(raw[:16]) + [(4, 8), (4, 8)] + list(raw[24:]), lit_lens=lit, dist_lens=dist)
    f["clsyms"] = write_png(7, 4, 0, 8, zwrap(b.bytes(), raw))
    raw = bytes(4 * 8)
    b = Bits()
    put_block(b, True, "dynamic", [0, (3, 1), 0, (3, 1), (3, 1), (3, 1), (3, 1), (3, 1), (3, 1), (3, 1), (3, 1), (3, 1)], lit_lens=[1] + [0] * 255 + [2, 2], dist_lens=[1])
    f["single.dist"] = write_png(7, 4, 0, 8, zwrap(b.bytes(), raw))
    rows = rng.integers(0, 3, (4, 7), dtype=np.uint8)
    raw = filtered(rows, 1, [0])
    b = Bits()
    put_block(b, True, "dynamic", list(raw), lit_lens=[2, 2, 2] + [0] * 253 + [2], dist_lens=[0])
    f["literals.only"] = write_png(7, 4, 0, 8, zwrap(b.bytes(), raw))
    # IDAT framing
    p = R.parse(f["rgb"])
    f["idat.bytes"] = write_png(7, 5, 2, 8, p.stream, split=[1] * (len(p.stream) - 1))
    f["idat.empty"] = write_png(7, 5, 2, 8, p.stream, split=[len(p.stream) // 2, 0])
    f["idat.header"] = write_png(7, 5, 2, 8, p.stream, split=[1])
    # long: smooth, photo-like, with Pillow's adaptive filters; several IDATs, output far beyond one window
    yy, xx = np.mgrid[0:256, 0:256]
    base = np.stack([128 + 100 * np.sin(xx / 37.0 + yy / 91.0), 128 + 90 * np.cos(xx / 53.0) * np.sin(yy / 29.0), (xx + 2 * yy) / 3.0], -1)
    f["long"] = pil(np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8))
    # fallback
    px = rnd(3, 5, 3)
    f["rgb16"] = write_png(5, 3, 2, 16, z(filtered(rnd(3, 5 * 6), 6, [0, 1, 4])))
    f["grey2"] = write_png(5, 3, 0, 2, z(filtered(rnd(3, 2), 1, [0])))
    f["interlaced"] = write_png(5, 3, 2, 8, z(_adam7(px)), interlace=1)
    good = f["rgb"]
    at = good.index(b"IDAT") + 4 + len(R.parse(good).stream)
    f["badcrc"] = good[:at] + bytes([good[at] ^ 0x55]) + good[at + 1:]
    buf = io.BytesIO()
    Image.fromarray(rnd(9, 11, 3)).save(buf, "JPEG", quality=90)
    f["jpeg"] = buf.getvalue()
    # flagged by the kernels: grey 7 x 4, 32 raw bytes
    rows = rng.integers(0, 3, (4, 7), dtype=np.uint8)
    raw = filtered(rows, 1, [0])
    grey = lambda deflate, data=raw: write_png(7, 4, 0, 8, zwrap(deflate, data))

    def stream(fn) -> bytes:
        b = Bits()
        fn(b)
        return b.bytes()
    lit3 = [2, 2, 2] + [0] * 253 + [2]
    f["bad.btype"] = grey(stream(lambda b: (b.put(1, 1), b.put(3, 2), b.put(0, 29))))
    f["bad.stored"] = grey(stream(lambda b: (b.put(1, 1), b.put(0, 2), b.align(), b.put(32, 16), b.put(~32 ^ 1, 16))) + raw)
    f["bad.hlit"] = grey(stream(lambda b: (b.put(1, 1), b.put(2, 2), b.put(30, 5), b.put(0, 5), b.put(0, 4), b.put(0, 40))))
    f["bad.hdist"] = grey(stream(lambda b: (b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(30, 5), b.put(0, 4), b.put(0, 40))))
    f["bad.repeat.first"] = grey(stream(lambda b: (b.put(1, 1), b.put(2, 2), put_dynamic_header(b, 257, 1, [(16, 0, 2), (2, 0, 0)]), b.put(0, 40))))
    f["bad.repeat.past"] = grey(stream(lambda b: (b.put(1, 1), b.put(2, 2), put_dynamic_header(b, 257, 1, [(2, 0, 0), (18, 127, 7), (18, 127, 7)]), b.put(0, 40))))

    def header_only(lit_lens, dist_lens=(0,)):
        return lambda b: (b.put(1, 1), b.put(2, 2), put_dynamic_header(b, len(lit_lens), len(dist_lens), run_lengths(list(lit_lens) + list(dist_lens))), b.put(0, 40))
    f["bad.over"] = grey(stream(header_only([1, 1] + [0] * 254 + [1])))
    f["bad.incomplete"] = grey(stream(header_only([2] + [0] * 255 + [2])))
    f["bad.noeob"] = grey(stream(header_only([1, 1] + [0] * 255)))
    fl, fd = canonical(FIXED_LIT), canonical(FIXED_DIST)
    f["bad.sym286"] = grey(stream(lambda b: (b.put(1, 1), b.put(1, 2), b.code(fl[0]), b.code(fl[286]), b.put(0, 40))))
    f["bad.dist30"] = grey(stream(lambda b: (b.put(1, 1), b.put(1, 2), b.code(fl[0]), b.code(fl[257]), b.code(fd[30]), b.put(0, 40))))
    f["bad.far"] = grey(stream(lambda b: put_block(b, True, "fixed", [0, 0, (3, 3)] + [0] * 27)))
    whole = stream(lambda b: put_block(b, True, "dynamic", list(raw), lit_lens=lit3, dist_lens=[0]))
    f["bad.end"] = grey(whole[:len(whole) - 3])
    f["bad.less"] = write_png(7, 4, 0, 8, z(raw[:-3]))
    f["surplus"] = write_png(7, 4, 0, 8, z(raw + bytes(range(9))))
    f["bad.filter"] = write_png(7, 4, 0, 8, z(raw[:16] + b"\x05" + raw[17:]))
    good = z(raw)
    f["bad.adler"] = write_png(7, 4, 0, 8, good[:-1] + bytes([good[-1] ^ 1]))
    big = R.parse(f["dynamic"]).stream
    f["bad.cut"] = write_png(16, 16, 2, 8, big[:len(big) * 6 // 10])
    # Sub over a row of 150 pixels: 64 lanes take three pixels each, the last fourteen none (made last: the files above keep their bytes)
    f["sub.wide"] = write_png(150, 3, 2, 8, z(filtered(rnd(3, 150 * 3), 3, [1])))
    return f
