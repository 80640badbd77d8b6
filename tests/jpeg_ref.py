"""TEST INFRASTRUCTURE: integer restatement of libjpeg's baseline encoder as Pillow drives it with
`save(format="JPEG", quality=q, subsampling=0, optimize=True)` (GAN_Variant1/generate_folder.py:252): 8-bit, JDCT_ISLOW, 4:4:4, one
interleaved scan, optimal Huffman tables, no restart markers.  It is the statement csrc/jpeg.hip is held to, stage by stage;
`stages()` keeps every intermediate (quantised zig-zag coefficients, histograms, tables, the unstuffed bit string) so a device mismatch
can be located without rerunning anything.  Never imported by the product package.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Sequence, Tuple

import numpy as np

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
TABLE_IDS = ((0, 0), (1, 0), (0, 1), (1, 1))          # (class, id) of the four DHT segments in file order: DC0, AC0, DC1, AC1


def quant_tables(quality: int) -> np.ndarray:
    """(2, 64) in natural order: jpeg_quality_scaling + jpeg_add_quant_table with force_baseline."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((base * s + 50) // 100, 1, 255) for base in (LUMA, CHROMA)]).astype(np.int64)


def ycc(rgb: np.ndarray) -> np.ndarray:
    """jccolor.c rgb_ycc_convert, (H, W, 3) uint8 -> (H, W, 3) int64 in 0 .. 255."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr], -1)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first: bool):
    """One pass of jfdctint.c over the last axis of d (..., 8)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct(blocks: np.ndarray) -> np.ndarray:
    """(..., 8, 8) level-shifted samples -> (..., 8, 8) coefficients scaled by 8 (jpeg_fdct_islow)."""
    rows = _fdct_pass(blocks.astype(np.int64), True)
    return np.swapaxes(_fdct_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def coefficients(rgb: np.ndarray, quality: int) -> np.ndarray:
    """(H, W, 3) uint8 -> (nmcu, 3, 64) quantised coefficients in zig-zag order; MCUs row-major, edges replicated to a multiple of 8."""
    H, W, _ = rgb.shape
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    px = np.pad(ycc(rgb), ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge") - 128
    blk = px.reshape(Hp // 8, 8, Wp // 8, 8, 3).transpose(0, 2, 4, 1, 3).reshape(-1, 3, 8, 8)
    c = fdct(blk).reshape(-1, 3, 64)
    d = 8 * quant_tables(quality)[[0, 1, 1]][None]
    q = np.sign(c) * ((np.abs(c) + (d >> 1)) // d)
    return q[..., ZIGZAG]


def _nbits(v: int) -> int:
    return int(abs(int(v))).bit_length()


def block_symbols(coef: np.ndarray) -> List[List[Tuple[int, int, int, int]]]:
    """jchuff.c encode_one_block: per block (scan order: MCU-major, Y Cb Cr) the list of (table, symbol, extra bits, extra bit count);
    table 0 DC-Y, 1 AC-Y, 2 DC-C, 3 AC-C."""
    out = []
    last = [0, 0, 0]
    for m in range(coef.shape[0]):
        for ci in range(3):
            blk = coef[m, ci]
            tb = 0 if ci == 0 else 2
            syms = []
            diff = int(blk[0]) - last[ci]
            last[ci] = int(blk[0])
            n = _nbits(diff)
            syms.append((tb, n, (diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n))
            r = 0
            for k in range(1, 64):
                v = int(blk[k])
                if v == 0:
                    r += 1
                    continue
                while r > 15:
                    syms.append((tb + 1, 0xF0, 0, 0))
                    r -= 16
                n = _nbits(v)
                syms.append((tb + 1, (r << 4) | n, (v if v >= 0 else v - 1) & ((1 << n) - 1), n))
                r = 0
            if r > 0:
                syms.append((tb + 1, 0x00, 0, 0))
            out.append(syms)
    return out


def histograms(symbols) -> np.ndarray:
    h = np.zeros((4, 256), np.int64)
    for blk in symbols:
        for tb, s, _, _ in blk:
            h[tb, s] += 1
    return h


def merged_code_sizes(freq_in: Sequence[int]) -> List[int]:
    """The first half of jpeg_gen_optimal_table: code lengths before limiting, of the 256 symbols and the pseudo-symbol 256."""
    freq = [int(f) for f in freq_in] + [1]
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    return codesize


def optimal_table(freq_in: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """jpeg_gen_optimal_table: 256 frequencies -> (bits[17] with bits[0] = 0, huffval[n])."""
    codesize, bits = merged_code_sizes(freq_in), [0] * 33
    for i in range(257):
        if codesize[i]:
            assert codesize[i] <= 32, "Huffman code size table overflow"
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [j for i in range(1, 33) for j in range(256) if codesize[j] == i]
    return np.array(bits[:17], np.uint8), np.array(vals, np.uint8)


def canonical_codes(bits: np.ndarray, vals: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """jpeg_make_c_derived_tbl: (code[256], size[256]); size 0 for symbols without a code."""
    code, size = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, p = 0, 0
    for ln in range(1, 17):
        for _ in range(int(bits[ln])):
            code[vals[p]], size[vals[p]] = c, ln
            c, p = c + 1, p + 1
        c <<= 1
    return code, size


def bit_string(symbols, codes) -> Tuple[int, int]:
    """The entropy-coded scan before padding and stuffing, as (value, bit count), first bit most significant."""
    acc, n = 0, 0
    for blk in symbols:
        for tb, s, extra, ne in blk:
            code, size = codes[tb]
            assert size[s] > 0
            acc = (acc << int(size[s])) | int(code[s])
            acc = (acc << ne) | extra
            n += int(size[s]) + ne
    return acc, n


def pad_and_stuff(acc: int, n: int) -> bytes:
    pad = -n % 8
    raw = ((acc << pad) | ((1 << pad) - 1)).to_bytes((n + pad) // 8, "big") if n else b""
    return raw.replace(b"\xff", b"\xff\x00")


def _seg(marker: int, body: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def header(H: int, W: int, quality: int, tables) -> bytes:
    """SOI .. SOS as libjpeg writes them for this configuration; tables: four (bits[17], vals) in the order DC0, AC0, DC1, AC1."""
    qt = quant_tables(quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i in range(2):
        out += _seg(0xDB, bytes([i]) + bytes(qt[i][ZIGZAG].astype(np.uint8)))
    out += _seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for (cls, tid), (bits, vals) in zip(TABLE_IDS, tables):
        out += _seg(0xC4, bytes([(cls << 4) | tid]) + bytes(np.asarray(bits[1:17], np.uint8)) + bytes(np.asarray(vals, np.uint8)))
    return out + _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0]))


def stages(rgb: np.ndarray, quality: int = 95, hist_override=None) -> SimpleNamespace:
    """Every stage of one image.  hist_override: (4, 256) histograms to build the tables from instead of the image's own (they must
    cover its symbols) -- the way a length-limited table is put under a real stream."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    H, W, _ = rgb.shape
    s = SimpleNamespace(H=H, W=W, quality=quality)
    s.coef = coefficients(rgb, quality)
    s.symbols = block_symbols(s.coef)
    s.hist = histograms(s.symbols)
    s.tables = [optimal_table(h) for h in (s.hist if hist_override is None else hist_override)]
    s.codes = [canonical_codes(b, v) for b, v in s.tables]
    s.bits, s.nbits = bit_string(s.symbols, s.codes)
    s.scan = pad_and_stuff(s.bits, s.nbits)
    s.header = header(H, W, quality, s.tables)
    s.file = s.header + s.scan + b"\xff\xd9"
    return s


def encode(rgb: np.ndarray, quality: int = 95) -> bytes:
    return stages(rgb, quality).file


def pillow_bytes(rgb: np.ndarray, quality: int = 95) -> bytes:
    """What the reference writes (generate_folder.py:252)."""
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb, dtype=np.uint8)).save(buf, format="JPEG", quality=quality, subsampling=0, optimize=True)
    return buf.getvalue()


def split_file(data: bytes) -> SimpleNamespace:
    """A baseline file of this layout -> header bytes, DHT tables [(class << 4 | id, bits16, vals)], scan bytes (stuffed, without EOI)."""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    pos, tables = 2, []
    while True:
        assert data[pos] == 0xFF
        m, ln = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + ln]
        if m == 0xC4:
            tables.append((body[0], np.frombuffer(body[1:17], np.uint8), np.frombuffer(body[17:], np.uint8)))
        pos += 2 + ln
        if m == 0xDA:
            break
    return SimpleNamespace(header=data[:pos], tables=tables, scan=data[pos:-2])
