"""TEST INFRASTRUCTURE: the decoder's test cases, read from tests/golden/jpegdec_cases.npz (written by tools/make_golden_jpegdec.py with
Pillow 12.2.0 / libjpeg-turbo): per case the file's bytes and the pixels np.array(Image.open(..).convert("RGB")) gave.  Also the
tests' own baseline writer (coefficients -> file), which makes the files Pillow cannot be asked for."""
from __future__ import annotations

import hashlib
import os
from functools import lru_cache

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpegdec_cases.npz")

# name -> (H, W, mode / subsampling, quality, save options): the smallest shapes at which each stage of the decoder can go wrong
S444, S422, S420 = 0, 1, 2
CASES = {
    "pixel.444": (1, 1, S444, 95, {}), "pixel.420": (1, 1, S420, 95, {}), "pixel.gray": (1, 1, "L", 95, {}),      # one MCU, all padding
    "mcu.444": (8, 8, S444, 95, {}), "mcu.420": (16, 16, S420, 95, {}),                                            # exactly one MCU
    "ragged.9x33.444": (9, 33, S444, 95, {}), "ragged.9x33.422": (9, 33, S422, 95, {}), "ragged.9x33.420": (9, 33, S420, 95, {}),
    "ragged.17x15.444": (17, 15, S444, 95, {}), "ragged.17x15.422": (17, 15, S422, 95, {}), "ragged.17x15.420": (17, 15, S420, 95, {}),
    # downsampled widths 2 (libjpeg replicates instead of its fancy upsampling) and 3 (the narrowest fancy one)
    "narrow.3.422": (5, 3, S422, 95, {}), "narrow.4.420": (5, 4, S420, 95, {}), "narrow.5.420": (7, 5, S420, 95, {}), "narrow.6.422": (3, 6, S422, 95, {}),
    "wide": (31, 48, S420, 95, {}),                        # downsampled height 16: the bottom context row falls on a block edge
    "gray": (24, 40, "L", 95, {}),
    "const": (32, 32, S420, 95, {}),                       # one-symbol tables, every DC difference 0
    "std_tables": (40, 31, S420, 95, {"optimize": False}),  # the standard tables: codes longer than the lookahead width
    "magnitudes": (16, 16, S444, 100, {}),                 # checkerboard: the largest categories
    "runs": (64, 64, S420, 1, {}),                         # ZRL
    "stuffing": (64, 64, S444, 95, {}),                    # 0xFF bytes in the scan
    "rst": (40, 50, S420, 95, {"restart_marker_blocks": 3}),
    "rst_wrap": (64, 64, S444, 60, {"restart_marker_blocks": 1}),      # 64 segments: RSTn wraps eight times, one lane each
    "long": (256, 256, S420, 90, {}),                      # the dataset's shape; pixels kept as a SHA-256
}
PIXEL_CASES = [n for n in CASES if n != "long"]
BATCH = ["ragged.9x33.422", "gray", "rst", "pixel.444", "std_tables", "ragged.17x15.420"]      # sizes, samplings and tables all differ
FALLBACK = ["progressive", "cmyk", "s411", "adobe", "png", "crafted", "corrupt"]               # files Pillow decodes and the device must not
CORRUPT_BYTES = 3


@lru_cache(maxsize=None)
def _npz():
    return dict(np.load(GOLDEN))


def file(name: str) -> bytes:
    return _npz()[f"{name}.file"].tobytes()


def pixels(name: str) -> np.ndarray:
    """Pillow's (H, W, 3) uint8 for the case (not kept for `long`: see pixels_sha256)."""
    return _npz()[f"{name}.rgb"]


def pixels_sha256(name: str) -> bytes:
    z = _npz()
    return z[f"{name}.sha256"].tobytes() if f"{name}.sha256" in z else hashlib.sha256(np.ascontiguousarray(z[f"{name}.rgb"]).tobytes()).digest()


def truncated() -> bytes:
    """`rst` cut at 60 %: Pillow raises for it."""
    d = file("rst")
    return d[:len(d) * 6 // 10]


# ------------------------------------------------------------------------------------------------ the tests' own writer
def _code_table(counts, symbols):
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[symbols[k]] = (code, l)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def _seg(marker: int, body: bytes) -> bytes:
    return bytes((0xFF, marker)) + (len(body) + 2).to_bytes(2, "big") + body


def write_jpeg(H: int, W: int, samp, coefs, qts, dc, ac) -> bytes:
    """A baseline file from quantised coefficients.  samp: (h, v) per component; coefs: per component int (blocks down, blocks across, 64)
    in natural order over the MCU-padded component; qts: per component a (64,) table in natural order; dc / ac: (counts, symbols), one
    table of each class for all components.  One interleaved scan, no restart markers."""
    from tests.jpegdec_ref import ZIGZAG
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    out = b"\xff\xd8"
    for i, q in enumerate(qts):
        out += _seg(0xDB, bytes([i]) + bytes(int(q[z]) for z in ZIGZAG))
    out += _seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([len(samp)]) + b"".join(bytes([c + 1, h << 4 | v, c]) for c, (h, v) in enumerate(samp)))
    out += _seg(0xC4, bytes([0x00]) + bytes(dc[0]) + bytes(dc[1])) + _seg(0xC4, bytes([0x10]) + bytes(ac[0]) + bytes(ac[1]))
    out += _seg(0xDA, bytes([len(samp)]) + b"".join(bytes([c + 1, 0]) for c in range(len(samp))) + bytes((0, 63, 0)))
    dct, act = _code_table(*dc), _code_table(*ac)
    bits, pred = [], [0] * len(samp)

    def put(code, n):
        if n:
            bits.append(f"{code:0{n}b}")

    def value(v):
        n = int(abs(v)).bit_length()
        return n, (v if v >= 0 else v + (1 << n) - 1)

    for my in range(mcuy):
        for mx in range(mcux):
            for c, (h, v) in enumerate(samp):
                for u in range(h * v):
                    blk = [int(x) for x in coefs[c][my * v + u // h, mx * h + u % h][ZIGZAG]]
                    n, e = value(blk[0] - pred[c])
                    pred[c] = blk[0]
                    put(*dct[n])
                    put(e, n)
                    run = 0
                    for k in range(1, 64):
                        if blk[k] == 0:
                            run += 1
                            continue
                        while run > 15:
                            put(*act[0xF0])
                            run -= 16
                        n, e = value(blk[k])
                        put(*act[run << 4 | n])
                        put(e, n)
                        run = 0
                    if run:
                        put(*act[0])
    s = "".join(bits)
    s += "1" * (-len(s) % 8)
    scan = int(s, 2).to_bytes(len(s) // 8, "big").replace(b"\xff", b"\xff\x00")
    return out + scan + b"\xff\xd9"
