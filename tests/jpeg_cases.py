"""TEST INFRASTRUCTURE: the encoder's test cases, read from tests/golden/jpeg_cases.npz (written by tools/make_golden_jpeg.py with
Pillow 12.2.0): per case the uint8 input batch and the bytes Pillow's save(format="JPEG", quality=q, subsampling=0, optimize=True) wrote."""
from __future__ import annotations

import os
from functools import lru_cache

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")

# name -> ((B, H, W), qualities): the smallest shapes at which each stage of the encoder can go wrong
CASES = {
    "pixel": ((1, 1, 1), (95,)),            # one MCU made only of replication
    "mcu": ((1, 8, 8), (95,)),              # no padding of the image; seed chosen so that the scan is a whole number of bytes
    "ragged": ((2, 9, 33), (95,)),          # replication both ways, 2 x 5 MCUs, per-image tables and offsets
    "batch": ((3, 16, 24), (95,)),          # noise / smooth / constant: compaction over streams of very different length
    "const": ((1, 32, 32), (95,)),          # one- and two-symbol tables, every DC difference 0, EOB only
    "checker": ((1, 16, 16), (95, 100)),    # largest magnitudes and bit categories
    "runs": ((1, 64, 64), (30, 1)),         # ZRL (0xF0)
    "stuffing": ((1, 64, 64), (95,)),       # 0xFF bytes in the scan
    "long": ((1, 256, 256), (95,)),         # 3072 blocks: every chunk / workgroup boundary of the scan and the stuffing scatter
}
CASE_IDS = [(name, q) for name, (_, qs) in CASES.items() for q in qs]


@lru_cache(maxsize=None)
def _npz():
    return dict(np.load(GOLDEN))


def smooth(h: int, w: int, k: int = 0) -> np.ndarray:
    y, x = np.mgrid[0:h, 0:w]
    return np.clip(np.stack([128 + 100 * np.sin(x / 9.0 + y / 17.0 + k), 128 + 90 * np.cos(y / 7.0 - k), (x * 3 + y * 2 + 40 * k) % 256], -1), 0, 255).astype(np.uint8)


@lru_cache(maxsize=None)
def long_input() -> np.ndarray:
    """The (1, 256, 256, 3) input of `long`: smooth content plus +-6 noise from a fixed seed.  It is not stored (196 KB that do not
    compress); the golden file keeps its SHA-256, which `rgb` checks, beside Pillow's bytes for it."""
    im = np.clip(smooth(256, 256, 1).astype(np.int64) + np.random.default_rng(7).integers(-6, 7, (256, 256, 3)), 0, 255).astype(np.uint8)
    return im[None]


def rgb(name: str) -> np.ndarray:
    """(B, H, W, 3) uint8."""
    if name == "long":
        import hashlib
        im = long_input()
        assert hashlib.sha256(im.tobytes()).digest() == _npz()["long.sha256"].tobytes(), "the regenerated `long` input is not the one Pillow encoded"
        return im
    return _npz()[f"{name}.rgb"]


def golden(name: str, q: int) -> list:
    """Pillow's files for the case's images, as bytes."""
    z = _npz()
    return [z[f"{name}.q{q}.{b}"].tobytes() for b in range(CASES[name][0][0])]


def fib_like(n: int) -> list:
    fib = [2, 3]
    while len(fib) < n:
        fib.append(fib[-1] + fib[-2] + len(fib))
    return fib[:n]


def fibonacci_hists() -> np.ndarray:
    """(4, 256) histograms whose optimal code lengths exceed 16 before limiting: Fibonacci-like frequencies f[i] = f[i-1] + f[i-2] + i
    (the + i keeps merged sums from tying with the next frequency, which would let libjpeg balance the tree) on 24 .. 30 symbols: in
    order, spread down from symbol 255, with a tail of equal counts, and reversed beside 40 singletons."""
    h = np.zeros((4, 256), np.int64)
    fib = fib_like(30)
    h[0, :24] = fib[:24]
    h[1, 255 - np.arange(30) * 8] = fib[:30]
    h[2, np.arange(26) * 3 + 1] = fib[:26]
    h[2, 200:206] = 5
    h[3, :28] = fib[:28][::-1]
    h[3, 100:140] = 1
    return h
