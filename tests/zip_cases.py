"""TEST INFRASTRUCTURE: the byte ranges the CRC-32 kernel is held to zlib on.

Every length of LENGTHS with three contents -- random bytes, zeros, 0xFF -- laid back to back in one buffer in that order, so that the
starts fall on every residue modulo 16 (checked below).  Zeros make a wrong length or a wrong shift visible: the CRC-32 of n zero bytes
depends on n alone.  The lengths sit around the kernel's seams: 16-byte loads (15, 16, 17), the 256 pieces of a workgroup (255 .. 257
bytes, 4095 .. 4097 = 256 x 16 bytes), and ranges long enough that every lane holds many loads."""
from __future__ import annotations

import zlib
from functools import lru_cache

import numpy as np

LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65537, 1048577)
CONTENTS = ("random", "zeros", "ones")


@lru_cache(maxsize=None)
def table():
    """(buffer uint8, offsets int64 [n + 1], ids [n], zlib's CRC-32 uint32 [n]); computed once, never modified by a test."""
    rng = np.random.default_rng(2024)
    parts, ids = [], []
    for n in LENGTHS:
        for c in CONTENTS:
            parts.append(rng.integers(0, 256, n, dtype=np.uint8) if c == "random" else np.full(n, 0 if c == "zeros" else 255, np.uint8))
            ids.append(f"{c}-{n}")
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    buf = np.concatenate(parts)
    assert {int(o) % 16 for o in offsets[:-1]} == set(range(16)), "the starts do not reach every residue modulo 16"
    want = np.array([zlib.crc32(p.tobytes()) for p in parts], dtype=np.uint32)
    for a in (buf, offsets, want):
        a.setflags(write=False)
    return buf, offsets, ids, want
