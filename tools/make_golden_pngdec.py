"""Writes tests/golden/pngdec_cases.npz: the files of the PNG decoder's test cases (tests/pngdec_cases.py builds them with Pillow, zlib
and the tests' own writers) and, per file, what np.array(Image.open(..).convert("RGB")) gave here: the pixels (a SHA-256 for the large
cases), or the text of the error Pillow raised.  Every file of the accepted class is first held to tests.pngdec_ref and to zlib.

usage: python tools/make_golden_pngdec.py
"""
import hashlib
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pngdec_cases as PC, pngdec_ref as R  # noqa: E402


def main():
    files = PC.build()
    assert set(files) == set(PC.CASES) | set(PC.FALLBACK) | set(PC.FLAGGED), set(files) ^ (set(PC.CASES) | set(PC.FALLBACK) | set(PC.FLAGGED))
    out = {}
    for name, data in files.items():
        out[f"{name}.file"] = np.frombuffer(data, np.uint8)
        try:
            px = R.pillow_pixels(data)
        except Exception as e:
            assert name not in PC.CASES, (name, e)
            out[f"{name}.error"] = np.frombuffer(str(e).encode(), np.uint8)
            print(f"{name:18s} {len(data):7d} bytes  Pillow raises: {e}")
            continue
        if name in PC.CASES:
            p = R.parse(data)
            assert zlib.decompress(p.stream) == R.inflate(p.stream, p.raw_bytes, p.wbits), name
            assert np.array_equal(R.decode(data), px), name
        if name in PC.HASHED:
            out[f"{name}.sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest(), np.uint8)
            out[f"{name}.shape"] = np.array(px.shape, np.int64)
        else:
            out[f"{name}.rgb"] = px
        print(f"{name:18s} {len(data):7d} bytes  {px.shape[0]}x{px.shape[1]}")
    np.savez_compressed(PC.GOLDEN, **out)
    print(f"{PC.GOLDEN}: {os.path.getsize(PC.GOLDEN)} bytes, {len(files)} files")


if __name__ == "__main__":
    main()
