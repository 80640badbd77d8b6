"""Writes tests/golden/jpegdec_cases.npz: the files of the JPEG decoder's test cases (tests/jpegdec_cases.py) and the pixels
np.array(Image.open(..).convert("RGB")) gives for them.  uint8 arrays only; `long` keeps the SHA-256 of its pixels instead of the pixels.
Every case is asserted to have the property it is named for.
usage: python tools/make_golden_jpegdec.py
"""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpeg_cases as JC, jpegdec_cases as DC, jpegdec_ref as R  # noqa: E402


def noise(h, w, seed, ch=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, ch) if ch > 1 else (h, w), dtype=np.uint8)


def content(name, h, w, mode):
    seed = sorted(DC.CASES).index(name) + 100
    if name == "const":
        return np.full((h, w, 3), 128, np.uint8)       # level-shifted to 0: every DC difference is 0, the first one included
    if name == "magnitudes":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, -1)
    if name == "runs":
        y, x = np.mgrid[0:h, 0:w]
        texture = np.where(y < 32, 20 * (1 - 2 * ((x + y) % 2)), 45 * (1 - 2 * (x % 2)))
        return np.clip(JC.smooth(h, w, 2).astype(np.int64) // 4 + 96 + texture[..., None], 0, 255).astype(np.uint8)
    if name == "long":
        return np.clip(JC.smooth(h, w, 1).astype(np.int64) + np.random.default_rng(7).integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)
    if name in ("rst", "wide"):                    # photographs are smooth: noise on a gradient
        return np.clip(JC.smooth(h, w, 3).astype(np.int64) + np.random.default_rng(seed).integers(-30, 31, (h, w, 3)), 0, 255).astype(np.uint8)
    return noise(h, w, seed, 1 if mode == "L" else 3)


def save(arr, sub, q, **opts):
    buf = io.BytesIO()
    if sub == "L":
        Image.fromarray(arr, "L").save(buf, format="JPEG", quality=q, optimize=opts.pop("optimize", True), **opts)
    else:
        Image.fromarray(arr).save(buf, format="JPEG", quality=q, subsampling=sub, optimize=opts.pop("optimize", True), **opts)
    return buf.getvalue()


def scan_of(data):
    p = R.parse(data)
    return p.segments[0][0], p.segments[-1][1]


def longest_code(data):
    seen = []
    sym = R._Bits.symbol

    def spy(self, table):
        p0 = self.pos
        s = sym(self, table)
        seen.append(self.pos - p0)
        return s
    R._Bits.symbol = spy
    try:
        R.decode(data)
    finally:
        R._Bits.symbol = sym
    return max(seen)


def main():
    from gan_variant_research_amd.dataio import parse_jpeg
    out = {}
    for name, (h, w, sub, q, opts) in DC.CASES.items():
        data = save(content(name, h, w, sub), sub, q, **dict(opts))
        px = R.pillow_pixels(data)
        st = R.stages(data)
        assert px.shape == (h, w, 3) and np.array_equal(st.pixels, px) and not st.extreme, name
        assert parse_jpeg(data) is not None, name
        out[f"{name}.file"] = np.frombuffer(data, np.uint8)
        if name == "long":
            out["long.sha256"] = np.frombuffer(hashlib.sha256(px.tobytes()).digest(), np.uint8)
        else:
            out[f"{name}.rgb"] = px
    f = lambda n: out[f"{n}.file"].tobytes()
    tables = lambda n: {m_b[1][0]: m_b[1] for m_b in R.markers(f(n))[0] if m_b[0] == 0xC4}
    assert all(sum(b[1:17]) == 1 for b in tables("const").values()), "const: tables of more than one symbol"
    assert longest_code(f("std_tables")) > 9, "std_tables: no code longer than the lookahead width"
    assert any(0xF0 in b[17:] for t, b in tables("runs").items() if t >> 4), "runs: no ZRL"
    b, e = scan_of(f("stuffing"))
    assert b"\xff\x00" in f("stuffing")[b:e], "stuffing: no stuffed byte"
    assert len(R.parse(f("rst")).segments) == 4 and R.parse(f("rst")).per == 3, "rst: 12 MCUs in segments of 3"
    assert len(R.parse(f("rst_wrap")).segments) == 64 and R.parse(f("rst_wrap")).per == 1, "rst_wrap: one MCU per segment"
    assert max(int(np.abs(c).max()) for c in R.stages(f("magnitudes")).coefs) >= 512, "magnitudes: small categories only"

    # ---- files the device must hand to Pillow
    buf = io.BytesIO(); Image.fromarray(noise(20, 24, 1)).save(buf, format="JPEG", quality=90, progressive=True)
    fb = {"progressive": buf.getvalue()}
    buf = io.BytesIO(); Image.fromarray(noise(16, 16, 2, 4), "CMYK").save(buf, format="JPEG", quality=90)
    fb["cmyk"] = buf.getvalue()
    std = tables("std_tables")
    dc, ac = (list(std[0x00][1:17]), list(std[0x00][17:])), (list(std[0x10][1:17]), list(std[0x10][17:]))
    rng = np.random.default_rng(5)
    q = np.full(64, 8, np.int64)

    def coefs(bh, bw):
        c = np.zeros((bh, bw, 64), np.int64)
        c[..., 0] = rng.integers(-60, 60, (bh, bw))
        c[..., 1:6] = rng.integers(-9, 10, (bh, bw, 5))
        return c
    fb["s411"] = DC.write_jpeg(10, 40, [(4, 1), (1, 1), (1, 1)], [coefs(2, 8), coefs(2, 2), coefs(2, 2)], [q, q, q], dc, ac)
    d = f("ragged.9x33.444")
    fb["adobe"] = d[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + d[2:]
    buf = io.BytesIO(); Image.fromarray(noise(12, 10, 3)).save(buf, format="PNG")
    fb["png"] = buf.getvalue()
    big = np.zeros((1, 1, 64), np.int64)
    big[0, 0, 0], big[0, 0, 1] = 1000, -900
    zero = np.zeros((1, 1, 64), np.int64)
    fb["crafted"] = DC.write_jpeg(8, 8, [(1, 1)] * 3, [big, zero, zero], [np.full(64, 255, np.int64)] * 3, dc, ac)
    assert parse_jpeg(fb["crafted"]) is not None and R.stages(fb["crafted"]).extreme, "crafted: in range"
    d = f("std_tables")
    b, e = scan_of(d)
    for seed in range(1000):
        r = np.random.default_rng(seed)
        v = bytearray(d)
        for p in r.choice(np.arange(b + 8, e - 8), DC.CORRUPT_BYTES, replace=False):
            v[p] = int(r.integers(1, 255))
        v = bytes(v)
        if parse_jpeg(v) is None:
            continue
        try:
            R.decode(v)
            continue
        except R.Corrupt:
            pass
        try:
            R.pillow_pixels(v)
        except OSError:
            continue
        fb["corrupt"] = v
        break
    for name in DC.FALLBACK:
        px = R.pillow_pixels(fb[name])                # Pillow returns an image for every one of them
        out[f"{name}.file"], out[f"{name}.rgb"] = np.frombuffer(fb[name], np.uint8), px
        if name not in ("crafted", "corrupt"):
            assert parse_jpeg(fb[name]) is None, f"{name}: the parser takes it"
    try:
        R.pillow_pixels(f("rst")[:len(f("rst")) * 6 // 10])
        raise AssertionError("truncated: Pillow decodes it")
    except OSError:
        pass
    os.makedirs(os.path.dirname(DC.GOLDEN), exist_ok=True)
    np.savez_compressed(DC.GOLDEN, **out)
    print(f"wrote {DC.GOLDEN}: {os.path.getsize(DC.GOLDEN)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
