"""Writes tests/golden/jpegprog_cases.npz: the files of the progressive JPEG decoder's test cases (tests/jpegprog_cases.py) and the pixels
np.array(Image.open(..).convert("RGB")) gives for them (Pillow 12.2.0).  uint8 arrays only; `long` keeps the SHA-256 of its pixels; a file
Pillow raises for keeps a `.raises` entry instead of pixels.  Every case is asserted to have the property it is named for.
usage: python tools/make_golden_jpegprog.py
"""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpeg_cases as JC, jpegprog_cases as PC, jpegprog_ref as P  # noqa: E402


def content(name, h, w, mode):
    seed = sorted(PC.CASES).index(name) + 300
    rng = np.random.default_rng(seed)
    if name == "const.gray":
        return np.full((h, w), 77, np.uint8)
    if name == "magnitudes":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, -1)
    if name == "runs":
        y, x = np.mgrid[0:h, 0:w]
        texture = np.where(y < 32, 20 * (1 - 2 * ((x + y) % 2)), 45 * (1 - 2 * (x % 2)))
        return np.clip(JC.smooth(h, w, 2).astype(np.int64) // 4 + 96 + texture[..., None], 0, 255).astype(np.uint8)
    if name == "long":
        return np.clip(JC.smooth(h, w, 1).astype(np.int64) + np.random.default_rng(7).integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)
    if name == "rst":                              # smooth with a little noise: EOB runs that the restart interval cuts
        return np.clip(JC.smooth(h, w, 3).astype(np.int64) + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    return rng.integers(0, 256, (h, w) if mode == "L" else (h, w, 3), dtype=np.uint8)


def save(arr, sub, q, **opts):
    buf = io.BytesIO()
    if sub == "L":
        Image.fromarray(arr, "L").save(buf, format="JPEG", quality=q, progressive=True, **opts)
    else:
        Image.fromarray(arr).save(buf, format="JPEG", quality=q, subsampling=sub, progressive=True, **opts)
    return buf.getvalue()


def pillow(data):
    try:
        return P.pillow_pixels(data)
    except Exception:
        return None


def writer_coefs(samp, H, W, seed, dc=200, ac=40, density=0.25):
    """Random sparse coefficients over the MCU-padded grids: small enough for the IDCT to stay in range with a flat table of 4."""
    rng = np.random.default_rng(seed)
    hmax, vmax = samp[0]
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    out = []
    for h, v in samp:
        c = np.zeros((mcuy * v, mcux * h, 64), np.int64)
        c[..., 0] = rng.integers(-dc, dc + 1, c.shape[:2])
        body = rng.integers(-ac, ac + 1, c.shape[:2] + (63,)) * (rng.random(c.shape[:2] + (63,)) < density)
        body[..., 20:] //= 8
        c[..., 1:] = body
        out.append(c)
    return out


def main():
    from gan_variant_research_amd.dataio import parse_jpeg, parse_jpeg_progressive
    out, counters = {}, {}

    def keep(name, data, sha_only=False):
        px = pillow(data)
        out[f"{name}.file"] = np.frombuffer(data, np.uint8)
        if px is None:
            out[f"{name}.raises"] = np.ones(1, np.uint8)
        elif sha_only:
            out[f"{name}.sha256"] = np.frombuffer(hashlib.sha256(px.tobytes()).digest(), np.uint8)
        else:
            out[f"{name}.rgb"] = px
        return px

    def accepted(name, data, sha_only=False):
        px = keep(name, data, sha_only)
        st = P.stages(data, counters.setdefault(name, {}))
        assert px is not None and np.array_equal(st.pixels, px) and not st.extreme, name
        assert parse_jpeg_progressive(data) is not None and parse_jpeg(data) is None, name

    for name, (h, w, sub, q, opts) in PC.CASES.items():
        accepted(name, save(content(name, h, w, sub), sub, q, **dict(opts)), name == "long")
    q4 = np.full(64, 4, np.int64)
    S420, S444 = [(2, 2), (1, 1), (1, 1)], [(1, 1)] * 3
    geometry = {"dc_split": (17, 33, S420), "spectral_only": (9, 17, S444), "deep": (17, 15, S420), "tables4": (16, 16, S444), "dri_change": (24, 40, S420),
                "order": (9, 33, [(2, 1), (1, 1), (1, 1)]), "tables20": (17, 33, S420)}
    for i, name in enumerate(PC.WRITER):
        H, W, samp = geometry[name]
        accepted(name, PC.write_progressive(H, W, samp, writer_coefs(samp, H, W, 40 + i), [q4] * 3, PC.script_of(3, name)))

    # ---- what the cases are for
    cnt = lambda n, k: counters[n][k]
    assert cnt("const.gray", "eobrun_across_blocks") >= 1, "const.gray: no long EOB run"
    assert cnt("rst", "eobrun_cut_by_restart") >= 1, "rst: no EOB run ends at a restart"
    assert cnt("runs", "zrl_refine") >= 1, ("runs", counters["runs"])
    for k in P.COUNTERS:                           # every path is reached by some case
        assert any(c[k] for c in counters.values()), k
    assert cnt("ragged.9x33.420", "grid_narrower") and cnt("ragged.17x15.420", "grid_shorter")
    t20 = parse_jpeg_progressive(out["tables20.file"].tobytes())
    used = [[max(s["tab"]) for s in t20["scans"] if s["level"] == lv] for lv in (0, 1)]
    assert len(t20["versions"]) == 25 and all(min(v) < 16 <= max(v) for v in used), ("tables20: versions", used)
    d = out["stuffing.file"].tobytes()
    assert any(b"\xff\x00" in d[b:e] for b, e in PC.scan_ranges(d)), "stuffing: no stuffed byte"
    assert all(len(sc.segments) == 64 for sc in P.parse(out["rst_wrap.file"].tobytes()).scans if sc.comp >= 0), "rst_wrap: one block per segment"

    # ---- files the parser must leave to Pillow
    H, W = 16, 24
    co = writer_coefs(S444, H, W, 60)
    S = lambda comps, Ss, Se, Ah, Al: dict(comps=comps, Ss=Ss, Se=Se, Ah=Ah, Al=Al)
    every = [0, 1, 2]
    full = [S(every, 0, 0, 0, 0)] + [S([c], 1, 63, 0, 0) for c in every]
    fb = {
        "short_of_al0": PC.write_progressive(H, W, S444, co, [q4] * 3, [S(every, 0, 0, 0, 0)] + [S([c], 1, 63, 0, 1) for c in every]),
        "no_ac_scan": PC.write_progressive(H, W, S444, co, [q4] * 3, full[:3]),
        "ac_before_dc": PC.write_progressive(H, W, S444, co, [q4] * 3, [S([0], 1, 63, 0, 0)] + full[:1] + full[2:]),
        "ac_two_components": PC.write_progressive(H, W, S444, co, [q4] * 3, full[:1] + [S([0, 1], 1, 63, 0, 0), S([2], 1, 63, 0, 0)]),
        "scans65": PC.write_progressive(8, 8, [(1, 1)], writer_coefs([(1, 1)], 8, 8, 61), [q4], [S([0], 0, 0, 0, 0)] + [S([0], k, k, 0, 0) for k in range(1, 63)]
                                        + [S([0], 63, 63, 0, 1), S([0], 63, 63, 1, 0)]),
        "s411": PC.write_progressive(10, 40, [(4, 1), (1, 1), (1, 1)], writer_coefs([(4, 1), (1, 1), (1, 1)], 10, 40, 62), [q4] * 3, full),
        "adobe": PC.write_progressive(H, W, S444, co, [q4] * 3, full, adobe=True),
        "arithmetic": out["mcu.444.file"].tobytes().replace(b"\xff\xc2", b"\xff\xca", 1),
    }
    rst = out["rst.file"].tobytes()
    fb["truncated"] = rst[:len(rst) * 6 // 10]
    assert len(P.parse(fb["scans65"]).scans) == 65
    for name in PC.FALLBACK:
        keep(name, fb[name])
        assert parse_jpeg_progressive(fb[name]) is None and parse_jpeg(fb[name]) is None, f"{name}: a parser takes it"
    assert "truncated.raises" in out

    # ---- files the parser takes and the kernels must flag
    sparse = writer_coefs(S444, H, W, 63, density=0.05)
    two = full[:1] + [S([c], 1, 63, 0, 1) for c in every] + [S([c], 1, 63, 1, 0) for c in every]
    fl = {"crafted.s2": PC.write_progressive(H, W, S444, sparse, [q4] * 3, two, s2=True),
          "crafted.eobrun": PC.write_progressive(H, W, S444, sparse, [q4] * 3, two, extra_eobrun=5)}
    big = [c.copy() for c in sparse]
    big[0][0, 1, 0] = 40000                          # 5000 << 3 leaves int16
    fl["crafted.range"] = PC.write_progressive(H, W, S444, big, [np.ones(64, np.int64)] * 3, PC.script_of(3, "deep"))
    for seed in range(1000):
        v = PC.corrupted(rst, seed)
        if parse_jpeg_progressive(v) is None:
            continue
        try:
            P.decode(v)
            continue
        except P.Corrupt:
            pass
        fl["corrupt"] = v
        out["corrupt.seed"] = np.array([seed], np.int64)
        break
    for name, word in PC.FLAGGED.items():
        keep(name, fl[name])
        assert parse_jpeg_progressive(fl[name]) is not None, f"{name}: the parser refuses it"
        try:
            P.decode(fl[name])
            raise AssertionError(f"{name}: the reference decodes it")
        except P.Corrupt as e:
            assert word is None or e.word == word, (name, e.word)
    os.makedirs(os.path.dirname(PC.GOLDEN), exist_ok=True)
    np.savez_compressed(PC.GOLDEN, **out)
    print(f"wrote {PC.GOLDEN}: {os.path.getsize(PC.GOLDEN)} bytes, {len(out)} arrays; corrupt seed {int(out['corrupt.seed'][0])}")
    print({n: {k: v for k, v in c.items() if v} for n, c in counters.items()})


if __name__ == "__main__":
    main()
