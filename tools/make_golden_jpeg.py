"""Writes tests/golden/jpeg_cases.npz: the inputs of the JPEG encoder's test cases (tests/jpeg_cases.py) and the files Pillow writes
for them with save(format="JPEG", quality=q, subsampling=0, optimize=True) (GAN_Variant1/generate_folder.py:252).  uint8 arrays only.
The noise seed of the 8 x 8 case is searched so that its scan is a whole number of bytes (no padding bits); the file must also hold a
scan that is not, a scan with a stuffed 0xFF and, at q 30 and q 1, AC tables with the ZRL symbol 0xF0 -- asserted here and in the tests.
usage: python tools/make_golden_jpeg.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpeg_cases as JC, jpeg_ref as R  # noqa: E402


smooth = JC.smooth


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def build():
    seed = next(s for s in range(1000) if R.stages(noise(8, 8, s), 95).nbits % 8 == 0)
    yy, xx = np.mgrid[0:16, 0:16]
    y64, x64 = np.mgrid[0:64, 0:64]
    # a gentle gradient under two faint high-frequency textures: a +-20 checkerboard (only the last zig-zag coefficient survives q 30) and
    # +-45 one-pixel stripes (only coefficient 28 survives q 1), so both qualities code runs of more than 15 zeros
    texture = np.where(y64 < 32, 20 * (1 - 2 * ((x64 + y64) % 2)), 45 * (1 - 2 * (x64 % 2)))
    runs = np.clip(smooth(64, 64, 2).astype(np.int64) // 4 + 96 + texture[..., None], 0, 255).astype(np.uint8)
    return {
        "pixel": np.array([[[[200, 30, 99]]]], np.uint8),
        "mcu": noise(8, 8, seed)[None],
        "ragged": np.stack([noise(9, 33, 11), noise(9, 33, 12)]),
        "batch": np.stack([noise(16, 24, 21), smooth(16, 24), np.full((16, 24, 3), 77, np.uint8)]),
        "const": np.full((1, 32, 32, 3), 200, np.uint8),
        "checker": np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[None, :, :, None], 3, -1),
        "runs": runs[None],
        "stuffing": noise(64, 64, 31)[None],
        "long": JC.long_input(),
    }


def main():
    out = {}
    for name, batch in build().items():
        shape, qs = JC.CASES[name]
        assert batch.shape == shape + (3,) and batch.dtype == np.uint8, (name, batch.shape)
        if name == "long":                       # regenerated from its seed by tests/jpeg_cases.py; only its digest is stored
            import hashlib
            out["long.sha256"] = np.frombuffer(hashlib.sha256(batch.tobytes()).digest(), np.uint8)
        else:
            out[f"{name}.rgb"] = batch
        for q in qs:
            for b, im in enumerate(batch):
                out[f"{name}.q{q}.{b}"] = np.frombuffer(R.pillow_bytes(im, q), np.uint8)
    for q in JC.CASES["runs"][1]:
        assert any(t >> 4 == 1 and 0xF0 in vals for t, _, vals in R.split_file(out[f"runs.q{q}.0"].tobytes()).tables), f"no ZRL at q {q}"
    assert b"\xff\x00" in R.split_file(out["stuffing.q95.0"].tobytes()).scan
    os.makedirs(os.path.dirname(JC.GOLDEN), exist_ok=True)
    np.savez_compressed(JC.GOLDEN, **out)
    print(f"wrote {JC.GOLDEN}: {os.path.getsize(JC.GOLDEN)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
