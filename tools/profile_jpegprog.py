"""One chunk of 256 JPEGs of 256 x 256 through dataio.JpegDecoder, for a kernel trace of its own:
    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/profile_jpegprog.py --mode MODE
--mode levels   : the images saved progressive, the scans' levels as the parser states them (independent scans side by side)
--mode series   : the same files with every scan on a level of its own (file order): what the levels buy is the difference
--mode baseline : the same images saved as baseline JPEGs, through the baseline entropy kernel
Each mode decodes the chunk --reps times after one warm-up call; the entropy kernel's average in the trace's statistics is the figure.
"""
import argparse
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_variant_research_amd import dataio  # noqa: E402

def images(n, size, progressive):
    from PIL import Image
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:size, 0:size]
    out = []
    for i in range(n):                       # tools/bench_stylize.py make_jpeg_folder's images
        base = np.stack([127 + 120 * np.sin(yy / (11.0 + i % 7) + c + i) * np.cos(xx / (19.0 + i % 5) - c) for c in range(3)], -1)
        img = np.clip(base + rng.integers(-20, 21, (size, size, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=90, progressive=progressive)
        out.append(buf.getvalue())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("levels", "series", "baseline"), default="levels")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    files = images(a.n, a.size, a.mode != "baseline")
    if a.mode == "series":
        parse = dataio.parse_jpeg_progressive

        def in_series(data):
            plan = parse(data)
            if plan is not None:
                for j, sc in enumerate(plan["scans"]):
                    sc["level"] = j
                plan["nlevel"] = len(plan["scans"])
            return plan
        dataio.parse_jpeg_progressive = in_series
    dec = dataio.JpegDecoder("cuda:0", progressive=a.mode != "baseline")
    for _ in range(1 + a.reps):
        got = dec.decode(files)
        torch.cuda.synchronize()
    want = [dataio._decode(io.BytesIO(f)) for f in files[:8]]
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)) and dec.stats["device"] == (1 + a.reps) * a.n, dec.stats
    print(f"{a.mode}: {a.n} files of {a.size}x{a.size}, {1 + a.reps} calls, stats {dec.stats}, progressive {dec.progressive_stats}")


if __name__ == "__main__":
    main()
