"""Inference I/O, old path against new path in the same process (256x256, bf16, B = 1, 4, 16).

(a) output path: inference.stylize + download + host permute to HWC   vs   inference.stylize_hwc + one contiguous download
(b) folder path: inference.stylize_folder on 64 seeded PNGs of mixed sizes, host I/O vs device I/O (images/s, decode and JPEG encode included)
(c) JPEG encode (--jpeg): the folder path at batch 16 on two folders (the mixed PNGs; 256 JPEGs of 256 x 256), device I/O with serial PIL
    against PIL on a thread pool (io_threads 4, 16) against the device encoder (device_jpeg, io_threads 1, 4, 16); same files every mode
(d) JPEG decode (--decode): the same two folders at batch 16 with device_jpeg: PIL decoding serially and on a pool (io_threads 4, 16)
    against the device decoder (device_decode, decode_chunk 16 / 64 / 256; other formats still go through PIL); same files every mode

(e) PNG decode (--png): the mixed PNGs and 256 PNGs of 256 x 256 (the JPEG folder's images) at batch 16 with device_jpeg: PIL decoding
    serially and on a pool (io_threads 4, 16) against the device decoder (device_png, decode_chunk 16 / 64 / 256); same files every mode

(f) progressive JPEG decode (--progressive): 256 progressive JPEGs of 256 x 256 (the JPEG folder's images) at batch 16 with device_jpeg: PIL
    decoding serially and on a pool (io_threads 4, 16) against device_progressive (with device_decode) at decode_chunk 64 / 256; same files every mode

(g, h, i) the archive (--zip): 256 JPEGs of 256 x 256 at batch 16 with device_jpeg and device_decode (decode_chunk 256), from the first read
    to the closed images.zip: (g) stylize_folder into a folder, then zipfile (stored) over that folder; (h) zip_path with the files from
    encode() and zlib's CRC on the host; (i) zip_path with encode_block (files and CRC-32 from the device); same archive bytes every mode

Every shape is warmed up; the two paths are then timed in rotation for --rounds rounds (a host clock around work that ends in a device
synchronise: each call ends in a download); the median round and the spread (min .. max) are reported.  The outputs of the two paths
are compared before anything is timed.
usage: bench_stylize.py [--size 256] [--batches 1,4,16] [--calls 40] [--rounds 5] [--photos 64] [--out FILE] [--jpeg] [--only-jpeg] [--decode] [--only-decode] [--png] [--only-png] [--progressive] [--only-progressive] [--zip] [--only-zip]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_variant_research_amd import BF16, cut as C, inference as I  # noqa: E402


def make_folder(root: Path, n: int, seed: int = 0):
    """n PNGs of mixed sizes (120 .. 640 pixels a side) under root and root/sub, smooth content plus noise, from a seed."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    (root / "sub").mkdir(parents=True, exist_ok=True)
    for i in range(n):
        h, w = (int(v) for v in rng.integers(120, 641, 2))
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([127 + 120 * np.sin(yy / 17.0 + c + i) * np.cos(xx / 23.0 - c) for c in range(3)], -1)
        img = np.clip(base + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(root / ("sub" if i % 4 == 0 else ".") / f"p{i:03d}.png")


def make_jpeg_folder(root: Path, n: int, size: int = 256, seed: int = 1, png: bool = False, progressive: bool = False):
    """n JPEGs of size x size under root: the realistic input (the reference's photo_jpg folder).  png: the same images as PNGs;
    progressive: the same images saved with Pillow's progressive scan script."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    root.mkdir(parents=True, exist_ok=True)
    yy, xx = np.mgrid[0:size, 0:size]
    for i in range(n):
        base = np.stack([127 + 120 * np.sin(yy / (11.0 + i % 7) + c + i) * np.cos(xx / (19.0 + i % 5) - c) for c in range(3)], -1)
        img = np.clip(base + rng.integers(-20, 21, (size, size, 3)), 0, 255).astype(np.uint8)
        if png:
            Image.fromarray(img).save(root / f"q{i:03d}.png")
        else:
            Image.fromarray(img).save(root / f"q{i:03d}.jpg", quality=90, progressive=progressive)


JPEG_MODES = (("a  device_io, serial PIL", dict()), ("b  PIL pool, io_threads 4", dict(io_threads=4)), ("b  PIL pool, io_threads 16", dict(io_threads=16)),
              ("c  device_jpeg, io_threads 1", dict(device_jpeg=True)), ("c  device_jpeg, io_threads 4", dict(device_jpeg=True, io_threads=4)),
              ("c  device_jpeg, io_threads 16", dict(device_jpeg=True, io_threads=16)))


DECODE_MODES = (("a  PIL serial", dict()), ("b  PIL pool, io_threads 4", dict(io_threads=4)), ("b  PIL pool, io_threads 16", dict(io_threads=16)),
                ("d  device_decode, chunk 16", dict(device_decode=True, decode_chunk=16)), ("d  device_decode, chunk 64", dict(device_decode=True, decode_chunk=64)),
                ("d  device_decode, chunk 256", dict(device_decode=True, decode_chunk=256)),
                ("d  device_decode, chunk 256, io_threads 4", dict(device_decode=True, decode_chunk=256, io_threads=4)))


PNG_MODES = tuple((name.replace("device_decode", "device_png").replace("d  ", "e  "), {("device_png" if k == "device_decode" else k): v for k, v in kw.items()})
                  for name, kw in DECODE_MODES)


def decode_section(G, dev, S, rounds, photos, tmp: Path, png: bool = False):
    """(d), or (e) with png: every mode writes the same files (checked first), then the modes run in rotation; images/s, median [min .. max]."""
    tag, MODES, attr = ("e", PNG_MODES, "_png_dec") if png else ("d", DECODE_MODES, "_jpeg_dec")
    lines = [f"# ({tag}) images/s over one pass of a folder, batch 16, {S}x{S}, device_jpeg, decode and encode included; median of {rounds} alternating rounds [min .. max]"]
    second = (f"256 PNGs of {S}x{S}", tmp / "pngs", 256) if png else (f"256 JPEGs of {S}x{S}", tmp / "jpegs", 256)
    if not second[1].exists():
        make_jpeg_folder(second[1], 256, S, png=png)
    for label, src, n in ((f"{photos} PNGs of mixed sizes", tmp / "photos", photos), second):
        d = tag

        def mode(i, kw):
            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert I.stylize_folder(G, str(src), str(tmp / f"{d}_{src.name}_{i}"), device=str(dev), img_size=S, batch=16, device_io=True, device_jpeg=True, **kw) == n
                torch.cuda.synchronize()
                return n / (time.perf_counter() - t0)
            return run
        paths = {name: mode(i, kw) for i, (name, kw) in enumerate(MODES)}
        for fn in paths.values():
            fn()
        outs = [{p.name: p.read_bytes() for p in (tmp / f"{d}_{src.name}_{i}").rglob("*.jpg")} for i in range(len(MODES))]
        assert len(outs[0]) == n and all(o == outs[0] for o in outs), "the modes wrote different files"
        times = rotate(paths, rounds)
        lines.append(f"# {label}; the device decoder's counts since the start of the section: {getattr(G, attr).stats}")
        for name, v in times.items():
            lines.append(f"({d}) {name:44s} {statistics.median(v):8.1f} images/s [{min(v):8.1f} .. {max(v):8.1f}]")
        best_pool = max(max(times[k]) for k in times if k.startswith("b"))
        for name, v in times.items():
            if name.startswith(d):
                verdict = "beats" if min(v) > best_pool else "does not beat"
                lines.append(f"({d}) {name[3:]}: {verdict} the PIL pools beyond both spreads (its min {min(v):.1f} vs their max {best_pool:.1f})")
        for ln in lines[-(2 * len(MODES) - 2):]:
            print(ln, flush=True)
    return lines


PROGRESSIVE_MODES = (("a  PIL serial", dict()), ("b  PIL pool, io_threads 4", dict(io_threads=4)), ("b  PIL pool, io_threads 16", dict(io_threads=16)),
                     ("f  device_progressive, chunk 64", dict(device_decode=True, device_progressive=True, decode_chunk=64)),
                     ("f  device_progressive, chunk 256", dict(device_decode=True, device_progressive=True, decode_chunk=256)))


def progressive_section(G, dev, S, rounds, tmp: Path):
    """(f): every mode writes the same files (checked first), then the modes run in rotation; images/s, median [min .. max]."""
    n, src = 256, tmp / "progressive"
    make_jpeg_folder(src, n, S, progressive=True)
    lines = [f"# (f) images/s over one pass of a folder of {n} progressive JPEGs of {S}x{S}, batch 16, device_jpeg, decode and encode included; "
             f"median of {rounds} alternating rounds [min .. max]"]

    def mode(i, kw):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert I.stylize_folder(G, str(src), str(tmp / f"f_{i}"), device=str(dev), img_size=S, batch=16, device_io=True, device_jpeg=True, **kw) == n
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)
        return run
    paths = {name: mode(i, kw) for i, (name, kw) in enumerate(PROGRESSIVE_MODES)}
    for fn in paths.values():
        fn()
    outs = [{p.name: p.read_bytes() for p in (tmp / f"f_{i}").rglob("*.jpg")} for i in range(len(PROGRESSIVE_MODES))]
    assert len(outs[0]) == n and all(o == outs[0] for o in outs), "the modes wrote different files"
    times = rotate(paths, rounds)
    lines.append(f"# the decoder's counts since the start of the section: {G._jpeg_dec.stats}, progressive among them: {G._jpeg_dec.progressive_stats}")
    for name, v in times.items():
        lines.append(f"(f) {name:44s} {statistics.median(v):8.1f} images/s [{min(v):8.1f} .. {max(v):8.1f}]")
    for th in ("serial", "pool, io_threads 4", "pool, io_threads 16"):
        ref = times[("a  PIL " if th == "serial" else "b  PIL ") + th]
        for name, v in times.items():
            if name.startswith("f"):
                verdict = "faster than" if min(v) > max(ref) else "slower than" if max(v) < min(ref) else "not apart from"
                lines.append(f"(f) {name[3:]}: {verdict} PIL {th} beyond both spreads ([{min(v):.1f} .. {max(v):.1f}] vs [{min(ref):.1f} .. {max(ref):.1f}])")
    for ln in lines:
        print(ln, flush=True)
    return lines


def zip_section(G, dev, S, rounds, tmp: Path):
    """(g), (h), (i): every mode leaves the same archive bytes (checked first), then the modes run in rotation; images/s, median [min .. max]."""
    import zipfile
    n, src = 256, tmp / "jpegs"
    if not src.exists():
        make_jpeg_folder(src, n, S)
    kw = dict(device=str(dev), img_size=S, batch=16, device_io=True, device_jpeg=True, device_decode=True, decode_chunk=256)
    device_block = I.JpegEncoder.encode_block

    def host_block(self, batch):
        """What a writer without the device's files has: encode()'s per-file assembly, joined, and no CRC (the writer runs zlib's)."""
        files = self.encode(batch)
        off = [0]
        for f in files:
            off.append(off[-1] + len(f))
        return b"".join(files), off, None

    def today(out):
        assert I.stylize_folder(G, str(src), str(tmp / "g_dir"), **kw) == n
        with zipfile.ZipFile(out, "w", zipfile.ZIP_STORED) as z:
            for p in sorted((tmp / "g_dir").rglob("*.jpg")):
                z.writestr(zipfile.ZipInfo(p.relative_to(tmp / "g_dir").as_posix(), date_time=(1980, 1, 1, 0, 0, 0)), p.read_bytes())

    def direct(block_fn):
        def go(out):
            I.JpegEncoder.encode_block = block_fn
            try:
                assert I.stylize_folder(G, str(src), zip_path=str(out), **kw) == n
            finally:
                I.JpegEncoder.encode_block = device_block
        return go
    MODES = (("g  folder, then zipfile over it", today), ("h  zip_path, encode() + host CRC", direct(host_block)), ("i  zip_path, encode_block", direct(device_block)))

    def mode(i, go):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            go(tmp / f"zip_{i}.zip")
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)
        return run
    paths = {name: mode(i, go) for i, (name, go) in enumerate(MODES)}
    for fn in paths.values():
        fn()
    outs = [(tmp / f"zip_{i}.zip").read_bytes() for i in range(len(MODES))]
    assert all(o == outs[0] for o in outs), "the modes wrote different archives"
    with zipfile.ZipFile(tmp / "zip_2.zip") as z:
        assert z.testzip() is None and len(z.infolist()) == n
    times = rotate(paths, rounds)
    lines = [f"# (g, h, i) images/s from the first read to the closed archive: {n} JPEGs of {S}x{S}, batch 16, device_jpeg, device_decode (chunk 256); "
             f"median of {rounds} alternating rounds [min .. max]; archive of {len(outs[0])} bytes, identical in every mode"]
    for name, v in times.items():
        lines.append(f"({name[0]}) {name[3:]:36s} {statistics.median(v):8.1f} images/s [{min(v):8.1f} .. {max(v):8.1f}]")
    keys = list(times)
    for a, b in ((2, 1), (2, 0), (1, 0)):
        va, vb = times[keys[a]], times[keys[b]]
        verdict = "faster than" if min(va) > max(vb) else "slower than" if max(va) < min(vb) else "not apart from"
        lines.append(f"({keys[a][0]}) {verdict} ({keys[b][0]}) beyond both spreads ([{min(va):.1f} .. {max(va):.1f}] vs [{min(vb):.1f} .. {max(vb):.1f}])")
    for ln in lines:
        print(ln, flush=True)
    return lines


def jpeg_section(G, dev, S, rounds, photos, tmp: Path):
    """(c): every mode writes the same files (checked first), then the modes run in rotation; images/s, median [min .. max]."""
    lines = [f"# (c) images/s over one pass of a folder, batch 16, {S}x{S}, decode and JPEG encode included; median of {rounds} alternating rounds [min .. max]"]
    make_jpeg_folder(tmp / "jpegs", 256, S)
    for label, src, n in ((f"{photos} PNGs of mixed sizes", tmp / "photos", photos), (f"256 JPEGs of {S}x{S}", tmp / "jpegs", 256)):
        def mode(i, kw):
            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert I.stylize_folder(G, str(src), str(tmp / f"c_{src.name}_{i}"), device=str(dev), img_size=S, batch=16, device_io=True, **kw) == n
                torch.cuda.synchronize()
                return n / (time.perf_counter() - t0)
            return run
        paths = {name: mode(i, kw) for i, (name, kw) in enumerate(JPEG_MODES)}
        for fn in paths.values():
            fn()
        outs = [{p.name: p.read_bytes() for p in (tmp / f"c_{src.name}_{i}").rglob("*.jpg")} for i in range(len(JPEG_MODES))]
        assert len(outs[0]) == n and all(o == outs[0] for o in outs), "the modes wrote different files"
        times = rotate(paths, rounds)
        lines.append(f"# {label}")
        for name, v in times.items():
            lines.append(f"(c) {name:30s} {statistics.median(v):8.1f} images/s [{min(v):8.1f} .. {max(v):8.1f}]")
        for th in (4, 16):
            b, c = times[f"b  PIL pool, io_threads {th}"], times[f"c  device_jpeg, io_threads {th}"]
            verdict = "beats" if min(c) > max(b) else "does not beat"
            lines.append(f"(c) io_threads {th:2d}: device_jpeg {verdict} the PIL pool beyond both spreads (min c {min(c):.1f} vs max b {max(b):.1f})")
        for ln in lines[-(len(JPEG_MODES) + 3):]:
            print(ln, flush=True)
    return lines


def rotate(paths, rounds):
    """paths: name -> callable returning the seconds one round of it took.  Runs them in rotation; name -> list of round times."""
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(fn())
    return times


def line(label, unit, vals, better_is_lower):
    a, b = (statistics.median(vals[k]) for k in ("old", "new"))
    sa, sb = ((min(vals[k]), max(vals[k])) for k in ("old", "new"))
    apart = sb[1] < sa[0] if better_is_lower else sb[0] > sa[1]          # every new round beats every old round
    gain = a / b if better_is_lower else b / a
    verdict = f"new/old speed {gain:.3f}x" + ("" if apart else "  (rounds overlap: not faster beyond the spread)")
    return (f"{label}: old {a:.3f} {unit} [{sa[0]:.3f} .. {sa[1]:.3f}]   new {b:.3f} {unit} [{sb[0]:.3f} .. {sb[1]:.3f}]   {verdict}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--photos", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--jpeg", action="store_true", help="also run section (c)")
    ap.add_argument("--only-jpeg", action="store_true", help="run section (c) alone")
    ap.add_argument("--decode", action="store_true", help="also run section (d)")
    ap.add_argument("--only-decode", action="store_true", help="run section (d) alone")
    ap.add_argument("--png", action="store_true", help="also run section (e)")
    ap.add_argument("--only-png", action="store_true", help="run section (e) alone")
    ap.add_argument("--progressive", action="store_true", help="also run section (f)")
    ap.add_argument("--only-progressive", action="store_true", help="run section (f) alone")
    ap.add_argument("--zip", action="store_true", help="also run sections (g, h, i)")
    ap.add_argument("--only-zip", action="store_true", help="run sections (g, h, i) alone")
    a = ap.parse_args()
    a.zip = a.zip or a.only_zip
    a.decode = a.decode or a.only_decode
    a.png = a.png or a.only_png
    a.progressive = a.progressive or a.only_progressive
    assert torch.cuda.is_available(), "bench_stylize.py measures on the GPU"
    dev, S = torch.device("cuda:0"), a.size
    C.set_seed(0)
    G = C.ResNetGenerator(3, 3, 64, 9).to(dev).eval()
    for p in G.parameters():
        p.requires_grad_(False)
    G.compute_dtype = BF16
    lines = [f"# tools/bench_stylize.py --size {S} --batches {a.batches} --calls {a.calls} --rounds {a.rounds} --photos {a.photos}"
             + (" --only-jpeg" if a.only_jpeg else " --jpeg" if a.jpeg else "") + (" --only-decode" if a.only_decode else " --decode" if a.decode else "")
             + (" --only-png" if a.only_png else " --png" if a.png else "") + (" --only-progressive" if a.only_progressive else " --progressive" if a.progressive else "")
             + (" --only-zip" if a.only_zip else " --zip" if a.zip else ""),
             f"# generator ngf 64, 9 blocks, bf16 operands, eager launches; median of {a.rounds} alternating rounds [min .. max]"]
    only = a.only_jpeg or a.only_decode or a.only_png or a.only_progressive or a.only_zip
    if not only:
        lines.append(f"# (a) ms per call of {a.calls} consecutive calls, each ending in the download of the uint8 HWC batch to the host")
    old_out = lambda x: I.stylize(G, x).cpu().permute(0, 2, 3, 1).contiguous()
    new_out = lambda x: I.stylize_hwc(G, x).cpu()
    batches = [] if only else [int(v) for v in a.batches.split(",")]
    for B in batches:
        x = (torch.rand(B, 3, S, S) * 2 - 1).to(dev)
        for _ in range(3):
            yo, yn = old_out(x), new_out(x)
        assert torch.equal(yo, yn), "the two output paths differ"

        def timed(fn):
            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn(x)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / a.calls * 1e3
            return run
        lines.append(line(f"(a) B={B:2d} {S}x{S}", "ms", rotate({"old": timed(old_out), "new": timed(new_out)}, a.rounds), True))
        print(lines[-1], flush=True)
    if not only:
        lines.append(f"# (b) images/s over one pass of a folder of {a.photos} PNGs (120 .. 640 pixels a side), PNG decode and JPEG encode included")
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        make_folder(tmp / "photos", a.photos)
        for B in batches:
            def folder(device_io, out):
                def run():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n = I.stylize_folder(G, str(tmp / "photos"), str(tmp / out), device=str(dev), img_size=S, batch=B, device_io=device_io)
                    torch.cuda.synchronize()
                    return n / (time.perf_counter() - t0)
                return run
            paths = {"old": folder(False, f"host{B}"), "new": folder(True, f"dev{B}")}
            for fn in paths.values():
                fn()
            ho = {p.name: p.read_bytes() for p in (tmp / f"host{B}").rglob("*.jpg")}
            do = {p.name: p.read_bytes() for p in (tmp / f"dev{B}").rglob("*.jpg")}
            assert len(ho) == a.photos and ho == do, "the two folder paths wrote different files"
            lines.append(line(f"(b) batch={B:2d} {S}x{S}", "images/s", rotate(paths, a.rounds), False))
            print(lines[-1], flush=True)
        if a.jpeg or a.only_jpeg:
            lines += jpeg_section(G, dev, S, a.rounds, a.photos, tmp)
        if a.decode:
            lines += decode_section(G, dev, S, a.rounds, a.photos, tmp)
        if a.png:
            lines += decode_section(G, dev, S, a.rounds, a.photos, tmp, png=True)
        if a.progressive:
            lines += progressive_section(G, dev, S, a.rounds, tmp)
        if a.zip:
            lines += zip_section(G, dev, S, a.rounds, tmp)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
