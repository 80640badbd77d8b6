"""What feeding the CUT step from image folders costs: train_cutpp's own step loop (train_cutpp.step_losses) on one trainer
(256x256, batch 16, bf16), its batches coming in rotation from

    fixed               the same two device batches every step, losses read every step   (no host preparation at all: the step alone)
    synthetic           uniform-noise batches drawn on the host, losses read every step  (what --synthetic runs: 2 x 3.1 M floats from one
                        host thread and a pageable upload per step, in series with the step)
    resident            dataio.ImageStore resident on the device, host work in series    (jobs drawn and transform queued between steps)
    resident+overlap    the same, batch k+1 prepared while step k runs                   (what the driver runs on folders)
    streaming           dataio.ImageStore decoding every batch on its thread pool, in series
    streaming+overlap   the same, overlapped
    streaming+dd, streaming+dd+overlap   (--device-decode) the streaming store with device_decode=True: dataio.JpegDecoder decodes every batch
                        (--device-png: the folders hold the same images as PNGs and the +dd stores are built with device_png=True: dataio.PngDecoder)


over N random 256x256 JPEGs per domain written with Pillow into a temporary folder.  Every mode is warmed up, then timed in ROUNDS
alternating rounds of STEPS steps (a multiple of the lazy-R1 period, so every window holds the same work); one JSON line per mode with
the median round and [min .. max], one line per store build, and what the resident store adds to the synthetic and to the fixed rounds
against those rounds' own spread (the overlap was decided by it).

usage: bench_dataio.py [--n 512] [--steps 32] [--rounds 5] [--device-decode | --device-png]
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import default_config  # noqa: E402
from gan_variant_research_amd import cut as C, dataio, train_cutpp as T  # noqa: E402

B, S = 16, 256


def write_jpegs(folder, n, seed, png=False):
    """n photo-like 256x256 JPEGs (low-frequency colour plus noise: a decode cost like a photograph's, not like white noise's)."""
    from PIL import Image
    os.makedirs(folder)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    bases = []
    for i in range(8):
        f = rng.uniform(8.0, 40.0, 6)
        bases.append(np.stack([127 + 120 * np.sin(yy / f[c] + i) * np.cos(xx / f[3 + c] - c) for c in range(3)], -1).astype(np.int16))

    def write(i):
        noise = np.random.default_rng([seed, i]).integers(-20, 21, (S, S, 3), dtype=np.int16)
        img = Image.fromarray(np.clip(bases[i % 8] + noise, 0, 255).astype(np.uint8))
        img.save(os.path.join(folder, f"{i:05d}.png")) if png else img.save(os.path.join(folder, f"{i:05d}.jpg"), quality=90)
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(write, range(n)))
    return sorted(os.path.join(folder, f) for f in os.listdir(folder))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="JPEGs per domain")
    ap.add_argument("--steps", type=int, default=32, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device-decode", action="store_true", help="also build both stores with device_decode=True and time the streaming one")
    ap.add_argument("--device-png", action="store_true", help="the same over PNG folders, the +dd stores built with device_png=True")
    args = ap.parse_args()
    switch = "device_png" if args.device_png else "device_decode"
    args.device_decode = args.device_decode or args.device_png
    assert torch.cuda.is_available(), "bench_dataio needs the GPU"
    dev = torch.device("cuda")
    cfg = default_config()
    C.set_seed(42)
    gen, disc = C.build_models(cfg, "cpu")
    trainer = C.CutTrainer(gen, disc, cfg, B, S, device=dev, amp=True)

    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        paths = {d: write_jpegs(os.path.join(tmp, d), args.n, k, png=args.device_png) for k, d in enumerate(("photos", "monet"))}
        print(json.dumps({"wrote": f"2 x {args.n} {'PNGs' if args.device_png else 'JPEGs'} {S}x{S}", "seconds": round(time.perf_counter() - t0, 2)}), flush=True)
        stores = {}
        kinds = [("resident", None, False), ("streaming", 1, False)] + ([("resident+dd", None, True), ("streaming+dd", 1, True)] if args.device_decode else [])
        for kind, budget, dd in kinds:
            t0 = time.perf_counter()
            stores[kind] = [dataio.ImageStore(paths[d], dev, budget_bytes=budget, **({switch: True} if dd else {})) for d in ("photos", "monet")]
            torch.cuda.synchronize()
            st = stores[kind][0]
            assert st.resident == kind.startswith("resident")
            if dd:
                assert st._decoder.stats["unsupported"] == st._decoder.stats["flagged"] == 0
            print(json.dumps({"store": kind, "images": 2 * args.n, "decoded_MB": round(2 * st.nbytes / 1e6, 1), "workers": st.workers,
                              "build_seconds": round(time.perf_counter() - t0, 3)}), flush=True)

        def folder_source(kind):
            return tuple(T.folder_batches(st, B, T.default_transform(S, dev, max_batch=B), 42 + k) for k, st in enumerate(stores[kind]))
        sources = {"synthetic": (T.synthetic_batches(B, S, dev, 1234), T.synthetic_batches(B, S, dev, 4321))}
        sources["fixed"] = tuple(itertools.repeat(next(it).clone()) for it in sources["synthetic"])
        modes = [("fixed", "fixed", False), ("synthetic", "synthetic", False)]
        if args.device_decode:
            assert all(torch.equal(a[i], b[i]) for a, b in zip(stores["resident"], stores["resident+dd"]) for i in range(0, args.n, 37))
        for kind in ("resident", "streaming") + (("streaming+dd",) if args.device_decode else ()):
            sources[kind] = folder_source(kind)
            modes += [(kind, kind, False), (kind + "+overlap", kind, True)]

        step = 16                         # windows start at a multiple of the R1 period; the identity warm-up stays on throughout

        def window(source, overlap, n):
            nonlocal step
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in T.step_losses(trainer, *sources[source], step, step + n, overlap):
                pass
            torch.cuda.synchronize()
            step += n
            return (time.perf_counter() - t0) / n * 1e3
        for _, source, overlap in modes:          # warm-up: every mode's launches, tables and buffers
            window(source, overlap, 16)
        times = {name: [] for name, _, _ in modes}
        for _ in range(args.rounds):
            for name, source, overlap in modes:
                times[name].append(window(source, overlap, args.steps))
        med = {}
        for name, _, _ in modes:
            t = times[name]
            med[name] = statistics.median(t)
            print(json.dumps({"mode": name, "ms_per_step": round(med[name], 3), "min": round(min(t), 3), "max": round(max(t), 3),
                              "rounds": [round(v, 3) for v in t], "steps_per_round": args.steps, "batch": B, "size": S, "dtype": "bf16"}), flush=True)
        for base in ("synthetic", "fixed"):
            spread = max(times[base]) - min(times[base])
            print(json.dumps({"base": base, "base_spread_ms": round(spread, 3),
                              **{f"{name}_minus_base_ms": round(med[name] - med[base], 3) for name, _, _ in modes if name not in ("fixed", "synthetic")},
                              "host_preparation_shows": bool(med["resident"] - med[base] > spread)}), flush=True)
        for pair in stores.values():
            for st in pair:
                st.close()


if __name__ == "__main__":
    main()
