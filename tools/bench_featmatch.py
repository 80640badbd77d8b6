"""Times the fused CUT step (bench.py's configuration: 256 x 256, batch 16, bf16) with loss_weights.featmatch 0 and 10, and gan_featmatch
alone at the four feature-layer shapes of that step.

    python tools/bench_featmatch.py [--rounds 5] [--steps 20] [--warmup 6] [--batch 16] [--size 256] [--weights 0 10] [--out FILE]

Step: one trainer per weight, built from the same seed, in one process; after a warm-up the trainers take turns, `rounds` times, `steps`
steps each (queued with sync="lag" like bench.py, the last dict collected inside the window) between two host timestamps around a device
synchronisation.  Per weight one JSON line: the median of the rounds and [min .. max], in ms per step.  The yardstick for "nothing changed"
is the weight-0 line against bench.py (or this tool with --weights 0) on the parent commit; the cost of the term is the difference of the
two lines of one run, with the rounds' own spread as its margin.

Kernel: per layer one JSON line -- the launch as the trainer queues it (LeakyReLU factor, accumulate into g; f and r with halo 1, g with the
halo its consumer wants), timed with device events over `--kernel-reps` calls that walk through enough buffer sets to exceed the 256 MiB
Infinity Cache (so every call reads HBM, as it does inside a step), median of `rounds` such windows; beside it the bytes the call has to move
(f, r, g read, g written) and the floor bytes / 6.29 TB/s (the measured copy rate of the machine).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                                 # noqa: E402
from gan_variant_research_amd import BF16                                    # noqa: E402
from gan_variant_research_amd import cut as C                                # noqa: E402
from gan_variant_research_amd._lib import ACT_LRELU                          # noqa: E402
from gan_variant_research_amd.runtime import Ctx, HipOps                     # noqa: E402

HBM_COPY_RATE = 6.29e12          # bytes / s, measured float4 copy (MI355X)
CACHE_BYTES = 256 << 20


def layer_shapes(batch, size, ndf=64, n_layers=3):
    """(B, H, W, C, halo of g) of every feature layer of one scale: the discriminator's LeakyReLU outputs"""
    out, h = [], size
    for i in range(n_layers + 1):
        s = 2 if i < n_layers else 1
        h = (h + 2 - 4) // s + 1
        # g's halo is what the input gradient of the convolution that produced the layer needs: 2 behind a stride-1 one (the last layer's)
        out.append((batch, h, h, ndf * min(2 ** i, 8), 1 if s == 2 else 2))
    return out


def bench_kernel(dev, shapes, rounds, reps):
    ops = HipOps(dev)
    ctx = Ctx(ops, dev, BF16)
    lines = []
    for (B, H, W, Cc, hg) in shapes:
        n = B * H * W * Cc
        nbytes = 4 * n * 2                                                   # f, r, g read; g written; bf16
        sets = max(2, -(-2 * CACHE_BYTES // (3 * n * 2)))
        bufs = []
        gen = torch.Generator(device=dev).manual_seed(3)
        for _ in range(sets):
            f, r, g = ctx.view(B, H, W, Cc, 1), ctx.view(B, H, W, Cc, 1), ctx.view(B, H, W, Cc, hg)
            f.nhwc().copy_(torch.randn(B, H, W, Cc, device=dev, generator=gen))
            r.nhwc().copy_(torch.randn(B, H, W, Cc, device=dev, generator=gen))
            bufs.append((f, r, g))
        loss = ctx.f32(1)
        ws = ctx.f32(ops.featmatch_ws_floats(bufs[0][0]))
        calls = [ops.featmatch(f, r, Cc, 0.25, loss, 2.5, ACT_LRELU, g, True, ws) for f, r, g in bufs]
        for c in calls:
            c()
        torch.cuda.synchronize()
        us = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(reps):
                calls[k % sets]()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / reps)
        med = statistics.median(us)
        rec = {"metric": "featmatch_kernel_us", "shape": [B, H, W, Cc], "dtype": "bf16", "halo_g": hg, "elements": n, "bytes": nbytes, "buffer_sets": sets,
               "reps": reps, "median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
               "floor_us_at_6.29TBps": round(nbytes / HBM_COPY_RATE * 1e6, 2), "achieved_TBps": round(nbytes / (med * 1e-6) / 1e12, 3)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del bufs, calls
        torch.cuda.empty_cache()
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--weights", type=float, nargs="+", default=[0.0, 10.0])
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_featmatch.py measures on the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234)
    photos = (torch.rand(args.batch, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
    monets = (torch.rand(args.batch, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
    runs = []
    for w in args.weights:
        cfg = bench.default_config()
        if w > 0:
            cfg["loss_weights"]["featmatch"] = w
        C.set_seed(42)
        gen, disc = C.build_models(cfg, "cpu")
        tr = C.CutTrainer(gen, disc, cfg, args.batch, args.size, device=dev, amp=True, ops=HipOps(dev))
        runs.append({"weight": w, "trainer": tr, "step": 0, "ms": [], "last": None,
                     "gens": (torch.Generator().manual_seed(7), torch.Generator().manual_seed(8))})

    def steps(run, n):
        tr = run["trainer"]
        for _ in range(n):
            r = tr.train_step(run["step"], photos, monets, tr.sample_randomness(*run["gens"]), sync="lag")
            run["last"] = r if r is not None else run["last"]
            run["step"] += 1
        r = tr.flush_losses()
        run["last"] = r if r is not None else run["last"]

    for run in runs:
        steps(run, args.warmup)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for run in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(run, args.steps)
            torch.cuda.synchronize()
            run["ms"].append((time.perf_counter() - t0) / args.steps * 1e3)
    lines = []
    for run in runs:
        t = run["ms"]
        rec = {"metric": "cut_step_ms", "featmatch_weight": run["weight"], "batch": args.batch, "size": args.size, "dtype": "bf16", "rounds": args.rounds,
               "steps_per_round": args.steps, "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
               "rounds_ms": [round(x, 4) for x in t], "last_losses": run["last"]}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if not args.no_kernel:
        d = bench.default_config()["model"]["discriminator"]
        del runs
        torch.cuda.empty_cache()
        lines += bench_kernel(dev, layer_shapes(args.batch, args.size, d["ndf"], d["n_layers"]), args.rounds, args.kernel_reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
