"""Step time of the fused CutTrainer in its three operand modes -- bf16, fp8 (e4m3 forward and input gradient of the residual
convolutions) and fp8 + fp8_wgrad (their weight gradients on e4m3 operands too) -- in one process.  The three trainers are built once
and warmed up, then timed in rotation: each round times `--steps` consecutive steps of every mode between two HIP events on the launch
stream, so clock and temperature drift hits all modes alike; the median round and the spread are reported.

usage: bench_fp8_wgrad.py [--size 256] [--batch 16] [--steps 16] [--warmup 4] [--rounds 5] [--modes bf16,fp8,fp8_wgrad]
One JSON line per mode."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gan_variant_research_amd import cut as C  # noqa: E402

MODES = {"bf16": (False, False), "fp8": (True, False), "fp8_wgrad": (True, True)}


def make(name, S, B, dev):
    fp8, fp8_wgrad = MODES[name]
    cfg = bench.default_config()
    C.set_seed(0)
    gen, disc = C.build_models(cfg, "cpu")
    g = torch.Generator().manual_seed(1)
    photos = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    monets = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    tr = C.CutTrainer(gen, disc, cfg, B, S, device=dev, amp=True, fp8=fp8, fp8_wgrad=fp8_wgrad)
    return tr, (lambda step: tr.train_step(step, photos, monets, sync=False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    a = ap.parse_args()
    dev = "cuda:0"
    names = a.modes.split(",")
    trainers, runs, steps = {}, {}, {}
    for n in names:
        trainers[n], runs[n] = make(n, a.size, a.batch, dev)
        steps[n] = 1                                     # step 0 has an R1 pass; the timed windows of 16 steps hold exactly one
        for _ in range(a.warmup):
            runs[n](steps[n])
            steps[n] += 1
        torch.cuda.synchronize()
    times = {n: [] for n in names}
    for _ in range(a.rounds):
        for n in names:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                runs[n](steps[n])
                steps[n] += 1
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / a.steps)
    base = statistics.median(times["bf16"]) if "bf16" in times else None
    for n in names:
        ms = statistics.median(times[n])
        took = [v for p in trainers[n].G.passes for v in getattr(p, "wgrad8_layers", {}).values()]
        out = {"mode": n, "size": a.size, "batch": a.batch, "ms_per_step": round(ms, 3), "images_per_s": round(a.batch / ms * 1e3, 2),
               "ms_rounds": [round(t, 3) for t in times[n]], "ms_min": round(min(times[n]), 3), "ms_max": round(max(times[n]), 3),
               "e4m3_wgrad_layers": sum(took), "bf16_fallback_layers": len(took) - sum(took)}
        if base:
            out["vs_bf16"] = round(ms / base, 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
