"""Iteration time of the fused CycleGANTrainer in bf16, with fp8 and with fp8 + fp8_wgrad (e4m3 operand copies of the residual 3x3 256->256
convolutions of both generators: forward and input gradient, then the weight gradient too).

Configurations: BASELINE.json configs[1] (64x64, batch 256: 16x16 residual maps, where the e4m3 weight gradient sums 8 images per split) and
256x256, batch 16; ngf 64, 9 blocks, ndf 64, bf16 (amp) mode.  The three trainers live in one process, are warmed up, and are then timed
in rotation for --rounds rounds (each round: --steps consecutive iterations between two device synchronisations); the median and the
[min ... max] of the rounds are reported.

usage: bench_basic_fp8.py [--sizes 64x256,64x64,256x16] [--steps 10] [--warmup 3] [--rounds 5] [--out profiles/basic_fp8_bench.jsonl]
One JSON line per configuration and mode (appended to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_variant_research_amd import basic as BG  # noqa: E402
from gan_variant_research_amd._lib import GanError  # noqa: E402

MODES = {"bf16": {}, "fp8": {"fp8": True}, "fp8_wgrad": {"fp8": True, "fp8_wgrad": True}}


def config() -> dict:
    return {"training": {"amp": True, "seed": 0}, "optim": {"lr_g": 2e-4, "lr_d": 2e-4, "betas": [0.5, 0.999]},
            "loss": {"gan": "lsgan", "lambda_cycle": 10.0, "lambda_identity": 0.5},
            "model": {"ngf": 64, "ndf": 64, "n_blocks": 9, "spectral_norm_d": False}}


def inputs(S, B, dev):
    g = torch.Generator().manual_seed(1234)
    return (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev), (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)


def trainer(S, B, dev, **kw):
    cfg = config()
    torch.manual_seed(0)
    tr = BG.CycleGANTrainer(*BG.build_models(cfg, dev), cfg, B, S, device=dev, amp=True, **kw)
    a, b = inputs(S, B, dev)
    return tr, (lambda: tr.train_iteration(a, b, sync=False))


def wgrad8_summary(tr):
    """How the residual weight gradients of the six passes were planned: launches on e4m3 operands / all, and their images per split."""
    took = [ok for p in tr.P.values() for ok in getattr(p, "wgrad8_layers", {}).values()]
    ips = sorted({c.B // c.nsplit if c.nsplit < c.B else 1 for p in tr.P.values() for c in getattr(p, "wgrad8_calls", [])})
    return {"e4m3_wgrads": sum(took), "residual_wgrads": 6 * 18, "images_per_split": ips}


def timed(run, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64x256,64x64,256x16")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "basic_fp8_bench.jsonl"))
    a = ap.parse_args()
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    for spec in a.sizes.split(","):
        S, B = (int(x) for x in spec.split("x"))
        trs = {}
        for k, kw in MODES.items():
            try:
                trs[k] = trainer(S, B, dev, **kw)
            except GanError as e:                       # a mode the kernels do not take at this size is reported, not skipped silently
                out = {"mode": k, "size": S, "batch": B, "error": str(e)}
                print(json.dumps(out), flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(json.dumps(out) + "\n")
        if "bf16" not in trs:                           # nothing to compare against at this size
            continue
        for _, run in trs.values():
            for _ in range(a.warmup):
                run()
        times = {k: [] for k in trs}
        for _ in range(a.rounds):                       # in rotation
            for k, (_, run) in trs.items():
                times[k].append(timed(run, a.steps))
        base = statistics.median(times["bf16"])
        for k, ts in times.items():
            ms = statistics.median(ts)
            out = {"mode": k, "size": S, "batch": B, "ms_per_iter": round(ms, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                   "images_per_s": round(B / ms * 1e3, 1), "ms_rounds": [round(t, 3) for t in ts], "vs_bf16": round(ms / base, 4),
                   "steps": a.steps, "rounds": a.rounds, **(wgrad8_summary(trs[k][0]) if k == "fp8_wgrad" else {})}
            print(json.dumps(out), flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(out) + "\n")
        del trs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
