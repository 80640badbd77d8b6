"""Step time of the fused CutTrainer with the reference's discriminator family (MultiscaleDiscriminator num_scales, use_spectral_norm)
against the baseline discriminator, and of the compatibility path module_step.train_step, in one process at the bench shape
(256x256, B=16, bf16 operands).  The configurations are built once, warmed up, then timed in rotation (each round times `--steps`
consecutive steps of every configuration between two HIP events on the launch stream); the median round is reported.

usage: bench_dfamily.py [--size 256] [--batch 16] [--steps 16] [--warmup 4] [--rounds 3] [--configs 1F,3F,2T,3T,module3T]
One JSON line per configuration."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gan_variant_research_amd import cut as C  # noqa: E402
from gan_variant_research_amd._lib import BF16  # noqa: E402

CONFIGS = {"1F": (1, False, False), "3F": (3, False, False), "2T": (2, True, False), "3T": (3, True, False), "module3T": (3, True, True)}


def make(name, S, B, dev):
    K, sn, module = CONFIGS[name]
    cfg = bench.default_config()
    cfg["model"]["discriminator"].update(num_scales=K, use_spectral_norm=sn)
    C.set_seed(0)
    gen, disc = C.build_models(cfg, "cpu")
    g = torch.Generator().manual_seed(1)
    photos = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    monets = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    if not module:
        tr = C.CutTrainer(gen, disc, cfg, B, S, device=dev, amp=True)
        return lambda step: tr.train_step(step, photos, monets, sync=False)
    from gan_variant_research_amd import losses as L, module_step as MS, training as T
    gen, disc = gen.to(dev), disc.to(dev)
    gen.compute_dtype = disc.compute_dtype = BF16
    opt_G, opt_D = T.get_optimizer(gen, cfg["optim"]["G"]), T.get_optimizer(disc, cfg["optim"]["D"])
    ema, amp = T.EMA(gen, cfg["ema"]["decay"], optimizer=opt_G), T.AMPContext(False)
    aug = L.DiffAugment(cfg["diffaugment"]["policy"])
    return lambda step: MS.train_step(step, photos, monets, gen, disc, opt_G, opt_D, ema, amp, aug, cfg, torch.device(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    dev = "cuda:0"
    names = a.configs.split(",")
    runs, steps = {}, {}
    for n in names:
        runs[n] = make(n, a.size, a.batch, dev)
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
    base = statistics.median(times["1F"]) if "1F" in times else None
    for n in names:
        K, sn, module = CONFIGS[n]
        ms = statistics.median(times[n])
        out = {"path": "module_step" if module else "fused", "num_scales": K, "spectral_norm": sn, "size": a.size, "batch": a.batch,
               "ms_per_step": round(ms, 3), "ms_rounds": [round(t, 3) for t in times[n]]}
        if base:
            out["vs_1F"] = round(ms / base, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
