"""Times the fused CUT step (bench.py's configuration: 256 x 256, batch 16, bf16) with loss_weights.palette 0 and 0.5.

    python tools/bench_palette.py [--rounds 5] [--steps 20] [--warmup 6] [--batch 16] [--size 256] [--weights 0 0.5] [--out FILE]

One trainer per weight, built from the same seed, in one process; after a warm-up the trainers take turns, `rounds` times, `steps` steps
each (queued with sync="lag" like bench.py, the last dict collected inside the window) between two host timestamps around a device
synchronisation.  Per weight one JSON line: the median of the rounds and [min .. max], in ms per step.  The yardstick for "nothing
changed" is the weight-0 line against the same tool run on the parent commit (--weights 0); the cost of the term is the difference of
the two lines of one run, with the rounds' own spread as its margin.  Per-kernel times come from a run of their own under
`rocprofv3 --kernel-trace --stats -- python tools/bench_palette.py --weights 0.5 --rounds 1 --steps 3`.  Needs a GPU."""
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
from gan_variant_research_amd import cut as C                                # noqa: E402
from gan_variant_research_amd.runtime import HipOps                          # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--weights", type=float, nargs="+", default=[0.0, 0.5])
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_palette.py measures on the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234)
    photos = (torch.rand(args.batch, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
    monets = (torch.rand(args.batch, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
    runs = []
    for w in args.weights:
        cfg = bench.default_config()
        if w > 0:
            cfg["loss_weights"]["palette"] = w
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
        rec = {"metric": "cut_step_ms", "palette_weight": run["weight"], "batch": args.batch, "size": args.size, "dtype": "bf16", "rounds": args.rounds,
               "steps_per_round": args.steps, "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
               "rounds_ms": [round(x, 4) for x in t], "last_losses": run["last"]}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
