"""Measures patchnce.nce_includes_all_negatives_from_minibatch: the fused CUT step with the key false and true, and the whole-minibatch kernels
per layer shape against a plain torch fp32 statement.

    python tools/bench_nce_all.py [--rounds 5] [--steps 20] [--warmup 6] [--batch 16] [--size 256] [--part step|layers|both] [--out FILE]

STEP (bench.py's configuration: 256 x 256, batch 16, bf16).  One trainer per key value, built from the same seed, in one process; after a
warm-up the trainers take turns, `rounds` times, `steps` steps each (queued with sync="lag" like bench.py) between two host timestamps
around a device synchronisation.  Per key value one JSON line: the median of the rounds and [min .. max], in ms per step.

LAYERS (Q = batch x 256 query rows, C = 64 / 128 / 256: the present layers of the step).  gather + forward + backward of the
gan_patchnce_all_* entry points (one rank: the keys are the workspace's own rows) against the same statement in torch fp32 -- normalize,
`mm`, clamp, `logsumexp`, autograd -- on the gathered rows, in rotation, `rounds` rounds of `steps` calls each.  Per shape one JSON line:
both medians with [min .. max], torch's peak memory allocated above the inputs during its call and the workspace the kernels need, and the
largest difference of the loss and of the gradient rows.  No speed is promised; the numbers are reported as they fall.

Kernel times come from a run of their own: `rocprofv3 --kernel-trace --stats -- python tools/bench_nce_all.py --part layers --rounds 1
--steps 3`.  Needs a GPU."""
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
from gan_variant_research_amd import F32                                     # noqa: E402
from gan_variant_research_amd import cut as C                                # noqa: E402
from gan_variant_research_amd.runtime import Ctx, HipOps                     # noqa: E402

KEY = "nce_includes_all_negatives_from_minibatch"
T, WEIGHT = 0.07, 1.0


def _spread(t):
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "rounds_ms": [round(x, 4) for x in t]}


def bench_step(args, dev):
    g = torch.Generator().manual_seed(1234)
    photos = (torch.rand(args.batch, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
    monets = (torch.rand(args.batch, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
    runs = []
    for key in (False, True):
        cfg = bench.default_config()
        cfg["patchnce"][KEY] = key
        C.set_seed(42)
        gen, disc = C.build_models(cfg, "cpu")
        tr = C.CutTrainer(gen, disc, cfg, args.batch, args.size, device=dev, amp=True, ops=HipOps(dev))
        runs.append({"key": key, "trainer": tr, "step": 0, "ms": [], "last": None, "gens": (torch.Generator().manual_seed(7), torch.Generator().manual_seed(8))})

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
    return [json.dumps({"metric": "cut_step_ms", KEY: run["key"], "batch": args.batch, "size": args.size, "dtype": "bf16", "rounds": args.rounds,
                        "steps_per_round": args.steps, **_spread(run["ms"]), "last_losses": run["last"]}) for run in runs]


def torch_statement(s, t):
    """s, t: (Q, C) fp32 gathered rows, t requires grad -> the loss of one call with one key segment"""
    sn = torch.nn.functional.normalize(s, dim=1, eps=1e-6)
    tn = torch.nn.functional.normalize(t, dim=1, eps=1e-6)
    lg = (torch.mm(tn, sn.t()) / T).clamp(-50.0, 50.0)
    return WEIGHT * (torch.logsumexp(lg, 1) - torch.diagonal(lg)).mean()


def bench_layers(args, dev):
    ctx = Ctx(HipOps(dev), dev, F32)
    ops = ctx.ops
    B, P, H = args.batch, 256, 64
    lines = []
    for Cc in (64, 128, 256):
        g = torch.Generator().manual_seed(100 + Cc)
        src = torch.randn(B, H, H, Cc, generator=g)
        tgt = src + 0.5 * torch.randn(B, H, H, Cc, generator=g)
        ids = torch.randperm(H * H, generator=g)[:P]
        sv, tv, gv = ctx.view(B, H, H, Cc, 1, dtype=F32), ctx.view(B, H, H, Cc, 1, dtype=F32), ctx.view(B, H, H, Cc, 1, dtype=F32)
        sv.nhwc().copy_(src.to(dev))
        tv.nhwc().copy_(tgt.to(dev))
        iv = ctx.i32(ids.tolist())
        n_ws = ops.patchnce_all_ws_floats(B, P, Cc)
        ws, loss = ctx.f32(n_ws), ctx.f32(1)
        hip = [ops.patchnce_all_gather(sv, tv, iv, P, Cc, ws), ops.patchnce_all_fwd(tv, P, Cc, T, WEIGHT, ws, 1, 0, 0, loss, ws),
               ops.patchnce_all_bwd(tv, iv, P, Cc, T, WEIGHT, ws, 1, 0, 0, gv, ws)]
        ys, xs = (ids // H).to(dev), (ids % H).to(dev)
        s_rows = sv.nhwc()[:, ys, xs].reshape(B * P, Cc).contiguous()
        t_rows = tv.nhwc()[:, ys, xs].reshape(B * P, Cc).contiguous().requires_grad_(True)

        def run_hip():
            loss.zero_()
            for op in hip:
                op()

        def run_torch():
            t_rows.grad = None
            torch_statement(s_rows, t_rows).backward()

        for fn in (run_hip, run_torch):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        run_torch()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        ref_loss = float(torch_statement(s_rows, t_rows).detach())
        run_hip()
        torch.cuda.synchronize()
        Q = B * P
        dX = ws[n_ws - 64 - Q * Cc:n_ws - 64].view(Q, Cc)
        d_loss, d_grad = abs(float(loss) - ref_loss), float((dX - t_rows.grad).abs().max())
        ms = {"hip": [], "torch": []}
        for _ in range(args.rounds):
            for name, fn in (("hip", run_hip), ("torch", run_torch)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
        lines.append(json.dumps({"metric": "nce_all_fwd_bwd_ms", "Q": Q, "K": Q, "C": Cc, "rounds": args.rounds, "calls_per_round": args.steps,
                                 "hip": _spread(ms["hip"]), "torch_fp32": _spread(ms["torch"]), "torch_peak_bytes_above_inputs": int(peak),
                                 "hip_workspace_bytes": 4 * n_ws, "loss": ref_loss, "max_abs_diff_loss": d_loss, "max_abs_diff_grad": d_grad,
                                 "max_abs_grad": float(t_rows.grad.abs().max())}))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--part", choices=("step", "layers", "both"), default="both")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_nce_all.py measures on the GPU"
    dev = torch.device("cuda:0")
    lines = []
    if args.part in ("step", "both"):
        lines += bench_step(args, dev)
    if args.part in ("layers", "both"):
        lines += bench_layers(args, dev)
    for line in lines:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
