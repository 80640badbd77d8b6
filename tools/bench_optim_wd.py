"""Times the fused optimiser step over the generator's real parameter list (ResNet-9, ngf 64: 48 tensors, 11.4 M elements, EMA on) through
four paths: gan_adam_step, gan_adam_step_wd with weight_decay 0 (the same kernels), L2 decay and decoupled decay.

    python tools/bench_optim_wd.py [--rounds 5] [--iters 1000] [--out FILE]

The paths run in rotation after a warm-up, `rounds` times, `iters` calls each between two HIP events; per path the median and [min .. max]
of the rounds are printed, with bytes/s at 36 B per parameter (p, m, v, ema read and written, g read by the update kernel; the
sum-of-squares kernel reads g once more, which is not counted).  The yardstick for "unchanged" is the first path in the same run; the
margin is the rounds' own spread.  All four paths step the same state block.  Needs a GPU.

    python tools/bench_optim_wd.py --host [--calls 200] [--reps 3] [--out FILE]

times the HOST side instead (see host()): what training.HipAdam.step and the fused_clip_adam_ema_ op cost per call on four small tensors."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_variant_research_amd import F32                                     # noqa: E402
from gan_variant_research_amd import cut as C                                # noqa: E402
from gan_variant_research_amd.runtime import Ctx, HipOps                     # noqa: E402

MODEL = {"generator": {"ngf": 64, "n_blocks": 9, "n_downsampling": 2, "padding_type": "reflect", "norm": "instance", "activation": "relu"},
         "discriminator": {"ndf": 64, "n_layers": 3, "num_scales": 1, "use_spectral_norm": False}}


SMALL = [1, 5, 16384, 16387]      # four tensors, five chunks: the kernels take their least time, what is left is the host's


def host(args, dev):
    """--host: host clock per call of training.HipAdam.step and of torch.ops.mi355x_gan.fused_clip_adam_ema_ (L2 decay, EMA, clipping)
    on the SMALL tensors, `--calls` calls between two device synchronises, `--reps` repetitions in rotation after a warm-up."""
    from gan_variant_research_amd import ops_library  # noqa: F401  (registers the ops)
    from gan_variant_research_amd import training as T
    new = lambda: [torch.randn(n, device=dev) for n in SMALL]
    ps = [torch.nn.Parameter(t) for t in new()]
    opt = T.HipAdam(ps, weight_decay=1e-4)
    opt.attach_ema({id(p): p.detach().clone() for p in ps}, 0.999)
    for p, g in zip(ps, new()):
        p.grad = g
    q, g, m, v, ema = new(), new(), [torch.zeros(n, device=dev) for n in SMALL], [torch.zeros(n, device=dev) for n in SMALL], new()
    steps = torch.zeros(len(SMALL), dtype=torch.int32, device=dev)
    paths = [("HipAdam.step", lambda: opt.step(max_grad_norm=10.0)),
             ("fused_clip_adam_ema_", lambda: torch.ops.mi355x_gan.fused_clip_adam_ema_(q, g, m, v, ema, steps, 2e-4, 0.5, 0.999, 1e-8, 10.0, 1.0, 0.999,
                                                                                         None, False, 1e-4, False))]
    times = {name: [] for name, _ in paths}
    for rep in range(-1, args.reps):          # -1: the warm-up (plans, tables and launches are built)
        for name, call in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            torch.cuda.synchronize()
            if rep >= 0:
                times[name].append((time.perf_counter() - t0) / args.calls * 1e6)
    lines = [f"{name:22s} host us per call over {args.calls} calls, {args.reps} repetitions: " + "  ".join(f"{t:.2f}" for t in ts) +
             f"   median {statistics.median(ts):.2f}  spread {max(ts) - min(ts):.2f}" for name, ts in times.items()]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_optim_wd.py measures on the GPU"
    dev = torch.device("cuda:0")
    if args.host:
        return host(args, dev)
    ctx = Ctx(HipOps(dev), dev, F32)
    gen, _ = C.build_models({"model": MODEL}, "cpu")
    sd = {k: v.detach().float() for k, v in gen.state_dict().items()}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def optimiser(wd, decoupled):
        opt = C.FusedAdam(ctx, list(sd), [v.shape for v in sd.values()], sd, 2e-4, (0.5, 0.999), 1e-8, wd, ema_decay=0.999, decoupled=decoupled)
        torch.manual_seed(0)
        opt.flat_g.normal_(0, 1e-3)
        return opt
    a = lambda o: (o.table(), len(o.names), o.chunk_tensor, o.chunk_off, o.nchunks, o.lr, 0.5, 0.999, 1e-8, 10.0, 1.0, 0.999, o.norm_out, o.ws)
    # one state block for all four paths (the decay is an argument of the call): four blocks of their own would time their placement too
    o0 = optimiser(0.0, False)
    paths = [("gan_adam_step", ctx.ops.adam_step(*a(o0), lr_dev=o0.lr_dev)),
             ("gan_adam_step_wd wd=0", ctx.ops.adam_step_wd(*a(o0), 0.0, False, lr_dev=o0.lr_dev)),
             ("gan_adam_step_wd L2 1e-4", ctx.ops.adam_step_wd(*a(o0), 1e-4, False, lr_dev=o0.lr_dev)),
             ("gan_adam_step_wd decoupled 1e-4", ctx.ops.adam_step_wd(*a(o0), 1e-4, True, lr_dev=o0.lr_dev))]
    n = sum(o0.sizes)
    say(f"{len(o0.names)} tensors, {n} elements, {o0.nchunks} chunks, EMA on; {args.rounds} rounds x {args.iters} calls per path, in rotation")
    for _, op in paths:
        for _ in range(20):
            op()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in paths}
    for r in range(args.rounds):
        for name, op in paths:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                op()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters * 1e3)
        say(f"round {r}: " + "  ".join(f"{name} {times[name][-1]:.2f} us" for name, _ in paths))
    base = statistics.median(times[paths[0][0]])
    for name, _ in paths:
        t = times[name]
        med = statistics.median(t)
        say(f"{name:34s} median {med:8.2f} us [{min(t):.2f} .. {max(t):.2f}]  {36 * n / med / 1e6:5.2f} TB/s at 36 B/param  x{med / base:.4f} of gan_adam_step")
    for o in (o0,):
        assert bool(torch.isfinite(o.flat_p).all()), "a path went non-finite"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
