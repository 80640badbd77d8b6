"""What the data-parallel driver layer costs and how `train_cutpp --gpus N` scales: train_cutpp's own run on a generated folder
(256x256, batch 16 per GPU, bf16), timed step by step inside the driver's loop, in these modes

    plain         python -m ...train_cutpp                      (no process group: the launches of the single-GPU driver)
    group1        the same inside a one-rank RCCL group          (RANK=0 WORLD_SIZE=1 LOCAL_RANK=0 and a rendezvous address: stream binding
                                                                 before RCCL, every gradient all-reduce, the loss all-reduce -- sums over one
                                                                 rank, so it prices the collectives' launches alone)
    gpus2/4/8     --gpus N through launch.launch_ranks          (only where torch.cuda.device_count() shows that many)

Every run is a fresh child process under its own timeout (a worker of this file: the driver's main with its step loop timed); the
modes take turns over ROUNDS rounds, and after a child that fails or times out nothing further is started.  A run makes WARMUP + STEPS
steps (both multiples of the lazy-R1 period, so every window holds the same work) and reports the mean time of the last STEPS.  One
JSON line per mode: median and [min .. max] of ms/step and of global images/s over the rounds, and for --gpus N the ratio to N x plain.

usage: bench_train_dp.py [--n 256] [--steps 32] [--warmup 16] [--rounds 5] [--timeout 300]
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, S = 16, 256
RENDEZVOUS = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")


def write_jpegs(folder, n, seed):
    """n photo-like 256x256 JPEGs (low-frequency colour plus noise), as tools/bench_dataio.py writes them."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
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
        Image.fromarray(np.clip(bases[i % 8] + noise, 0, 255).astype(np.uint8)).save(os.path.join(folder, f"{i:05d}.jpg"), quality=90)
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(write, range(n)))


def worker(argv):
    """One rank (or the plain process): train_cutpp.main with its step loop timed; rank 0 prints the JSON line."""
    from gan_variant_research_amd import train_cutpp as T
    warmup, stamps, loop = int(argv[0]), [], T.step_losses

    def timed(*a, **kw):
        for item in loop(*a, **kw):          # a step is delivered when its losses have been read: one host wait per step
            stamps.append(time.perf_counter())
            yield item
    T.step_losses = timed
    r = T.main(argv[1:])
    n = len(stamps) - 1 - warmup
    if r.get("rank", 0) == 0:
        print(json.dumps({"worker": True, "ms_per_step": (stamps[-1] - stamps[warmup]) / n * 1e3, "steps": n, "world": r.get("world", 1)}), flush=True)


def run_mode(mode, argv, warmup, timeout):
    """A fresh child for one window of one mode; returns its ms/step, or raises SystemExit (then nothing further is started)."""
    env = {k: v for k, v in os.environ.items() if k not in RENDEZVOUS}
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(warmup), *argv]
    if mode == "group1":
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = str(sk.getsockname()[1])
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    elif mode.startswith("gpus"):
        cmd = [sys.executable, os.path.abspath(__file__), "--launch", mode[4:], str(warmup), *argv]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"[bench_train_dp] mode {mode}: no result within {timeout} s; stopping")
    if r.returncode != 0:
        raise SystemExit(f"[bench_train_dp] mode {mode} exited with code {r.returncode}; stopping\n{r.stderr[-2000:]}")
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{"worker"')]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0]["ms_per_step"]


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        return worker(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--launch":          # the launcher of `--gpus N`, starting this file's worker as the ranks
        from gan_variant_research_amd import launch
        return launch.launch_ranks([os.path.abspath(__file__), "--worker", sys.argv[3]], sys.argv[4:], int(sys.argv[2]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256, help="JPEGs per domain")
    ap.add_argument("--steps", type=int, default=32, help="timed steps per run")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    args = ap.parse_args()
    import yaml
    from bench import default_config
    from gan_variant_research_amd import launch
    gpus = launch.visible_gpus()              # asked of a short-lived child: this process opens no GPU
    assert gpus >= 1, "bench_train_dp needs the GPU"
    modes = ["plain", "group1"] + [f"gpus{n}" for n in (2, 4, 8) if n <= gpus]
    print(json.dumps({"visible_gpus": gpus, "modes": modes, "batch_per_gpu": B, "size": S, "dtype": "bf16", "steps": args.steps,
                      "warmup": args.warmup, "rounds": args.rounds}), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for k, d in enumerate(("photos", "monet")):
            write_jpegs(os.path.join(tmp, d), args.n, k)
        cfg = default_config()
        cfg.update({"seed": 42, "amp": True, "batch_size": B, "image_size": S, "epochs": 1, "max_steps": args.warmup + args.steps + 1,
                    "log_every": 1000, "metrics": {"save_checkpoint_every": 100000},
                    "data": {"photos_dir": os.path.join(tmp, "photos"), "monet_dir": os.path.join(tmp, "monet")}})
        with open(os.path.join(tmp, "cfg.yaml"), "w") as f:
            yaml.safe_dump(cfg, f)
        times = {m: [] for m in modes}
        for rnd in range(args.rounds):
            for m in modes:
                out = os.path.join(tmp, f"{m}_{rnd}")
                argv = ["--config", os.path.join(tmp, "cfg.yaml"), "--set", f"output.checkpoint_dir={out}/ck", f"output.log_dir={out}/lg"]
                times[m].append(run_mode(m, argv, args.warmup, args.timeout))
    med = {}
    for m in modes:
        t, n = times[m], int(m[4:]) if m.startswith("gpus") else 1
        med[m] = statistics.median(t)
        ips = sorted(n * B / (v * 1e-3) for v in t)
        line = {"mode": m, "n_gpus": n, "global_batch": n * B, "ms_per_step": round(med[m], 3), "min": round(min(t), 3), "max": round(max(t), 3),
                "rounds": [round(v, 3) for v in t], "images_per_s": round(statistics.median(ips), 1), "images_per_s_min": round(ips[0], 1),
                "images_per_s_max": round(ips[-1], 1)}
        if m == "group1":
            line.update(minus_plain_ms=round(med[m] - med["plain"], 3), plain_spread_ms=round(max(times["plain"]) - min(times["plain"]), 3),
                        own_spread_ms=round(max(t) - min(t), 3))
        if n > 1:
            line["ratio_to_n_times_plain"] = round(statistics.median(ips) / (n * B / (med["plain"] * 1e-3)), 4)
        print(json.dumps(line), flush=True)
    if gpus < 2:
        print(json.dumps({"scaling": None, "why": "one GPU visible: --gpus N was not run"}), flush=True)


if __name__ == "__main__":
    main()
