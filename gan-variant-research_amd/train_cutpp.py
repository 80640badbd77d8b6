"""Training driver with the reference's command line (GAN_Variant1/training/train_cutpp.py:39-85, 340-498):

    python -m gan_variant_research_amd.train_cutpp --config GAN_Variant1/configs/train_gan_cutpp.yaml [--resume CKPT] [--set a.b=c ...] [--gpus N]

Same flags, same YAML schema (the keys the reference reads; its dead keys are accepted and ignored), same `--set` coercion
(true/false -> bool, then int, then float, else string), same checkpoint layout and file names, same loss CSV / JSON log lines.
What differs is what runs underneath: the step is the fused `cut.CutTrainer` on the HIP kernels instead of torch.nn modules.
Image folders are decoded once with Pillow at start-up into a `dataio.ImageStore` (resident on the device when they fit
`mi355x.dataset_cache_gb`, default 8; decoded per batch otherwise) and transformed on the device (dataio.py, the reference's train
transform); with `--synthetic` uniform noise batches of the right shape stand in (there is no dataset on the benchmark box); folders
that do not exist are an error.  Build-only keys live under `mi355x:` (amp dtype, synthetic data, dataset_cache_gb,
device_decode: the stores decode their baseline JPEGs on the device with dataio.JpegDecoder, default false;
device_png: the same for their PNGs with dataio.PngDecoder, default false;
device_progressive: with device_decode, the progressive JPEGs are decoded on the device too, default false;
decoupled_weight_decay: `optim.{G,D}.weight_decay` as AdamW's decay instead of torch.optim.Adam's L2 term).

`--gpus N` (build-only flag; launch.py) trains data-parallel on N GPUs of one node: `batch_size` stays the per-GPU batch, and at every
step rank r feeds and draws rows [r B, (r+1) B) of what one process with `batch_size` N B and the same seed feeds and draws -- the same
epoch permutations cut into global batches, the transform jobs and the step's DiffAugment / PatchNCE draws of the whole global batch
drawn on every rank.  Rank 0 alone logs and saves (losses of the global batch); checkpoints do not depend on N and resume on any N.
Every rank holds its own ImageStore (sharding it across ranks is not done) with 16 // N decode threads.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
from collections import defaultdict
from pathlib import Path
from typing import Iterator, List, Optional

import numpy as np
import torch
import yaml

from . import cut as C
from . import launch

IMAGE_EXTS = {".jpg", ".jpeg", ".png", ".bmp", ".webp"}


def parse_args(argv=None):
    """train_cutpp.py:39-48."""
    p = argparse.ArgumentParser(description="Train CUT++ GAN (MI355X-native step)")
    p.add_argument("--config", type=str, default="GAN_Variant1/configs/train_gan_cutpp.yaml", help="Path to config file")
    p.add_argument("--resume", type=str, default=None, help="Path to checkpoint to resume from")
    p.add_argument("--set", nargs="+", default=[], help="Override config values (e.g., loss_weights.adv=0.5)")
    p.add_argument("--synthetic", action="store_true", help="uniform-noise batches instead of the image folders (build-only flag)")
    launch.add_arguments(p)
    return p.parse_args(argv)


def override_config(config: dict, overrides) -> dict:
    """train_cutpp.py:51-85: `a.b.c=value`; missing intermediate dicts are created; value coercion true/false, int, float, string;
    entries without '=' are skipped."""
    for item in overrides:
        if "=" not in item:
            continue
        path, value = item.split("=", 1)
        keys = path.split(".")
        cur = config
        for k in keys[:-1]:
            if k not in cur:
                cur[k] = {}
            cur = cur[k]
        low = value.lower()
        if low == "true":
            value = True
        elif low == "false":
            value = False
        else:
            for cast in (int, float):
                try:
                    value = cast(value)
                    break
                except ValueError:
                    pass
        cur[keys[-1]] = value
    return config


def _list_images(folder) -> List[Path]:
    root = Path(folder)
    return sorted(p for p in root.rglob("*") if p.suffix.lower() in IMAGE_EXTS) if root.is_dir() else []


def build_store(paths: List[Path], device, config: dict, name: str, folder=None, workers: Optional[int] = None, quiet: bool = False):
    """One `dataio.ImageStore` per domain, decoded at start-up; `mi355x.dataset_cache_gb` (default 8) is what may stay on the device;
    `mi355x.device_decode` (default false) decodes the baseline JPEGs on the device instead of with Pillow (same bytes), and
    `mi355x.device_png` (default false) the PNGs; `mi355x.device_progressive` (default false, needs device_decode) the progressive JPEGs too.
    workers: decode threads (data parallel: 16 // N per rank, every rank holds its own store)."""
    import time
    from .dataio import DEFAULT_CACHE_GB, ImageStore
    build = config.get("mi355x", {}) or {}
    t0 = time.perf_counter()
    store = ImageStore(paths, device, budget_bytes=int(float(build.get("dataset_cache_gb", DEFAULT_CACHE_GB)) * (1 << 30)), workers=workers, folder=folder,
                       device_decode=bool(build.get("device_decode", False)), **({"device_png": True} if build.get("device_png", False) else {}),
                       **({"device_progressive": True} if build.get("device_progressive", False) else {}))
    mode = f"resident on {store.device}" if store.resident else "streaming (decoded per batch)"
    if not quiet:
        print(f"[data] {name}: {len(store)} images, {store.nbytes / 1e6:.1f} MB decoded, {mode}, {time.perf_counter() - t0:.2f} s")
    return store


def default_transform(image_size: int, device, max_batch: int = 64):
    """The reference's train transform on the device (dataio.get_train_transforms: random-crop-resize bicubic, flip, ColorJitter,
    normalise -- transforms.py:10-39)."""
    from .dataio import get_train_transforms
    return get_train_transforms(image_size, device=device, max_batch=max_batch)


def folder_batches(store, batch: int, tf, seed: int) -> Iterator[torch.Tensor]:
    """Shuffled, drop_last epochs over an image folder held by a `dataio.ImageStore` (decoded once; on the device when it fits).  `tf`
    draws one job per image of the batch, in order, and runs the transform (dataio._Transform)."""
    rng = random.Random(seed)
    while True:
        order = list(range(len(store)))
        rng.shuffle(order)
        for i in range(0, len(order) - batch + 1, batch):
            yield tf(store.fetch(order[i:i + batch]))


def folder_batches_dp(store, batch: int, tf, seed: int, image_size: int, place) -> Iterator[torch.Tensor]:
    """`folder_batches` for one rank of `place.world`: the same permutations cut into global batches of world * batch, one train_job per
    image of the GLOBAL batch drawn in order on every rank (numpy's global RNG moves as in one process at that batch size); this rank
    fetches its rows and runs `tf(images, jobs)` on them."""
    from .dataio import train_job
    rng = random.Random(seed)
    whole, rows = place.world * batch, place.rows(batch)
    while True:
        order = list(range(len(store)))
        rng.shuffle(order)
        for i in range(0, len(order) - whole + 1, whole):
            idx = order[i:i + whole]
            jobs = [train_job(*store.sizes[j], image_size) for j in idx]
            yield tf(store.fetch(idx[rows]), jobs[rows])


def synthetic_batches(batch: int, image_size: int, device, seed: int, rows: Optional[slice] = None) -> Iterator[torch.Tensor]:
    """rows: the global batch of `batch` images is drawn, these rows of it are handed out (data parallel)."""
    g = torch.Generator().manual_seed(seed)
    while True:
        x = torch.rand(batch, 3, image_size, image_size, generator=g) * 2 - 1
        yield (x if rows is None else x[rows]).to(device)


def step_losses(trainer, photos_it, monet_it, start: int, stop: int, overlap: bool, draw=None):
    """The steps start .. stop-1, one `(step, loss dict)` at a time, in order.  overlap: step k is queued (sync="lag"), the host
    prepares batch k+1 while the device runs it, then step k's losses are read (flush_losses) -- so they are checked for NaN and
    delivered before the caller logs or saves anything of step k, and no batch beyond stop-1 is drawn.
    draw (data parallel): returns the step's randomness (this rank's rows of the global draws); None: the trainer draws its own."""
    rnd = (lambda: None) if draw is None else draw
    if not overlap:
        for step in range(start, stop):
            yield step, trainer.train_step(step, next(photos_it), next(monet_it), rnd())
        return
    batch = (next(photos_it), next(monet_it)) if start < stop else None
    for step in range(start, stop):
        trainer.train_step(step, batch[0], batch[1], rnd(), sync="lag")
        batch = (next(photos_it), next(monet_it)) if step + 1 < stop else None
        yield step, trainer.flush_losses()


class LossLog:
    """utils/loss_tracker.py:25-42 (CSV `step,d_loss,g_loss`, flushed per step) and the JSON line of train_cutpp.py:449-459."""

    def __init__(self, log_dir: Path):
        log_dir.mkdir(parents=True, exist_ok=True)
        self.csv = open(log_dir / "losses_history.csv", "a")      # the file name of utils/loss_tracker.py:17
        if self.csv.tell() == 0:
            self.csv.write("step,d_loss,g_loss\n")
        self.txt = log_dir / "train_log.txt"

    def step(self, step, losses):
        self.csv.write(f"{step},{losses['d_loss']},{losses['g_loss']}\n")
        self.csv.flush()

    def summary(self, step, avg):
        with open(self.txt, "a") as f:
            f.write(f"Step {step}: {json.dumps(avg)}\n")

    def close(self):
        self.csv.close()


def main(argv=None, ops=None, device: Optional[str] = None, transform=None) -> dict:
    """train_cutpp.py:340-498.  `ops` / `device` / `transform` are test hooks (the CPU suite drives the host logic through the emulator):
    `transform(image_size, device)` returns the callable that turns a list of decoded uint8 (H, W, 3) images into the (B, 3, S, S) fp32
    batch (default: `default_transform`, the device pipeline -- on a CPU device it raises that it runs on the GPU).

    With image folders the host prepares batch k+1 while the device runs step k (the step is queued with sync="lag" and its losses are
    read after the preparation): the rows of the CSV, the summaries and the checkpoints are those of the unoverlapped loop, a NaN step
    raises before anything later is saved.  --synthetic reads every step's losses before it draws the next batch, as before."""
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:      # this process becomes the launcher, before any GPU call
        launch.launch_ranks(["-m", __spec__.name if __spec__ is not None else __name__], sys.argv[1:] if argv is None else list(argv), args.gpus,
                            check_devices=not args.launch_check)
        return {"launched": args.gpus}
    launch.check_rank_count(args.gpus, check_devices=False)
    world = launch.world_from_env(args.gpus)
    if args.launch_check:
        launch.launch_check()
        return {"launch_check": True}
    with open(args.config) as f:
        config = yaml.safe_load(f)
    config = override_config(config, args.set)
    C.set_seed(config.get("seed", 42))
    with launch.join(world, device, ops) as place:
        return _train(args, config, place, transform)


def _train(args, config: dict, place, transform) -> dict:
    """One rank's run (the only one without --gpus): `place.group` is None in the plain single-process run, which then does what it
    always did.  With a group, N ranks x batch B are one process at batch N B (module docstring); rank 0 logs and saves."""
    device, ops, dp, N = place.device, place.ops, place.group is not None, place.world
    say = print if place.first else (lambda *a, **kw: None)
    say(f"Using device: {device}" + (f" ({N} rank(s), global batch {N * int(config['batch_size'])})" if dp else ""))
    ckpt_dir, log_dir = Path(config["output"]["checkpoint_dir"]), Path(config["output"]["log_dir"])
    log = None
    if place.first:
        ckpt_dir.mkdir(parents=True, exist_ok=True)
        log = LossLog(log_dir)
    B, S = int(config["batch_size"]), int(config["image_size"])
    whole = N * B                                              # the global batch
    build = config.get("mi355x", {}) or {}
    photos_paths, monet_paths = _list_images(config["data"]["photos_dir"]), _list_images(config["data"]["monet_dir"])
    synthetic = bool(args.synthetic or build.get("synthetic", False))
    if not synthetic:      # like the reference, a wrong data path is an error -- never a silent run on noise that still writes ckpt_*.pt
        for name, paths in (("photos_dir", photos_paths), ("monet_dir", monet_paths)):
            if len(paths) < whole:
                raise FileNotFoundError(f"data.{name} = {config['data'][name]!r} holds {len(paths)} images (< batch_size {whole}"
                                        + (f" = {N} ranks x {B}" if dp else "") + "); "
                                        "pass --synthetic (or mi355x.synthetic: true) to train on uniform-noise batches instead")
    if synthetic:
        say("[train_cutpp] --synthetic: uniform-noise batches stand in for the data loaders")
        rows = place.rows(B) if dp else None
        photos_it, monet_it = synthetic_batches(whole, S, device, 1234, rows), synthetic_batches(whole, S, device, 4321, rows)
        steps_per_epoch = 7038 // whole      # the reference's photo count (train_gan_cutpp.yaml: 70 epochs x 7038 // 12 steps)
    else:
        seed = config.get("seed", 42)
        make_tf = transform if transform is not None else (lambda size, dev: default_transform(size, dev, max_batch=max(B, 16)))
        workers = max(1, 16 // N) if dp else None
        photos = build_store(photos_paths, device, config, "photos", config["data"]["photos_dir"], workers, quiet=not place.first)
        monets = build_store(monet_paths, device, config, "monet", config["data"]["monet_dir"], workers, quiet=not place.first)
        if dp:
            photos_it = folder_batches_dp(photos, B, make_tf(S, device), seed, S, place)
            monet_it = folder_batches_dp(monets, B, make_tf(S, device), seed + 1, S, place)
        else:
            photos_it, monet_it = folder_batches(photos, B, make_tf(S, device), seed), folder_batches(monets, B, make_tf(S, device), seed + 1)
        steps_per_epoch = len(photos_paths) // whole
        say(f"Photos: {len(photos_paths)}, Monet: {len(monet_paths)}")

    generator, discriminator = C.build_models(config, "cpu")
    if dp:
        trainer = C.CutTrainer(generator, discriminator, config, B, S, device=device, amp=config.get("amp", True), ops=ops, world_size=N,
                               process_group=place.group, average_losses=True)
        trainer.force_allreduce = True       # a one-rank group runs the collectives too (sums over one rank: the same bits)
        rows = place.rows(B)
        # the global batch's draws from the global generator, seeded alike on every rank (set_seed), as one process at batch N B makes them
        draw = lambda: trainer.shard_randomness(trainer.sample_randomness(batch=whole), rows.start, rows.stop)
    else:
        trainer, draw = C.CutTrainer(generator, discriminator, config, B, S, device=device, amp=config.get("amp", True), ops=ops), None
    start_step = 0
    if args.resume:
        start_step = int(trainer.load_checkpoint(args.resume)["step"])
        say(f"Resumed from step {start_step}")
    max_steps = config.get("max_steps", None)
    if max_steps is None:
        max_steps = config["epochs"] * steps_per_epoch
    say(f"Training for {max_steps} steps")

    acc = defaultdict(list)
    losses = {}
    for step, losses in step_losses(trainer, photos_it, monet_it, start_step, max_steps, overlap=not synthetic, draw=draw):
        if not place.first:
            continue
        for k, v in losses.items():
            acc[k].append(v)
        log.step(step, losses)
        if step % config.get("log_every", 100) == 0 and step > 0:
            log.summary(step, {k: float(np.mean(v)) for k, v in acc.items()})
            acc.clear()
        if step % config["metrics"]["save_checkpoint_every"] == 0 and step > 0:
            path = ckpt_dir / f"ckpt_step{step}.pt"
            trainer.save_checkpoint(str(path), step)
            print(f"\nSaved checkpoint to {path}")
    step = max(start_step, max_steps)
    final = ckpt_dir / "ckpt_final.pt"
    if place.first:
        trainer.save_checkpoint(str(final), step)
        print(f"\nTraining complete. Final checkpoint: {final}")
        log.close()
    trainer._device_sync()
    out = {"step": step, "losses": losses, "checkpoint": str(final), "digest": launch.state_digest((trainer.opt_G, trainer.opt_D))}
    if dp:
        out.update(rank=place.rank, world=N)
        print(f"[rank {place.rank}/{N}] state digest {out['digest']}", file=sys.stderr, flush=True)     # equal on all ranks
    return out


if __name__ == "__main__":
    main()
