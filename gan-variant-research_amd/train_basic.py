"""CycleGAN training driver with the reference's command line (Basic_GAN/src/train.py:33-144):

    python -m gan_variant_research_amd.train_basic --config Basic_GAN/configs/baseline.yaml [--resume CKPT] [--set a.b=c ...] [--synthetic] [--gpus N]

`--config` is the reference's only flag (default `configs/baseline.yaml`, train.py:142); the YAML schema, the epoch loop (schedulers
at every epoch end, `ckpt_e{epoch}.pt` every `save_every` epochs and at the last one) and the checkpoint layout are the reference's.
What runs underneath is the fused `basic.CycleGANTrainer` on the HIP kernels; the two image folders are decoded once into
`dataio.ImageStore`s and transformed on the device (`dataio.basic_job`, the `_image_tf` of Basic_GAN/src/data.py:8-26).

The data order restates Basic_GAN/src/data.py:43-74 with `num_workers: 0` (the shipped value): an epoch has max(len A, len B) items in
the order of a `DataLoader(shuffle=True)` -- a real one over the item numbers, so the sampler's draws are PyTorch's own -- and per item
A is `idx % len A` with its transform drawn first, then B's index from `random.randint(0, len B - 1)`, then B's transform.

Where this driver departs from the reference:
  * --resume, --set and --synthetic are build-only flags.  The reference has no resume: `--resume CKPT` loads the checkpoint with
    `CycleGANTrainer.load_checkpoint` (weights, Adam states, the schedulers' epoch counter) and continues at `epoch + 1`.
  * Ragged last batch: the trainer's buffers are fixed at `batch_size`, the reference's loader has no `drop_last`.  When
    max(len A, len B) is no multiple of `batch_size`, only the full batches of an epoch run; the driver prints once how many items per
    epoch that leaves out (none are drawn for them).  With the shipped `batch_size: 1` the count is zero.
  * The progress bar's per-iteration losses (train.py:118-122) are printed as epoch means.
  * `--gpus N` (build-only flag; launch.py) trains data-parallel on N GPUs of one node.  `training.batch_size` stays the per-GPU batch;
    the loader batches N x batch_size items, every rank draws the whole global batch in order (`draw_batch`: Python's `random` moves as
    in one process at that batch size) and fetches and transforms its own rows, so N ranks x B are one process at batch N B.  Only full
    global batches run.  Rank 0 alone prints and saves, the losses are those of the global batch; checkpoints do not depend on N.
    Every rank holds its own ImageStores (sharding them across ranks is not done) with 16 // N decode threads.
"""
from __future__ import annotations

import argparse
import os
import random
import sys
from typing import List, Optional

import torch
import torch.utils.data
import yaml

from . import basic as BG
from . import dataio
from . import launch
from .cut import set_seed
from .train_cutpp import build_store, override_config

IMAGE_EXTS = (".jpg", ".jpeg", ".png")          # data.py:32
SYNTHETIC_ITEMS = 7038                          # the photo count of the data both reference configs point at


def parse_args(argv=None):
    """train.py:140-143, plus the build-only flags."""
    ap = argparse.ArgumentParser(description="Train the CycleGAN baseline (MI355X-native step)")
    ap.add_argument("--config", type=str, default="configs/baseline.yaml")
    ap.add_argument("--resume", type=str, default=None, help="checkpoint to continue from (build-only flag)")
    ap.add_argument("--set", nargs="+", default=[], help="override config values, e.g. training.epochs=2 (build-only flag)")
    ap.add_argument("--synthetic", action="store_true", help="uniform-noise batches instead of the image folders (build-only flag)")
    launch.add_arguments(ap)
    return ap.parse_args(argv)


def list_images(root: str, subdir: str) -> List[str]:
    """data.py:29-33: the files of one folder ending in .jpg / .jpeg / .png, sorted; not recursive."""
    folder = os.path.join(root, subdir)
    if not os.path.isdir(folder):
        return []
    return sorted(p for p in (os.path.join(folder, f) for f in os.listdir(folder)) if os.path.isfile(p) and p.lower().endswith(IMAGE_EXTS))


class _Items(torch.utils.data.Dataset):
    """The item numbers 0 .. n-1: what the DataLoader shuffles and batches."""

    def __init__(self, n: int):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


def make_loader(n_items: int, batch_size: int):
    """data.py:68-74: shuffle=True, num_workers=0, no drop_last; the batches stay lists of item numbers."""
    return torch.utils.data.DataLoader(_Items(n_items), batch_size=batch_size, shuffle=True, num_workers=0, collate_fn=list)


def draw_batch(items, sizes_a, sizes_b, load_size: int, img_size: int):
    """UnpairedDataset.__getitem__ (data.py:55-58) for every item of a batch, in order: A's transform, B's index, B's transform."""
    ia, ib, jobs_a, jobs_b = [], [], [], []
    for idx in items:
        a = int(idx) % len(sizes_a)
        jobs_a.append(dataio.basic_job(*sizes_a[a], load_size, img_size, train=True))
        b = random.randint(0, len(sizes_b) - 1)
        jobs_b.append(dataio.basic_job(*sizes_b[b], load_size, img_size, train=True))
        ia.append(a)
        ib.append(b)
    return ia, ib, jobs_a, jobs_b


def default_transform(image_size: int, device, max_batch: int = 64):
    """`callable(images, jobs)` -> (B, 3, S, S) fp32 on the device pipeline."""
    pipe = dataio.InputPipeline(image_size, device, max_batch=max_batch)
    return pipe.run


def main(argv=None, ops=None, device: Optional[str] = None, transform=None) -> dict:
    """train.py:33-137.  `ops` / `device` / `transform` are test hooks: `transform(image_size, device)` returns the
    `callable(images, jobs)` that turns decoded uint8 (H, W, 3) images and their drawn jobs into the (B, 3, S, S) fp32 batch (default:
    the device pipeline; on a CPU device it raises that it runs on the GPU).  Returns the last epoch, its mean losses, the checkpoints
    written, the three current learning rates and the per-epoch history of losses and rates."""
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
        cfg = yaml.safe_load(f)
    cfg = override_config(cfg, args.set)
    set_seed(cfg["training"]["seed"])
    with launch.join(world, device if device is not None else (cfg.get("runtime") or {}).get("device", "cuda"), ops) as place:
        return _train(args, cfg, place, transform)


def _train(args, cfg: dict, place, transform) -> dict:
    """One rank's run (the only one without --gpus): `place.group` is None in the plain single-process run, which then does what it
    always did.  With a group, N ranks x batch B are one process at batch N B (module docstring); rank 0 prints and saves."""
    tr_cfg, data = cfg["training"], cfg["data"]
    device, ops, dp, N = place.device, place.ops, place.group is not None, place.world
    say = print if place.first else (lambda *a, **kw: None)
    say(f"Using device: {device}" + (f" ({N} rank(s), global batch {N * int(tr_cfg['batch_size'])})" if dp else ""))
    B, S, load_size = int(tr_cfg["batch_size"]), int(data["img_size"]), int(data["load_size"])
    whole, rows = N * B, place.rows(B)                         # the global batch and this rank's rows of it
    synthetic = bool(args.synthetic or (cfg.get("mi355x") or {}).get("synthetic", False))
    if synthetic:
        say("[train_basic] --synthetic: uniform-noise batches stand in for the data loader")
        n_items = SYNTHETIC_ITEMS
        g = torch.Generator().manual_seed(1234)
    else:
        folder_a, folder_b = os.path.join(data["root"], data["domain_a"]), os.path.join(data["root"], data["domain_b"])
        workers = max(1, 16 // N) if dp else None
        store_a = build_store(list_images(data["root"], data["domain_a"]), device, cfg, "domain_a", folder_a, workers, quiet=not place.first)
        store_b = build_store(list_images(data["root"], data["domain_b"]), device, cfg, "domain_b", folder_b, workers, quiet=not place.first)
        n_items = max(len(store_a), len(store_b))
        make_tf = transform if transform is not None else (lambda size, dev: default_transform(size, dev, max_batch=max(B, 16)))
        tf_a, tf_b = make_tf(S, device), make_tf(S, device)
        loader = make_loader(n_items, whole)
    if n_items < whole:
        raise ValueError(f"an epoch has {n_items} items, fewer than training.batch_size = {whole}" + (f" = {N} ranks x {B}" if dp else ""))
    if n_items % whole:
        say(f"[train_basic] {n_items} items per epoch, batch_size {whole}: the last {n_items % whole} item(s) of every epoch are left out "
            "(the trainer's buffers hold full batches only)")

    mods = BG.build_models(cfg, "cpu")
    if dp:
        trainer = BG.CycleGANTrainer(*[m.to(device) for m in mods], cfg, B, S, device=device, amp=tr_cfg["amp"], ops=ops, world_size=N,
                                     process_group=place.group, average_losses=True)
        trainer.force_allreduce = True       # a one-rank group runs the collectives too (sums over one rank: the same bits)
    else:
        trainer = BG.CycleGANTrainer(*[m.to(device) for m in mods], cfg, B, S, device=device, amp=tr_cfg["amp"], ops=ops)
    start_epoch = 1
    if args.resume:
        start_epoch = int(trainer.load_checkpoint(args.resume)) + 1
        say(f"Resumed from epoch {start_epoch - 1}")
    total_epochs, save_dir = int(tr_cfg["epochs"]), tr_cfg["save_dir"]
    if place.first:
        os.makedirs(save_dir, exist_ok=True)

    def batches():
        if synthetic:
            for _ in range(n_items // whole):
                x = torch.rand(2, whole, 3, S, S, generator=g) * 2 - 1
                yield (x[:, rows] if dp else x).to(device)
            return
        for items in loader:
            if len(items) < whole:
                continue
            ia, ib, jobs_a, jobs_b = draw_batch(items, store_a.sizes, store_b.sizes, load_size, S)      # the global batch, on every rank
            if dp:
                ia, ib, jobs_a, jobs_b = ia[rows], ib[rows], jobs_a[rows], jobs_b[rows]
            yield tf_a(store_a.fetch(ia), jobs_a), tf_b(store_b.fetch(ib), jobs_b)

    rates = lambda: [o.lr for o in (trainer.opt_G, trainer.opt_DA, trainer.opt_DB)]
    epoch, means, checkpoints, history = start_epoch - 1, {}, [], []
    for epoch in range(start_epoch, total_epochs + 1):
        sums, n = {}, 0
        for real_a, real_b in batches():
            losses = trainer.train_iteration(real_a, real_b, sync=True)
            for k, v in losses.items():
                sums[k] = sums.get(k, 0.0) + v
            n += 1
        means = {k: v / n for k, v in sums.items()}
        say(f"Epoch {epoch}/{total_epochs}: {n} iterations, " + ", ".join(f"{k[5:]} {v:.3f}" for k, v in means.items()))
        trainer.scheduler_step()          # epoch end: schedulers + checkpoint (train.py:124-137)
        if epoch % tr_cfg["save_every"] == 0 or epoch == total_epochs:
            path = os.path.join(save_dir, f"ckpt_e{epoch}.pt")
            if place.first:
                trainer.save_checkpoint(path, epoch)
                print(f"Saved checkpoint to {path}")
            checkpoints.append(path)
        history.append({"epoch": epoch, "losses": means, "lr": rates()})
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    out = {"epoch": epoch, "losses": means, "checkpoints": checkpoints, "lr": rates(), "history": history,
           "digest": launch.state_digest((trainer.opt_G, trainer.opt_DA, trainer.opt_DB))}
    if dp:
        out.update(rank=place.rank, world=N)
        print(f"[rank {place.rank}/{N}] state digest {out['digest']}", file=sys.stderr, flush=True)     # equal on all ranks
    return out


if __name__ == "__main__":
    main()
