"""CycleGAN training driver with the reference's command line (Basic_GAN/src/train.py:33-144):

    python -m gan_variant_research_amd.train_basic --config Basic_GAN/configs/baseline.yaml [--resume CKPT] [--set a.b=c ...] [--synthetic]

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
"""
from __future__ import annotations

import argparse
import os
import random
from typing import List, Optional

import torch
import torch.utils.data
import yaml

from . import basic as BG
from . import dataio
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
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    cfg = override_config(cfg, args.set)
    tr_cfg, data = cfg["training"], cfg["data"]
    set_seed(tr_cfg["seed"])
    device = torch.device(device if device is not None else (cfg.get("runtime") or {}).get("device", "cuda"))
    print(f"Using device: {device}")
    B, S, load_size = int(tr_cfg["batch_size"]), int(data["img_size"]), int(data["load_size"])
    synthetic = bool(args.synthetic or (cfg.get("mi355x") or {}).get("synthetic", False))
    if synthetic:
        print("[train_basic] --synthetic: uniform-noise batches stand in for the data loader")
        n_items = SYNTHETIC_ITEMS
        g = torch.Generator().manual_seed(1234)
    else:
        folder_a, folder_b = os.path.join(data["root"], data["domain_a"]), os.path.join(data["root"], data["domain_b"])
        store_a = build_store(list_images(data["root"], data["domain_a"]), device, cfg, "domain_a", folder_a)
        store_b = build_store(list_images(data["root"], data["domain_b"]), device, cfg, "domain_b", folder_b)
        n_items = max(len(store_a), len(store_b))
        make_tf = transform if transform is not None else (lambda size, dev: default_transform(size, dev, max_batch=max(B, 16)))
        tf_a, tf_b = make_tf(S, device), make_tf(S, device)
        loader = make_loader(n_items, B)
    if n_items < B:
        raise ValueError(f"an epoch has {n_items} items, fewer than training.batch_size = {B}")
    if n_items % B:
        print(f"[train_basic] {n_items} items per epoch, batch_size {B}: the last {n_items % B} item(s) of every epoch are left out "
              "(the trainer's buffers hold full batches only)")

    mods = BG.build_models(cfg, "cpu")
    trainer = BG.CycleGANTrainer(*[m.to(device) for m in mods], cfg, B, S, device=device, amp=tr_cfg["amp"], ops=ops)
    start_epoch = 1
    if args.resume:
        start_epoch = int(trainer.load_checkpoint(args.resume)) + 1
        print(f"Resumed from epoch {start_epoch - 1}")
    total_epochs, save_dir = int(tr_cfg["epochs"]), tr_cfg["save_dir"]
    os.makedirs(save_dir, exist_ok=True)

    def batches():
        if synthetic:
            for _ in range(n_items // B):
                yield (torch.rand(2, B, 3, S, S, generator=g) * 2 - 1).to(device)
            return
        for items in loader:
            if len(items) < B:
                continue
            ia, ib, jobs_a, jobs_b = draw_batch(items, store_a.sizes, store_b.sizes, load_size, S)
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
        print(f"Epoch {epoch}/{total_epochs}: {n} iterations, " + ", ".join(f"{k[5:]} {v:.3f}" for k, v in means.items()))
        trainer.scheduler_step()          # epoch end: schedulers + checkpoint (train.py:124-137)
        if epoch % tr_cfg["save_every"] == 0 or epoch == total_epochs:
            path = os.path.join(save_dir, f"ckpt_e{epoch}.pt")
            trainer.save_checkpoint(path, epoch)
            checkpoints.append(path)
            print(f"Saved checkpoint to {path}")
        history.append({"epoch": epoch, "losses": means, "lr": rates()})
    return {"epoch": epoch, "losses": means, "checkpoints": checkpoints, "lr": rates(), "history": history}


if __name__ == "__main__":
    main()
