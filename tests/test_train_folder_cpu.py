"""train_cutpp.main on real image folders (no --synthetic), host logic on the CPU: the step runs on the emulator, the transform hook
stands in for the device pipeline with the Pillow restatement (oracle.input_ref).  What the trainer is fed must be the documented
loader -- per epoch a permutation from random.Random(seed) (photos) / random.Random(seed + 1) (monet), drop_last, one train_job per
image in order -- replayed here through Pillow itself."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from gan_variant_research_amd import _lib, cut as C, dataio, train_cutpp as T
from oracle import input_ref as R
from tests.emulator import EmuOps
from tests.test_train_driver import SCHEMA

PHOTO_SIZES = [(40, 48), (33, 57), (64, 64), (35, 34), (50, 41)]
MONET_SIZES = [(36, 36), (45, 39), (34, 70)]


def write_folder(root, sizes, seed):
    rng = np.random.default_rng(seed)
    root.mkdir(parents=True)
    for n, (h, w) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / f"img_{n:02d}.png")
    return sorted(root.iterdir())


class PillowTransform:
    """The transform hook: `dataio._Transform` with oracle.input_ref.apply in place of the device pipeline."""

    def __init__(self, image_size, device):
        self.image_size, self.last_jobs, self.calls = image_size, [], []

    def __call__(self, images):
        self.last_jobs = [dataio.train_job(int(im.shape[0]), int(im.shape[1]), self.image_size) for im in images]
        out = torch.from_numpy(np.stack([R.apply(im.numpy(), job) for im, job in zip(images, self.last_jobs)]))
        self.calls.append(([im.numpy().copy() for im in images], self.last_jobs, out))
        return out


def loader_order(n, batch, seed, steps):
    """folder_batches' documented order: the image numbers of the first `steps` batches."""
    rng, out = random.Random(seed), []
    while len(out) < steps:
        order = list(range(n))
        rng.shuffle(order)
        out += [order[i:i + batch] for i in range(0, n - batch + 1, batch)]
    return out[:steps]


def run_driver(tmp_path, monkeypatch, ops, device, transform, image_size, sets=(), photo_sizes=PHOTO_SIZES, monet_sizes=MONET_SIZES):
    cfg_path = str(tmp_path / "cfg.yaml")
    with open(cfg_path, "w") as f:
        f.write(SCHEMA)
    photos, monets = write_folder(tmp_path / "photos", photo_sizes, 1), write_folder(tmp_path / "monet", monet_sizes, 2)
    ck, lg = str(tmp_path / "ck"), str(tmp_path / "lg")
    fed = []
    step = C.CutTrainer.train_step
    monkeypatch.setattr(C.CutTrainer, "train_step", lambda self, s, p, m, *a, **kw: fed.append((s, p.clone(), m.clone())) or step(self, s, p, m, *a, **kw))
    tfs = []
    factory = None if transform is None else (lambda size, dev: tfs.append(transform(size, dev)) or tfs[-1])
    sets = [f"image_size={image_size}", "batch_size=2", "max_steps=2", "amp=false", f"output.checkpoint_dir={ck}", f"output.log_dir={lg}",
            f"data.photos_dir={tmp_path / 'photos'}", f"data.monet_dir={tmp_path / 'monet'}"] + list(sets)
    r = T.main(["--config", cfg_path, "--set"] + sets, ops=ops, device=device, transform=factory)
    return r, fed, tfs, (photos, monets), (ck, lg)


def check_fed_batches(fed, tfs, paths, image_size, seed=42):
    """The two steps' batches against Pillow: the files the documented order names, through the recorded jobs."""
    assert [s for s, _, _ in fed] == [0, 1] and len(tfs) == 2
    for dom, (tf, files, sd) in enumerate(zip(tfs, paths, (seed, seed + 1))):
        assert len(tf.calls) == 2                    # exactly the batches of the two steps were prepared
        for k, (order, (images, jobs, out)) in enumerate(zip(loader_order(len(files), 2, sd, 2), tf.calls)):
            got = fed[k][1 + dom].cpu().numpy()
            assert got.shape == (2, 3, image_size, image_size) and got.dtype == np.float32
            for b, (i, job) in enumerate(zip(order, jobs)):
                src = np.array(Image.open(files[i]).convert("RGB"))
                assert np.array_equal(images[b], src) and job["size"] == src.shape[:2]
                assert np.array_equal(got[b], R.apply_pil(src, job)), (dom, k, b)


def test_folder_training_on_the_emulator(tmp_path, monkeypatch, capsys):
    torch.set_num_threads(4)
    r, fed, tfs, paths, (ck, lg) = run_driver(tmp_path, monkeypatch, EmuOps(), "cpu", PillowTransform, 32)
    assert r["step"] == 2 and all(np.isfinite(v) for v in r["losses"].values())
    assert sorted(os.listdir(ck)) == ["ckpt_final.pt"] and torch.load(os.path.join(ck, "ckpt_final.pt"), weights_only=True)["step"] == 2
    rows = open(os.path.join(lg, "losses_history.csv")).read().strip().splitlines()
    assert rows[0] == "step,d_loss,g_loss" and [ln.split(",")[0] for ln in rows[1:]] == ["0", "1"]
    assert float(rows[2].split(",")[2]) == r["losses"]["g_loss"]
    check_fed_batches(fed, tfs, paths, 32)
    text = capsys.readouterr().out
    assert "photos: 5 images" in text and "monet: 3 images" in text and "resident" in text and "Photos: 5, Monet: 3" in text


def test_streaming_store_feeds_the_same_batches(tmp_path, monkeypatch, capsys):
    torch.set_num_threads(4)
    _, fed, tfs, paths, _ = run_driver(tmp_path, monkeypatch, EmuOps(), "cpu", PillowTransform, 32, sets=["mi355x.dataset_cache_gb=0"])
    check_fed_batches(fed, tfs, paths, 32)
    assert "streaming" in capsys.readouterr().out


def test_folder_path_without_the_hook_needs_the_gpu(tmp_path, monkeypatch):
    with pytest.raises(_lib.GanError, match="runs on the GPU"):
        run_driver(tmp_path, monkeypatch, EmuOps(), "cpu", None, 32)
