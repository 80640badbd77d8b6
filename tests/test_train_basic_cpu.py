"""train_basic.main, the CycleGAN driver with the reference's command line (Basic_GAN/src/train.py:33-144), host logic on the CPU: the
iteration runs on the emulator, the transform hook stands in for the device pipeline with the Pillow restatement.  Epoch loop,
scheduler, checkpoint names and layout, the data order of Basic_GAN/src/data.py:43-74, the ragged tail and --resume."""
import os
import random

import numpy as np
import pytest
import torch
import yaml

from gan_variant_research_amd import basic as BG, cut as C, dataio, train_basic as TB
from oracle import input_ref as R
from tests.emulator import EmuOps
from tests.test_train_folder_cpu import write_folder

A_SIZES = [(40, 48), (33, 57), (64, 64), (37, 36), (50, 41)]
B_SIZES = [(36, 36), (45, 39), (38, 70)]
CKPT_KEYS = ["epoch", "G_A2B", "G_B2A", "D_A", "D_B", "optim_G", "optim_D_A", "optim_D_B"]       # train.py:127-137
BASE_LR = 2e-4


def config(tmp_path):
    """Basic_GAN/configs/baseline.yaml's schema with the sizes of this test."""
    return {"data": {"root": str(tmp_path / "data"), "domain_a": "photo_jpg", "domain_b": "monet_jpg", "img_size": 32, "load_size": 36, "num_workers": 0},
            "training": {"epochs": 3, "batch_size": 2, "amp": False, "seed": 0, "save_dir": str(tmp_path / "ck"), "log_dir": str(tmp_path / "runs"), "save_every": 2},
            "optim": {"lr_g": BASE_LR, "lr_d": BASE_LR, "betas": [0.5, 0.999], "lr_decay_after": 1},
            "loss": {"gan": "lsgan", "lambda_cycle": 10.0, "lambda_identity": 0.5},
            "model": {"ngf": 8, "ndf": 8, "n_blocks": 6, "spectral_norm_d": False},
            "runtime": {"device": "cuda"}}


def pillow_transform(image_size, device):
    return lambda images, jobs: torch.from_numpy(np.stack([R.apply(im.numpy(), job) for im, job in zip(images, jobs)]))


def run(tmp_path, monkeypatch, extra=()):
    """One run of the driver; returns its result and the (A numbers, B numbers, A jobs, B jobs) it drew per batch."""
    drawn = []
    draw = TB.draw_batch
    monkeypatch.setattr(TB, "draw_batch", lambda *a: drawn.append(draw(*a)) or drawn[-1])
    r = TB.main(["--config", str(tmp_path / "cfg.yaml")] + list(extra), ops=EmuOps(), device="cpu", transform=pillow_transform)
    monkeypatch.setattr(TB, "draw_batch", draw)
    return r, drawn


def restated_sequence(cfg, epochs):
    """data.py:43-74 with a plain DataLoader over the item numbers: shuffled epochs of max(len A, len B) items; per item A's transform,
    then `random.randint` for B, then B's transform; after the seeding and the model construction of train.py:35-40."""
    C.set_seed(cfg["training"]["seed"])
    BG.build_models(cfg, "cpu")
    n = max(len(A_SIZES), len(B_SIZES))
    loader = torch.utils.data.DataLoader(list(range(n)), batch_size=cfg["training"]["batch_size"], shuffle=True, num_workers=0, collate_fn=lambda b: b)
    out = []
    for _ in range(epochs):
        for items in loader:
            if len(items) < cfg["training"]["batch_size"]:
                continue
            ia, ib, ja, jb = [], [], [], []
            for idx in items:
                ia.append(idx % len(A_SIZES))
                ja.append(dataio.basic_job(*A_SIZES[ia[-1]], cfg["data"]["load_size"], cfg["data"]["img_size"], train=True))
                ib.append(random.randint(0, len(B_SIZES) - 1))
                jb.append(dataio.basic_job(*B_SIZES[ib[-1]], cfg["data"]["load_size"], cfg["data"]["img_size"], train=True))
            out.append((ia, ib, ja, jb))
    return out


def test_cli_defaults_match_the_reference():
    a = TB.parse_args([])
    assert a.config == "configs/baseline.yaml" and a.resume is None and a.set == [] and a.synthetic is False


def test_list_images_is_the_references_listing(tmp_path):
    d = tmp_path / "r" / "a"
    (d / "sub.png").mkdir(parents=True)
    for name in ("b.JPG", "a.png", "c.jpeg", "d.bmp", "e.txt"):
        (d / name).write_bytes(b"")
    (d / "sub.png" / "z.png").write_bytes(b"")
    assert [os.path.basename(p) for p in TB.list_images(str(tmp_path / "r"), "a")] == ["a.png", "b.JPG", "c.jpeg"]
    with pytest.raises(FileNotFoundError, match="nowhere"):
        TB.main(["--config", _write_cfg(tmp_path, config(tmp_path)), "--set", "data.domain_a=nowhere"], ops=EmuOps(), device="cpu", transform=pillow_transform)


def _write_cfg(tmp_path, cfg):
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def test_epochs_checkpoints_schedule_order_and_resume(tmp_path, monkeypatch, capsys):
    torch.set_num_threads(4)
    cfg = config(tmp_path)
    _write_cfg(tmp_path, cfg)
    write_folder(tmp_path / "data" / "photo_jpg", A_SIZES, 1)
    write_folder(tmp_path / "data" / "monet_jpg", B_SIZES, 2)
    ck_dir = cfg["training"]["save_dir"]

    r, drawn = run(tmp_path, monkeypatch)
    text = capsys.readouterr().out
    # two full batches per epoch out of five items; the one left out is reported, once
    assert len(drawn) == 6 and text.count("left out") == 1 and "the last 1 item(s) of every epoch are left out" in text
    assert all(f"Epoch {e}/3: 2 iterations" in text for e in (1, 2, 3))
    assert r["epoch"] == 3 and set(r["losses"]) == {"loss_G", "loss_D_A", "loss_D_B"} and all(np.isfinite(v) for v in r["losses"].values())
    assert sorted(os.listdir(ck_dir)) == ["ckpt_e2.pt", "ckpt_e3.pt"]
    assert r["checkpoints"] == [os.path.join(ck_dir, "ckpt_e2.pt"), os.path.join(ck_dir, "ckpt_e3.pt")]
    for e in (2, 3):
        ck = torch.load(os.path.join(ck_dir, f"ckpt_e{e}.pt"), weights_only=True)
        assert list(ck) == CKPT_KEYS and ck["epoch"] == e
        assert all(int(s["step"]) == 2 * e for s in ck["optim_G"]["state"].values())
    # the rates after each epoch: LambdaLR on lambda_rule (train.py:27-31, 54-58, 125)
    assert [h["epoch"] for h in r["history"]] == [1, 2, 3]
    for h in r["history"]:
        assert h["lr"] == [BASE_LR * BG.lambda_rule(h["epoch"], 1, 3)] * 3
    assert r["lr"] == r["history"][-1]["lr"] == [0.0, 0.0, 0.0] and r["history"][1]["lr"][0] == BASE_LR * 0.5
    # torch.optim.Adam takes the optimiser state as saved
    G1, G2, _, _ = BG.build_models(cfg, "cpu")
    torch.optim.Adam(list(G1.parameters()) + list(G2.parameters()), lr=BASE_LR, betas=(0.5, 0.999)).load_state_dict(ck["optim_G"])

    # the data order: what the reference's dataset and loader draw, and the same again for the same seed
    want = restated_sequence(cfg, 3)
    assert drawn == want
    for ia, ib, ja, jb in drawn:
        assert all(0 <= a < 5 for a in ia) and all(0 <= b < 3 for b in ib)
        assert [j["size"] for j in ja] == [A_SIZES[a] for a in ia] and [j["size"] for j in jb] == [B_SIZES[b] for b in ib]
    assert len({tuple(ia) for ia, _, _, _ in drawn}) > 1             # shuffled: not one fixed batch
    first = torch.load(os.path.join(ck_dir, "ckpt_e3.pt"), weights_only=True)
    r2, drawn2 = run(tmp_path, monkeypatch)
    assert drawn2 == drawn and r2["losses"] == r["losses"]

    # --resume (build-only): epoch 3 alone, the schedulers' counter and Adam's step counts continue
    os.remove(os.path.join(ck_dir, "ckpt_e3.pt"))
    capsys.readouterr()
    r3, drawn3 = run(tmp_path, monkeypatch, ["--resume", os.path.join(ck_dir, "ckpt_e2.pt")])
    text = capsys.readouterr().out
    assert "Resumed from epoch 2" in text and "Epoch 3/3" in text and "Epoch 2/3" not in text and len(drawn3) == 2
    assert r3["epoch"] == 3 and [h["epoch"] for h in r3["history"]] == [3] and r3["lr"] == [0.0, 0.0, 0.0]
    assert r3["checkpoints"] == [os.path.join(ck_dir, "ckpt_e3.pt")]
    resumed = torch.load(os.path.join(ck_dir, "ckpt_e3.pt"), weights_only=True)
    assert resumed["epoch"] == 3
    for key in ("optim_G", "optim_D_A", "optim_D_B"):
        assert [int(s["step"]) for s in resumed[key]["state"].values()] == [int(s["step"]) for s in first[key]["state"].values()]
        assert all(int(s["step"]) == 6 for s in resumed[key]["state"].values())
        assert resumed[key]["param_groups"][0]["lr"] == first[key]["param_groups"][0]["lr"] == 0.0
