"""The two training command lines on real image folders on the GPU (fp32, tiny runs): train_cutpp feeds the trainer exactly the Pillow
replay of its recorded jobs; train_basic writes the reference's checkpoints on the reference's schedule, and its checkpoint loads into
inference (basic.ResnetGenerator, forward_u8, stylize_folder on the device)."""
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from gan_variant_research_amd import basic as BG, inference as I, train_basic as TB, train_cutpp as T
from tests.test_train_basic_cpu import BASE_LR, CKPT_KEYS, config
from tests.test_train_folder_cpu import check_fed_batches, run_driver, write_folder

PHOTO_SIZES = [(80, 96), (67, 115), (128, 128), (70, 71)]
MONET_SIZES = [(72, 72), (90, 79), (68, 140)]


class RecordingTransform:
    """The driver's own device transform, keeping what went in and came out of every call."""

    def __init__(self, image_size, device):
        self.tf, self.calls = T.default_transform(image_size, device, max_batch=16), []

    def __call__(self, images):
        out = self.tf(images)
        self.calls.append(([im.cpu().numpy() for im in images], self.tf.last_jobs, out.clone()))
        return out


@pytest.mark.gpu
def test_train_cutpp_on_folders(tmp_path, monkeypatch):
    r, fed, tfs, paths, (ck, lg) = run_driver(tmp_path, monkeypatch, None, None, RecordingTransform, 64, photo_sizes=PHOTO_SIZES, monet_sizes=MONET_SIZES)
    assert r["step"] == 2 and all(np.isfinite(v) for v in r["losses"].values()) and os.path.exists(os.path.join(ck, "ckpt_final.pt"))
    rows = open(os.path.join(lg, "losses_history.csv")).read().strip().splitlines()
    assert [ln.split(",")[0] for ln in rows[1:]] == ["0", "1"] and all(np.isfinite(float(v)) for ln in rows[1:] for v in ln.split(",")[1:])
    assert all(t.is_cuda for _, p, m in fed for t in (p, m))
    check_fed_batches(fed, tfs, paths, 64)


@pytest.fixture(scope="module")
def basic_run(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("basic_gpu")
    cfg = config(tmp_path)
    cfg["data"].update({"img_size": 64, "load_size": 72})
    cfg["training"].update({"epochs": 2, "save_every": 1})
    cfg["model"].update({"ngf": 64, "ndf": 64, "n_blocks": 9})
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    photos = write_folder(tmp_path / "data" / "photo_jpg", PHOTO_SIZES, 1)
    write_folder(tmp_path / "data" / "monet_jpg", MONET_SIZES, 2)
    return TB.main(["--config", str(tmp_path / "cfg.yaml")]), cfg, tmp_path, photos


@pytest.mark.gpu
def test_train_basic_on_folders(basic_run):
    r, cfg, tmp_path, _ = basic_run
    ck_dir = cfg["training"]["save_dir"]
    assert r["epoch"] == 2 and sorted(os.listdir(ck_dir)) == ["ckpt_e1.pt", "ckpt_e2.pt"]
    assert all(np.isfinite(v) for h in r["history"] for v in h["losses"].values()) and set(r["losses"]) == {"loss_G", "loss_D_A", "loss_D_B"}
    assert r["history"][0]["lr"] == [BASE_LR * BG.lambda_rule(1, 1, 2)] * 3 == [BASE_LR] * 3        # the rate epoch 2 ran at
    assert r["lr"] == [BASE_LR * BG.lambda_rule(2, 1, 2)] * 3
    ck = torch.load(os.path.join(ck_dir, "ckpt_e2.pt"), map_location="cpu", weights_only=True)
    assert list(ck) == CKPT_KEYS and ck["epoch"] == 2 and all(int(s["step"]) == 4 for s in ck["optim_G"]["state"].values())
    assert all(bool(torch.isfinite(v).all()) for v in ck["G_A2B"].values())


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["G_A2B", "G_B2A"])
def test_checkpoint_of_train_basic_stylizes(basic_run, which):
    _, cfg, tmp_path, photos = basic_run
    path = os.path.join(cfg["training"]["save_dir"], "ckpt_e2.pt")
    G = I.load_generator(path, bf16=False, which=which)
    want = torch.load(path, map_location="cpu", weights_only=True)[which]
    assert type(G) is BG.ResnetGenerator and G.n_blocks == 9 and all(torch.equal(v.cpu(), want[k]) for k, v in G.state_dict().items())
    g = torch.Generator().manual_seed(8)
    for shape in ((1, 3, 16, 16), (2, 3, 32, 32)):
        x = (torch.rand(shape, generator=g) * 2 - 1).cuda()
        with torch.no_grad():
            ref = I.to_uint8(G(x)).permute(0, 2, 3, 1)
        got = G.forward_u8(x)
        assert got.shape == ref.shape and got.is_contiguous() and torch.equal(got, ref) and torch.equal(I.stylize_hwc(G, x), ref)
        assert len(set(ref.flatten().tolist())) > 8
    out = tmp_path / f"out_{which}"
    assert I.stylize_folder(G, str(tmp_path / "data" / "photo_jpg"), str(out), device="cuda", img_size=32, batch=3, device_io=True) == len(photos)
    assert sorted(p.name for p in out.iterdir()) == [p.with_suffix(".jpg").name for p in photos]
    assert all(Image.open(p).size == (32, 32) for p in out.iterdir())
