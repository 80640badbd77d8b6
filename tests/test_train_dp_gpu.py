"""`--gpus N` of the two training drivers on the device.  Every run is a fresh child process under its own timeout (a process group is
created once per process); after a failed child nothing further is started by that test.  64x64, batch 2, three steps with lazy R1 on
every second one, folders of eight PNGs."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import cases
from tests.test_train_basic_cpu import config as basic_config
from tests.test_train_folder_cpu import write_folder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 64
PHOTO_SIZES = [(80, 96), (67, 115), (128, 128), (70, 71), (100, 82), (72, 78), (94, 66), (84, 84)]
MONET_SIZES = [(72, 72), (90, 79), (68, 140), (104, 74), (66, 66), (82, 120), (76, 70), (98, 88)]
LR = 2e-4
RENDEZVOUS = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")


def child(module, argv, env=None):
    base = {k: v for k, v in os.environ.items() if k not in RENDEZVOUS}
    r = subprocess.run([sys.executable, "-m", f"gan_variant_research_amd.{module}", *argv], cwd=ROOT, env=dict(base, **(env or {})),
                       capture_output=True, text=True, timeout=300)
    return r


def one_rank_env():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    return {"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": port}


def same_tensors(a, b, path="ckpt"):
    """Nested containers equal, tensors by torch.equal."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            same_tensors(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same_tensors(x, y, f"{path}[{i}]")
    elif torch.is_tensor(a):
        assert torch.equal(a, b), path
    else:
        assert a == b, path


@pytest.fixture(scope="module")
def cut_data(tmp_path_factory):
    root = tmp_path_factory.mktemp("dp_cut_gpu")
    cfg = cases.small_config()
    cfg.update({"seed": 42, "epochs": 1, "log_every": 100, "metrics": {"save_checkpoint_every": 1000}})
    cfg["r1"]["every"] = 2
    with open(root / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    write_folder(root / "photos", PHOTO_SIZES, 1)
    write_folder(root / "monet", MONET_SIZES, 2)
    return root


def cut_argv(root, tag, batch, steps, amp, extra=()):
    out = root / tag
    return ["--config", str(root / "cfg.yaml"), *extra, "--set", f"image_size={S}", f"batch_size={batch}", f"max_steps={steps}",
            f"amp={'true' if amp else 'false'}", f"output.checkpoint_dir={out / 'ck'}", f"output.log_dir={out / 'lg'}",
            f"data.photos_dir={root / 'photos'}", f"data.monet_dir={root / 'monet'}"]


@pytest.mark.gpu
def test_train_cutpp_in_a_one_rank_group_changes_nothing(cut_data):
    """RCCL initialisation after the stream binding, the gradient all-reduces, the loss all-reduce in front of the lagged read-back and
    the rank-0 gating, at the smallest size: sums over one rank are the same bits, so the files are the plain run's."""
    plain = child("train_cutpp", cut_argv(cut_data, "plain", 2, 3, True))
    assert plain.returncode == 0, plain.stderr[-2000:]
    group = child("train_cutpp", cut_argv(cut_data, "group", 2, 3, True), env=one_rank_env())
    assert group.returncode == 0, group.stderr[-2000:]
    assert "1 rank(s)" in group.stdout and "rank(s)" not in plain.stdout
    a, b = (open(cut_data / t / "lg" / "losses_history.csv", "rb").read() for t in ("plain", "group"))
    assert a == b and len(a.splitlines()) == 4
    assert all(np.isfinite(float(v)) for ln in a.decode().splitlines()[1:] for v in ln.split(","))
    load = lambda t: torch.load(cut_data / t / "ck" / "ckpt_final.pt", map_location="cpu", weights_only=True)
    ck_a, ck_b = load("plain"), load("group")
    for ck, t in ((ck_a, "plain"), (ck_b, "group")):           # the two runs differ in their output paths only
        ck["config"]["output"] = None
    same_tensors(ck_a, ck_b)


@pytest.mark.gpu
def test_train_basic_in_a_one_rank_group_changes_nothing(tmp_path):
    write_folder(tmp_path / "data" / "photo_jpg", PHOTO_SIZES[:4], 1)
    write_folder(tmp_path / "data" / "monet_jpg", MONET_SIZES[:3], 2)
    runs = {}
    for tag, env in (("plain", None), ("group", one_rank_env())):
        cfg = basic_config(tmp_path)
        cfg["data"].update({"img_size": S, "load_size": 72})
        cfg["training"].update({"epochs": 1, "save_every": 1, "batch_size": 2, "save_dir": str(tmp_path / tag)})
        cfg["model"].update({"ngf": 64, "ndf": 64, "n_blocks": 9})
        with open(tmp_path / f"{tag}.yaml", "w") as f:
            yaml.safe_dump(cfg, f)
        r = child("train_basic", ["--config", str(tmp_path / f"{tag}.yaml")], env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[tag] = r.stdout
    assert "Epoch 1/1: 2 iterations" in runs["plain"] and "1 rank(s)" in runs["group"]
    epoch_line = lambda text: [ln for ln in text.splitlines() if ln.startswith("Epoch 1/1")]
    assert epoch_line(runs["plain"]) == epoch_line(runs["group"])            # the epoch's mean losses, as printed
    load = lambda t: torch.load(tmp_path / t / "ckpt_e1.pt", map_location="cpu", weights_only=True)
    same_tensors(load("plain"), load("group"))


def digests(stderr):
    return re.findall(r"\[rank (\d+)/(\d+)\] state digest ([0-9a-f]{64})", stderr)


@pytest.mark.gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (one RCCL rank per GPU)")
def test_two_gpus_at_batch_1_equal_one_gpu_at_batch_2(cut_data):
    """`--gpus 2 --set batch_size=1` against the plain run at batch_size=2, one step, fp32: losses within the tolerance of
    tests/test_gpu_parity.py::test_two_gpu_ranks_equal_one_rank, parameters within Adam's first-update sign flip (2 lr, as
    tests/test_dp_gloo.py states it: 4.5e-4 for G, twice for D with its R1 update), and both ranks hold the same state."""
    single = child("train_cutpp", cut_argv(cut_data, "one", 2, 1, False))
    assert single.returncode == 0, single.stderr[-2000:]
    two = child("train_cutpp", cut_argv(cut_data, "two", 1, 1, False, extra=["--gpus", "2"]))
    assert two.returncode == 0, two.stderr[-2000:]
    d = digests(two.stderr)
    assert sorted(r for r, _, _ in d) == ["0", "1"] and d[0][2] == d[1][2], d
    row = lambda t: [float(v) for v in open(cut_data / t / "lg" / "losses_history.csv").read().strip().splitlines()[1].split(",")[1:]]
    np.testing.assert_allclose(row("two"), row("one"), rtol=1e-3, atol=1e-4)
    load = lambda t: torch.load(cut_data / t / "ck" / "ckpt_final.pt", map_location="cpu", weights_only=True)
    a, b = load("two"), load("one")
    for key, atol in (("generator", 4.5e-4), ("discriminator", 9e-4)):
        for k in b[key]:
            np.testing.assert_allclose(a[key][k].numpy(), b[key][k].numpy(), rtol=0, atol=atol, err_msg=f"{key}.{k}")


@pytest.mark.gpu
def test_more_ranks_than_gpus_is_refused_before_any_rank_starts(cut_data):
    n = torch.cuda.device_count() + 1
    r = child("train_cutpp", cut_argv(cut_data, "refused", 1, 1, False, extra=["--gpus", str(n)]))
    assert r.returncode != 0
    assert (f"--gpus {n} but this machine shows {n - 1} GPU(s); no rank was started" in r.stderr) or "at most 8 ranks" in r.stderr
    assert "Using device" not in r.stdout and not os.path.exists(cut_data / "refused")
