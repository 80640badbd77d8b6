"""The folder path of gan_variant_research_amd.select_7k on the GPU: files -> decode -> resize -> extractor -> selection -> copied files.
Forty small generated JPEGs and PNGs in two candidate roots and a real folder of twelve; the extractor is tests/eval_extractor.py.  The
command runs with the Pillow pool and with both device decoders; the files it copies are those the feature-level `select` chooses
from the same features."""
import csv
import json

import numpy as np
import pytest
import torch

from gan_variant_research_amd import evaluate as E, select_7k as S
from tests import eval_extractor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def image(i):
    h, w = 24 + 8 * (i % 4), 40 - 8 * (i % 3)              # multiples of 8 and others, several sizes
    g = np.random.default_rng(700 + i)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // w), (y * 255 // h), ((x + y) * 255 // (h + w))], -1).astype(np.float64)
    return np.clip(base * (0.3 + 0.05 * (i % 13)) + g.normal(0, 25, (h, w, 3)) + 6 * (i % 9), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("select")
    for name, lo, n in (("real", 0, 12), ("cand_a", 100, 20), ("cand_b", 200, 20)):
        (root / name).mkdir()
        for i in range(n):
            if i % 2:
                Image.fromarray(image(lo + i)).save(root / name / f"{name}_{i:02d}.png")
            else:
                Image.fromarray(image(lo + i)).save(root / name / f"{name}_{i:02d}.jpg", quality=92)
    return root


@pytest.mark.parametrize("device_decoders", [False, True], ids=["pillow", "device"])
def test_command_copies_what_select_chooses(folders, tmp_path, device_decoders):
    real, a, b = folders / "real", folders / "cand_a", folders / "cand_b"
    extra = ["--device-decode", "--device-png"] if device_decoders else []
    out = tmp_path / "out"
    assert S.main(["--real", str(real), "--cand_roots", str(a), str(b), "--outdir", str(out), "--tau", "0.0", "--k", "4", "--target", "25", "--device", DEV,
                   "--batch", "16", "--img-size", "64", "--io-threads", "2", "--extractor", "tests.eval_extractor:make", *extra]) == 0
    ext = eval_extractor.make(torch.device(DEV))
    kw = dict(device=DEV, batch=16, img_size=64, io_threads=2, device_decode=device_decoders, device_png=device_decoders)
    feats = [E.extract_features(E.enumerate_images(d), ext, **kw) for d in (real, a, b)]
    cp = E.enumerate_images(a) + E.enumerate_images(b)
    want = S.select(feats[0], feats[1:], tau=0.0, k=4, target=25, device=DEV)
    assert len(cp) == 40 and len(want["chosen"]) == 25
    rows = list(csv.DictReader(open(out / "selection.csv")))
    assert [r["path"] for r in rows] == [str(cp[i]) for i in want["chosen"]]
    assert sorted(p.name for p in (out / "images").iterdir()) == sorted(cp[i].name for i in want["chosen"])
    for i in want["chosen"][:3]:
        assert (out / "images" / cp[i].name).read_bytes() == cp[i].read_bytes()
    meta = json.load(open(out / "selection_meta.json"))
    assert meta["selected"] == 25 and meta["candidates"] == 40 and meta["collisions"] == 0 and meta["k"] == 4
