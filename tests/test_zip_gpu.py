"""csrc/zip.hip on the device: `HipOps.crc32_ranges` against zlib on the case table of tests/zip_cases.py, `JpegEncoder.encode_block`
against `encode` (hence the Pillow goldens) with the device's CRCs against zlib, and the folder path / command line with an archive as
the output.  Offsets that leave the buffer are exercised by csrc/crc32_host.cpp on the CPU only; here every offset lies inside it."""
import os
import subprocess
import sys
import zipfile
import zlib

import numpy as np
import pytest
import torch

from gan_variant_research_amd import cut, inference as I
from gan_variant_research_amd.runtime import HipOps
from tests import jpeg_cases as JC, zip_cases as ZC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def table():
    buf, off, ids, want = ZC.table()
    return torch.from_numpy(buf.copy()).to(DEV), off, ids, want


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_crc32_of_the_case_table_in_one_launch(table):
    buf, off, ids, want = table
    ops, n = HipOps(DEV), len(ids)
    offsets = torch.from_numpy(off.copy()).to(DEV)
    crc = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)              # poisoned
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    op = ops.crc32_ranges(buf, offsets, crc, flag)
    op()
    got = _u32(crc)
    assert got.tolist() == want.tolist(), [ids[i] for i in np.flatnonzero(got != want)]
    assert int(flag.cpu()[0]) == 0
    crc.fill_(0x5A5A5A5A)
    op()
    assert np.array_equal(_u32(crc), got) and int(flag.cpu()[0]) == 0              # the same words again


def test_crc32_one_range_per_launch(table):
    """n = 1 for every range: the range's place in the launch does not matter, and neither does what surrounds it in the buffer."""
    buf, off, ids, want = table
    ops, n = HipOps(DEV), len(ids)
    crc = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    pairs = [torch.tensor([int(off[i]), int(off[i + 1])], dtype=torch.int64, device=DEV) for i in range(n)]
    for i in range(n):
        ops.crc32_ranges(buf, pairs[i], crc[i:i + 1], flag)()
    got = _u32(crc)
    assert got.tolist() == want.tolist(), [ids[i] for i in np.flatnonzero(got != want)]
    assert int(flag.cpu()[0]) == 0


def test_crc32_decreasing_pair_is_flagged_and_its_neighbours_are_right():
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, 5000, dtype=np.uint8)
    off = [0, 1000, 3000, 2000, 5000]                                               # all inside the buffer; (3000, 2000) decreases
    buf, offsets = torch.from_numpy(data).to(DEV), torch.tensor(off, dtype=torch.int64, device=DEV)
    crc = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    HipOps(DEV).crc32_ranges(buf, offsets, crc, flag)()
    raw = data.tobytes()
    assert _u32(crc).tolist() == [zlib.crc32(raw[0:1000]), zlib.crc32(raw[1000:3000]), 0, zlib.crc32(raw[2000:5000])]
    assert int(flag.cpu()[0]) == 1


@pytest.mark.parametrize("name,q", JC.CASE_IDS)
def test_encode_block_equals_encode(name, q):
    rgb = JC.rgb(name)
    B, H, W, _ = rgb.shape
    enc = I.JpegEncoder(DEV, B, H, W, quality=q, ops=HipOps(DEV))
    x = torch.from_numpy(rgb).to(DEV)
    files = enc.encode(x)
    assert files == JC.golden(name, q)
    block, off, crcs = enc.encode_block(x)
    assert off[0] == 0 and len(off) == B + 1 and off[B] == len(block) and all(off[b] < off[b + 1] for b in range(B))
    got = [bytes(block[off[b]:off[b + 1]]) for b in range(B)]
    assert got == files, [b for b in range(B) if got[b] != files[b]]
    assert crcs == [zlib.crc32(f) for f in files]
    assert all(f[-2:] == b"\xff\xd9" for f in got)
    block2, off2, crcs2 = enc.encode_block(x)
    assert bytes(block2) == bytes(block) and off2 == off and crcs2 == crcs
    assert enc.encode(x) == files                                                   # encode itself is untouched by the new buffers


def test_encode_block_through_one_encoder_for_several_batch_sizes():
    """max_batch 5 serves 3 images, then 5, then 1: files beyond the batch are not touched, and a shorter batch after a longer one
    gives the same bytes."""
    rgb = JC.rgb("batch")
    want = JC.golden("batch", 95)
    enc = I.JpegEncoder(DEV, 5, 16, 24, ops=HipOps(DEV))
    x = torch.from_numpy(rgb).to(DEV)
    for idx in ([0, 1, 2], [0, 1, 2, 0, 1], [1]):
        block, off, crcs = enc.encode_block(x[idx])
        assert [bytes(block[off[b]:off[b + 1]]) for b in range(len(idx))] == [want[i] for i in idx]
        assert crcs == [zlib.crc32(want[i]) for i in idx]


def _files(root):
    return {p.relative_to(root).as_posix(): p.read_bytes() for p in root.rglob("*") if p.is_file()}


def _entries(path):
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
        return [(i.filename, z.read(i)) for i in z.infolist()]


@pytest.fixture(scope="module")
def photos(tmp_path_factory):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("zip_folder")
    torch.manual_seed(3)
    ck = tmp / "ckpt.pt"
    torch.save({"generator": cut.ResNetGenerator(3, 3, ngf=8, n_blocks=1).state_dict()}, ck)
    src = tmp / "photos"
    (src / "sub").mkdir(parents=True)
    rng = np.random.default_rng(1)
    for name, (h, w) in (("a.png", (70, 64)), ("sub/b.png", (33, 97)), ("sub/c.png", (64, 64)), ("d.png", (80, 61)), ("e.png", (19, 120))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(src / name)
    return tmp, ck, src


def test_folder_archive_equals_the_folder_route(photos):
    """Five photos at img_size 64 in batches of 2 (a ragged last batch)."""
    tmp, ck, src = photos
    G = I.load_generator(str(ck), device="cuda:0", ngf=8, n_blocks=1)
    run = lambda **kw: I.stylize_folder(G, str(src), device="cuda", img_size=64, batch=2, device_io=True, device_jpeg=True, **kw)
    assert run(out_dir=str(tmp / "dir")) == 5
    want = _files(tmp / "dir")
    assert run(zip_path=str(tmp / "a.zip")) == 5
    got = _entries(tmp / "a.zip")
    assert [n for n, _ in got] == ["a.jpg", "d.jpg", "e.jpg", "sub/b.jpg", "sub/c.jpg"] and dict(got) == want
    assert run(zip_path=str(tmp / "b.zip"), out_dir=str(tmp / "both"), io_threads=4) == 5
    assert (tmp / "b.zip").read_bytes() == (tmp / "a.zip").read_bytes() and _files(tmp / "both") == want


def test_command_line_writes_the_archive(photos):
    tmp, ck, src = photos
    cmd = [sys.executable, "-m", "gan_variant_research_amd.generate_folder", "--ckpt", str(ck), "--photos", str(src), "--zip", str(tmp / "cmd.zip"),
           "--device", "cuda", "--size", "64", "--batch", "2", "--ngf", "8", "--n-blocks", "1", "--device-jpeg"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("Done.") and not (tmp / "cmd.zip.part").exists()
    got = _entries(tmp / "cmd.zip")
    G = I.load_generator(str(ck), device="cuda:0", ngf=8, n_blocks=1)
    assert I.stylize_folder(G, str(src), str(tmp / "cmd_dir"), device="cuda", img_size=64, batch=2, device_io=True, device_jpeg=True) == 5
    assert dict(got) == _files(tmp / "cmd_dir") and len(got) == 5
