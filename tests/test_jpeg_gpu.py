"""The JPEG encoder on the device (csrc/jpeg.hip, inference.JpegEncoder): complete files byte-identical to the golden files Pillow wrote
and to live Pillow, the table kernel on histograms that need the length limiter, determinism, argument checks, and the folder path /
command line with --device-jpeg against the PIL path."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gan_variant_research_amd import _lib, basic, cut, inference as I
from gan_variant_research_amd.runtime import HipOps
from tests import jpeg_cases as JC, jpeg_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _locate(enc, rgb, q, files):
    """Which stage of which image differs from tests.jpeg_ref (the buffers still hold the last encode)."""
    hist, dht, codes = enc.hist.cpu().numpy(), enc.dht.cpu().numpy(), enc.codes.cpu().numpy()
    for b, im in enumerate(rgb):
        st = R.stages(im, q)
        if not np.array_equal(hist[b], st.hist):
            t, s = (int(v[0]) for v in np.nonzero(hist[b] != st.hist))
            return f"image {b}: histograms differ (colour / DCT / quantisation / symbols), first at table {t} symbol {s:#x}: {hist[b][t, s]} vs {st.hist[t, s]}"
        for t, (bits, vals) in enumerate(st.tables):
            code, size = R.canonical_codes(bits, vals)
            if dht[b, t, :16].tolist() != bits[1:].tolist() or dht[b, t, 16:16 + len(vals)].tolist() != vals.tolist():
                return f"image {b}: table {t} differs: counts {dht[b, t, :16].tolist()} vs {bits[1:].tolist()}"
            if not np.array_equal(codes[b, t], (size << 16) | code):
                return f"image {b}: codes of table {t} differ"
        if files[b] != st.file:
            got, want = R.split_file(files[b]).scan, st.scan
            i = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
            return f"image {b}: tables equal, scan differs at byte {i} of {len(want)} (got {len(got)} bytes)"
    return "no stage differs from tests.jpeg_ref"


@pytest.mark.parametrize("name,q", JC.CASE_IDS)
def test_device_files_equal_pillow(name, q):
    from PIL import features
    rgb, golden = JC.rgb(name), JC.golden(name, q)
    B, H, W, _ = rgb.shape
    enc = I.JpegEncoder(DEV, B, H, W, quality=q, ops=HipOps(DEV))
    x = torch.from_numpy(rgb).to(DEV)
    files = enc.encode(x)
    assert isinstance(files, list) and all(isinstance(f, bytes) for f in files)
    assert files == golden, _locate(enc, rgb, q, files)
    assert enc.encode(x) == files                                           # integer atomics only: the same bytes every time
    live = [R.pillow_bytes(im, q) for im in rgb]
    if live != golden:
        pytest.skip(f"device files equal the golden files; live Pillow (libjpeg {features.version('jpg')}) differs from them, comparison with it skipped")
    assert files == live


def test_encoder_larger_than_the_batch_and_reused():
    """max_batch above B (images beyond B are not touched), then a longer and a shorter batch through the same buffers."""
    rgb = JC.rgb("batch")
    enc = I.JpegEncoder(DEV, 5, 16, 24, ops=HipOps(DEV))
    x = torch.from_numpy(rgb).to(DEV)
    want = JC.golden("batch", 95)
    assert enc.encode(x) == want
    assert enc.encode(x[[2, 0]]) == [want[2], want[0]]
    assert enc.encode(torch.cat([x, x[:2]])) == want + want[:2]
    assert enc.encode(x[1:2]) == want[1:2]


def test_table_kernel_limits_lengths_like_libjpeg():
    ops = HipOps(DEV)
    h = np.concatenate([JC.fibonacci_hists(), np.stack([R.stages(im, 95).hist for im in JC.rgb("ragged")]).reshape(-1, 256)])
    n = len(h)
    hist = torch.from_numpy(h.astype(np.int32)).to(DEV)
    dht = torch.full((n, 272), 0xAB, dtype=torch.uint8, device=DEV)
    codes = torch.full((n, 256), -1, dtype=torch.int32, device=DEV)
    ops.jpeg_tables(hist, n, dht, codes)()
    dht, codes = dht.cpu().numpy(), codes.cpu().numpy()
    assert max(R.merged_code_sizes(h[1])) > 16
    for t in range(n):
        bits, vals = R.optimal_table(h[t])
        code, size = R.canonical_codes(bits, vals)
        assert dht[t, :16].tolist() == bits[1:].tolist(), t
        assert dht[t, 16:16 + len(vals)].tolist() == vals.tolist() and not dht[t, 16 + len(vals):].any(), t
        assert np.array_equal(codes[t], (size << 16) | code), t


def test_argument_checks_return_errors():
    ops, lib = HipOps(DEV), _lib.load()
    ws_b, out_b = ops.jpeg_bounds(2, 9, 33)
    new = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device=DEV)
    rgb, ws, out, hist, codes, off = new((2, 9, 33, 3)), new(ws_b), new(out_b), new(2048, torch.int32), new(2048, torch.int32), new(3, torch.int64)
    p = lambda t: C.c_void_p(t.data_ptr())
    err = lambda: lib.gan_last_error()
    assert lib.gan_jpeg_blocks(p(rgb), 2, 9, 33, 0, p(ws), ws_b, p(hist), None) < 0 and b"quality" in err()
    assert lib.gan_jpeg_blocks(p(rgb), 2, 9, 33, 95, p(ws), ws_b - 1, p(hist), None) < 0 and b"workspace" in err()
    assert lib.gan_jpeg_blocks(None, 2, 9, 33, 95, p(ws), ws_b, p(hist), None) < 0 and b"null" in err()
    assert lib.gan_jpeg_blocks(p(rgb), 2, 0, 33, 95, p(ws), ws_b, p(hist), None) < 0 and b"65535" in err()
    assert lib.gan_jpeg_scan(p(ws), ws_b, 2, 9, 33, p(codes), p(out), out_b - 1, p(off), None) < 0 and b"output" in err()
    assert lib.gan_jpeg_scan(p(ws), ws_b, 2, 9, 33, p(codes), None, out_b, p(off), None) < 0 and b"null" in err()
    assert lib.gan_jpeg_tables(p(hist), 0, p(out), p(codes), None) < 0 and b"tables" in err()
    with pytest.raises(_lib.GanError, match="32-bit"):
        ops.jpeg_bounds(1, 16384, 16384)
    with pytest.raises(ValueError):
        I.JpegEncoder(DEV, 2, 9, 33, quality=101)
    enc = I.JpegEncoder(DEV, 2, 9, 33)
    for bad in (new((3, 9, 33, 3)), new((1, 9, 32, 3)), new((1, 9, 33, 3), torch.int32), torch.zeros(1, 9, 33, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            enc.encode(bad)
    torch.cuda.synchronize()                                                 # nothing above launched anything that could fault


def _files(root):
    return {p.relative_to(root).as_posix(): p.read_bytes() for p in root.rglob("*") if p.is_file()}


def test_folder_and_command_write_the_files_pil_writes(tmp_path):
    """Five photos of mixed sizes through a tiny generator: PIL's encode against the device's, serial and pooled I/O, the CUT and the
    CycleGAN generator, in process and through the command line."""
    from PIL import Image
    torch.manual_seed(3)
    ck, ckb = tmp_path / "ckpt.pt", tmp_path / "ckpt_basic.pt"
    torch.save({"generator": cut.ResNetGenerator(3, 3, ngf=8, n_blocks=1).state_dict()}, ck)
    torch.save({"G_A2B": basic.ResnetGenerator(3, 3, 8, 6).state_dict(), "G_B2A": basic.ResnetGenerator(3, 3, 8, 6).state_dict()}, ckb)
    G = I.load_generator(str(ck), device="cuda:0", ngf=8, n_blocks=1)
    photos = tmp_path / "photos"
    (photos / "sub").mkdir(parents=True)
    rng = np.random.default_rng(1)
    for name, (h, w) in (("a.png", (20, 24)), ("sub/b.png", (33, 17)), ("sub/c.png", (24, 24)), ("d.png", (40, 31)), ("e.png", (9, 50))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(photos / name)
    run = lambda G, out, **kw: I.stylize_folder(G, str(photos), str(tmp_path / out), device="cuda", img_size=24, batch=2, device_io=True, **kw)
    assert run(G, "pil") == 5
    want = _files(tmp_path / "pil")
    assert len(want) == 5 and len(set(want.values())) == 5
    assert run(G, "jpeg", device_jpeg=True) == 5 and _files(tmp_path / "jpeg") == want
    assert run(G, "jpeg4", device_jpeg=True, io_threads=4) == 5 and _files(tmp_path / "jpeg4") == want
    assert run(G, "pil4", io_threads=4) == 5 and _files(tmp_path / "pil4") == want
    Gb = I.load_generator(str(ckb), device="cuda:0", which="G_B2A")
    assert run(Gb, "bpil") == 5 and run(Gb, "bjpeg", device_jpeg=True) == 5
    assert _files(tmp_path / "bjpeg") == _files(tmp_path / "bpil") != want
    cmd = [sys.executable, "-m", "gan_variant_research_amd.generate_folder", "--ckpt", str(ck), "--photos", str(photos), "--out", str(tmp_path / "cmd"),
           "--device", "cuda", "--size", "24", "--batch", "2", "--ngf", "8", "--n-blocks", "1", "--device-jpeg", "--io-threads", "4"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device=cuda" in out.stdout and out.stdout.rstrip().endswith("Done.")
    assert _files(tmp_path / "cmd") == want
