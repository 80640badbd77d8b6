"""The JPEG decoder on the device (csrc/jpegdec.hip, dataio.JpegDecoder): pixels equal to the golden pixels Pillow gave and to live
Pillow for every case, with a locator that names the first stage that differs from tests.jpegdec_ref; reuse over batches; corrupt, crafted
and truncated files through the error word (tests/test_jpegdec_cpu.py runs the same files through the sanitizer-built host program);
argument checks; ImageStore, the folder path and the command line with device decoding against the Pillow paths."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gan_variant_research_amd import _lib, cut, dataio, inference as I
from gan_variant_research_amd.runtime import HipOps
from tests import jpegdec_cases as DC, jpegdec_ref as R
from tests.emulator_jpegdec import comp_shapes, read_block

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def dec():
    return dataio.JpegDecoder(DEV, ops=HipOps(DEV))


def _locate(dec, files) -> str:
    """Which stage of which image differs from tests.jpegdec_ref (the buffers still hold the last decode; `files`: the device's images)."""
    total, n, nseg = dec.last_block
    imgs, _, _ = read_block(dec._host.numpy()[:total], n, nseg)
    ws = dec._ws.cpu().numpy()
    for i, (im, data) in enumerate(zip(imgs, files)):
        st = R.stages(data)
        at = im.coef_off
        for c, ((bh, bw), want) in enumerate(zip(comp_shapes(im), st.coefs)):
            got = ws[at:at + bh * bw * 128].view(np.int16).reshape(bh, bw, 64)
            if not np.array_equal(got, want):
                by, bx, k = (int(v[0]) for v in np.nonzero(got != want))
                return f"image {i}: coefficients differ (tables / entropy decode), first at component {c} block ({by}, {bx}) index {k}: {got[by, bx, k]} vs {want[by, bx, k]}"
            at += bh * bw * 128
        at = im.plane_off
        for c, ((bh, bw), want) in enumerate(zip(comp_shapes(im), st.planes)):
            got = ws[at:at + bh * bw * 64].reshape(bh * 8, bw * 8)
            if not np.array_equal(got, want):
                y, x = (int(v[0]) for v in np.nonzero(got != want))
                return f"image {i}: coefficients equal, planes differ (dequantisation / IDCT), first at component {c} ({y}, {x}): {got[y, x]} vs {want[y, x]}"
            at += bh * bw * 64
        if not np.array_equal(st.pixels, R.pillow_pixels(data)):
            return f"image {i}: tests.jpegdec_ref itself differs from live Pillow"
    return "coefficients and planes equal tests.jpegdec_ref: the pixels differ (upsampling / colour conversion / placement)"


def _equals_golden(name, px) -> bool:
    return tuple(px.shape) == DC.CASES[name][:2] + (3,) and hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest() == DC.pixels_sha256(name)


@pytest.mark.parametrize("name", list(DC.CASES))
def test_device_pixels_equal_pillow(dec, name):
    from PIL import features
    data = DC.file(name)
    before = dict(dec.stats)
    (got,) = dec.decode([data])
    assert got.dtype == torch.uint8 and got.device == DEV and got.is_contiguous()
    px = got.cpu().numpy()
    assert dec.last_errors == {} and dec.stats["device"] == before["device"] + 1, dec.last_errors
    assert _equals_golden(name, px), _locate(dec, [data])
    assert torch.equal(dec.decode([data])[0], got)                            # no atomics on values: the same bytes every time
    live = R.pillow_pixels(data)
    if not _equals_golden(name, live):
        pytest.skip(f"device pixels equal the golden pixels; live Pillow (libjpeg {features.version('jpg')}) differs from them, comparison with it skipped")
    assert np.array_equal(px, live)


def test_many_files_in_one_call_and_the_decoder_reused(dec):
    """Six files of different sizes, samplings and tables in one call; then one decoder over a larger, a smaller and a reordered batch,
    and into a caller's buffer at unaligned offsets."""
    everything = DC.PIXEL_CASES + ["long"]
    for names in (DC.BATCH, everything, DC.BATCH[:2], DC.BATCH[::-1]):
        files = [DC.file(n) for n in names]
        got = dec.decode(files)
        assert dec.last_errors == {}
        for i, (n, g) in enumerate(zip(names, got)):
            assert _equals_golden(n, g.cpu().numpy()), (n, _locate(dec, files))
    sizes = [DC.pixels(n).size for n in DC.BATCH]
    offsets = [7 + sum(sizes[:i]) + 3 * i for i in range(len(sizes))]
    out = torch.full((offsets[-1] + sizes[-1] + 5,), 0xAB, dtype=torch.uint8, device=DEV)
    got = dec.decode([DC.file(n) for n in DC.BATCH], out=out, offsets=offsets)
    host, used = out.cpu().numpy(), np.zeros(out.numel(), bool)
    for n, g, o, s in zip(DC.BATCH, got, offsets, sizes):
        assert g.data_ptr() == out.data_ptr() + o and np.array_equal(g.cpu().numpy(), DC.pixels(n)), n
        used[o:o + s] = True
    assert (host[~used] == 0xAB).all()


def test_irregular_files_go_to_pillow_through_the_error_word(dec, tmp_path):
    """`corrupt` (three scan bytes overwritten), `crafted` (coefficients beyond the range in which libjpeg's C and SIMD code agree) and
    the other fallback files give Pillow's pixels; `truncated` raises what the Pillow path raises; the device is healthy afterwards."""
    before = dict(dec.stats)
    names = DC.FALLBACK + ["gray"]
    got = dec.decode([DC.file(n) for n in names])
    for n, g in zip(names, got):
        assert np.array_equal(g.cpu().numpy(), DC.pixels(n)), n
    assert dec.last_errors[names.index("crafted")] == 128
    assert dec.last_errors[names.index("corrupt")] not in (0, 128) and len(dec.last_errors) == 2
    assert {k: dec.stats[k] - before[k] for k in before} == {"device": 1, "unsupported": 5, "flagged": 2}
    p = tmp_path / "cut.jpg"
    p.write_bytes(DC.truncated())
    with pytest.raises(OSError) as plain:
        dataio._decode(p)
    with pytest.raises(OSError) as mine:
        dec.decode([DC.file("gray"), p])
    assert str(mine.value) == str(plain.value)
    (again,) = dec.decode([DC.file("wide")])
    assert np.array_equal(again.cpu().numpy(), DC.pixels("wide"))
    torch.cuda.synchronize()


def test_argument_checks_return_errors_and_launch_nothing(dec):
    lib, ops = _lib.load(), HipOps(DEV)
    dec.decode([DC.file(n) for n in DC.BATCH])
    total, n, nseg = dec.last_block
    blk, host, ws = dec._dev, dec._host, dec._ws
    out, err = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    msg = lambda: lib.gan_last_error()
    for entry in (lib.gan_jpegdec_tables, lib.gan_jpegdec_entropy, lib.gan_jpegdec_idct):
        assert entry(None, p(host), total, n, nseg, p(ws), ws.numel(), None) < 0 and b"null" in msg()
        assert entry(p(blk), p(host), total, 0, nseg, p(ws), ws.numel(), None) < 0 and b"65535" in msg()
        assert entry(p(blk), p(host), total, n, nseg, p(ws), 4096, None) < 0 and b"workspace" in msg()
        assert entry(p(blk), p(host), total, n, nseg, C.c_void_p(ws.data_ptr() + 4), ws.numel() - 4, None) < 0 and b"aligned" in msg()
        assert entry(p(blk), p(host), 64, n, nseg, p(ws), ws.numel(), None) < 0 and b"descriptors" in msg()
    assert lib.gan_jpegdec_pixels(p(blk), p(host), total, n, nseg, p(ws), ws.numel(), p(out), 16, p(err), None) < 0 and b"output" in msg()
    assert lib.gan_jpegdec_pixels(p(blk), p(host), total, n, nseg, p(ws), ws.numel(), None, out.numel(), p(err), None) < 0 and b"null" in msg()
    with pytest.raises(_lib.GanError, match="workspace"):
        ops.jpegdec_entropy(blk, host, total, n, nseg, ws[:4096])
    with pytest.raises(_lib.GanError):
        dec.decode([DC.file("gray")], out=torch.zeros(4, dtype=torch.uint8, device=DEV), offsets=[0])       # too small for 24 x 40 x 3
    with pytest.raises(_lib.GanError):
        dec.decode([DC.file("gray")], out=torch.zeros(1 << 16, dtype=torch.uint8), offsets=[0])             # not on the device
    torch.cuda.synchronize()                                                 # nothing above launched anything that could fault


def _write_folder(root, names):
    root.mkdir(parents=True, exist_ok=True)
    paths = []
    for n in names:
        paths.append(root / (n.replace(".", "_") + (".png" if n == "png" else ".jpg")))
        paths[-1].write_bytes(DC.file(n))
    return paths


@pytest.mark.parametrize("budget", [None, 0], ids=["resident", "streaming"])
def test_image_store_holds_identical_bytes(tmp_path, monkeypatch, budget):
    names = DC.BATCH + ["png", "progressive", "corrupt", "crafted", "wide"]
    paths = _write_folder(tmp_path / "imgs", names)
    monkeypatch.setattr(dataio, "DECODE_CHUNK", 4)
    plain = dataio.ImageStore(paths, DEV, budget_bytes=budget, workers=4)
    store = dataio.ImageStore(paths, DEV, budget_bytes=budget, workers=4, device_decode=True)
    assert store.resident == plain.resident == (budget is None) and store.offsets == plain.offsets and store.sizes == plain.sizes
    for i, n in enumerate(names):
        assert store[i].device == DEV and torch.equal(store[i], plain[i]) and np.array_equal(store[i].cpu().numpy(), DC.pixels(n)), n
    order = [7, 0, 3, 3, 9]
    for a, b in zip(store.fetch(order), plain.fetch(order)):
        assert torch.equal(a, b)
    st = store._decoder.stats
    assert st["device"] > 0 and st["unsupported"] > 0 and st["flagged"] > 0
    if budget is None:
        assert st == {"device": 7, "unsupported": 2, "flagged": 2}
    pipe = dataio.InputPipeline(16, DEV, max_batch=4)                          # the pipeline reads what the decoder wrote, where it wrote it
    jobs = [dataio.eval_job(*store.sizes[i], 16) for i in (0, 2, 10)]
    assert torch.equal(pipe.run([store[i] for i in (0, 2, 10)], jobs), pipe.run([plain[i] for i in (0, 2, 10)], jobs))
    store.close(), plain.close()
    torch.cuda.synchronize()


def _files(root):
    return {p.relative_to(root).as_posix(): p.read_bytes() for p in root.rglob("*") if p.is_file()}


def test_folder_and_command_write_the_same_files(tmp_path):
    """The five mixed-size photos of the encoder's folder test saved as JPEGs, plus a PNG and a progressive JPEG: every mode writes the
    files the Pillow decode writes, in process and through the command line."""
    from PIL import Image
    torch.manual_seed(3)
    ck = tmp_path / "ckpt.pt"
    torch.save({"generator": cut.ResNetGenerator(3, 3, ngf=8, n_blocks=1).state_dict()}, ck)
    G = I.load_generator(str(ck), device="cuda:0", ngf=8, n_blocks=1)
    photos = tmp_path / "photos"
    (photos / "sub").mkdir(parents=True)
    rng = np.random.default_rng(1)
    for name, (h, w) in (("a.jpg", (20, 24)), ("sub/b.jpg", (33, 17)), ("sub/c.jpg", (24, 24)), ("d.jpg", (40, 31)), ("e.jpg", (9, 50))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(photos / name, quality=90)
    Image.fromarray(rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)).save(photos / "f.png")
    Image.fromarray(rng.integers(0, 256, (16, 30, 3), dtype=np.uint8)).save(photos / "sub" / "g.jpg", progressive=True)
    run = lambda out, **kw: I.stylize_folder(G, str(photos), str(tmp_path / out), device="cuda", img_size=24, batch=2, device_io=True, **kw)
    assert run("pil") == 7
    want = _files(tmp_path / "pil")
    assert len(want) == 7 and len(set(want.values())) == 7
    assert run("dec", device_decode=True) == 7 and _files(tmp_path / "dec") == want
    assert G._jpeg_dec.stats == {"device": 5, "unsupported": 2, "flagged": 0}
    assert run("dec3", device_decode=True, decode_chunk=3, device_jpeg=True, io_threads=4) == 7 and _files(tmp_path / "dec3") == want
    cmd = [sys.executable, "-m", "gan_variant_research_amd.generate_folder", "--ckpt", str(ck), "--photos", str(photos), "--out", str(tmp_path / "cmd"),
           "--device", "cuda", "--size", "24", "--batch", "2", "--ngf", "8", "--n-blocks", "1", "--device-decode", "--decode-chunk", "4", "--device-jpeg"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device=cuda" in out.stdout and out.stdout.rstrip().endswith("Done.")
    assert _files(tmp_path / "cmd") == want
    torch.cuda.synchronize()
