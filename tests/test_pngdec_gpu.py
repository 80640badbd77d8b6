"""The PNG decoder on the device (csrc/pngdec.hip, dataio.PngDecoder, dataio.DeviceDecoder): pixels equal to the golden pixels Pillow
gave and to live Pillow for every case, with a locator that names the first stage that differs from tests.pngdec_ref (inflate, or what follows it: the
unfiltered rows never leave LDS, so there the locator names the first wrong row, its filter, and placement against arithmetic); reuse over
batches; fallback and flagged files through the parser and the error word (tests/test_pngdec_cpu.py runs the same files through the
sanitizer-built host program first); argument checks; ImageStore, the folder path and the command line against the Pillow paths."""
import ctypes as C
import hashlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gan_variant_research_amd import _lib, cut, dataio, inference as I
from gan_variant_research_amd.runtime import HipOps
from tests import jpegdec_cases as JC, pngdec_cases as PC, pngdec_ref as R
from tests.emulator_pngdec import read_block

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def dec():
    return dataio.PngDecoder(DEV, ops=HipOps(DEV))


@pytest.fixture(scope="module")
def want():
    """Computed once: tests.pngdec_ref's stages of every case."""
    return {n: R.stages(PC.file(n)) for n in PC.CASES}


def _locate(dec, names, want) -> str:
    """Which stage of which file differs from tests.pngdec_ref (the buffers still hold the last decode; `names`: the device's files)."""
    total, n = dec.last_block
    imgs = read_block(dec._host.numpy()[:total], n)
    ws = dec._ws.cpu().numpy()
    for i, (im, name) in enumerate(zip(imgs, names)):
        st = want[name]
        got = ws[im.raw_off:im.raw_off + len(st.raw)]
        ref = np.frombuffer(st.raw, np.uint8)
        if not np.array_equal(got, ref):
            at = int(np.nonzero(got != ref)[0][0])
            return f"file {i} ({name}): the raw bytes after inflate differ, first at byte {at} of {len(st.raw)}: {got[at]} vs {ref[at]}"
        if not np.array_equal(st.pixels, R.pillow_pixels(PC.file(name))):
            return f"file {i} ({name}): tests.pngdec_ref itself differs from live Pillow"
    return "the raw bytes after inflate equal tests.pngdec_ref: the unfiltered rows, the conversion to RGB or the placement differ"


def _locate_rows(px, name, want) -> str:
    """The second half of the locator.  The unfiltered rows exist only in LDS, so unfiltering and conversion cannot be told apart by
    reading a buffer; what can be told: the first row that differs and its filter, and whether that row of the reference's pixels
    (R.to_rgb of the reference's rows) stands somewhere else in the device's image, which is a placement fault and not an arithmetic one."""
    st = want[name]
    bad = np.nonzero((px != st.pixels).any(axis=(1, 2)))[0]
    if bad.size == 0:
        return "pixels equal"
    y = int(bad[0])
    ref_row = R.to_rgb(st.rows[y:y + 1], st.plan.W, st.plan.color, st.plan.depth, st.plan.palette).tobytes()
    at = px.tobytes().find(ref_row)
    where = f"the reference's row stands at byte {at} of the device's image instead of {y * st.plan.W * 3}: placement" if at >= 0 and len(set(ref_row)) > 1 else \
        "the reference's row stands nowhere in the device's image: unfiltering or conversion of this row"
    return f"{name}: rows 0 .. {y - 1} are right; first differing row {y} (filter {st.raw[y * (1 + st.plan.rowbytes)]}); {where}"


def _equals_golden(name, px) -> bool:
    return tuple(px.shape) == PC.shape(name) and hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest() == PC.pixels_sha256(name)


@pytest.mark.parametrize("name", PC.CASES)
def test_device_pixels_equal_pillow(dec, want, name):
    data = PC.file(name)
    before = dict(dec.stats)
    (got,) = dec.decode([data])
    assert got.dtype == torch.uint8 and got.device == DEV and got.is_contiguous()
    px = got.cpu().numpy()
    assert dec.last_errors == {} and dec.stats["device"] == before["device"] + 1, dec.last_errors
    assert _equals_golden(name, px), (_locate(dec, [name], want), _locate_rows(px, name, want))
    assert torch.equal(dec.decode([data])[0], got)                            # no atomics on values: the same bytes every time
    assert np.array_equal(px, R.pillow_pixels(data))                          # live Pillow: PNG decoding has one right answer


def test_many_files_in_one_call_and_the_decoder_reused(dec, want):
    """Files of different formats, sizes and block types in one call; then one decoder over a larger, a smaller and a reordered batch,
    and into a caller's buffer at unaligned offsets."""
    for names in (PC.BATCH, PC.CASES, PC.BATCH[:2], PC.BATCH[::-1]):
        got = dec.decode([PC.file(n) for n in names])
        assert dec.last_errors == {}
        for n, g in zip(names, got):
            assert _equals_golden(n, g.cpu().numpy()), (n, _locate(dec, names, want))
    sizes = [PC.pixels(n).size for n in PC.BATCH]
    offsets = [7 + sum(sizes[:i]) + 3 * i for i in range(len(sizes))]
    out = torch.full((offsets[-1] + sizes[-1] + 5,), 0xAB, dtype=torch.uint8, device=DEV)
    got = dec.decode([PC.file(n) for n in PC.BATCH], out=out, offsets=offsets)
    host, used = out.cpu().numpy(), np.zeros(out.numel(), bool)
    for n, g, o, s in zip(PC.BATCH, got, offsets, sizes):
        assert g.data_ptr() == out.data_ptr() + o and np.array_equal(g.cpu().numpy(), PC.pixels(n)), n
        used[o:o + s] = True
    assert (host[~used] == 0xAB).all()


def _outcome(data):
    try:
        return dataio._decode(io.BytesIO(data)), None
    except OSError as e:
        return None, str(e)


def test_fallback_and_flagged_files_go_to_pillow(dec, tmp_path):
    """The FALLBACK files never reach the device; every FLAGGED file is flagged with the error word tests.pngdec_ref names and gives
    Pillow's pixels or Pillow's OSError; the device is healthy afterwards."""
    before = dict(dec.stats)
    names = [n for n in PC.FALLBACK if _outcome(PC.file(n))[1] is None] + ["grey"]
    got = dec.decode([PC.file(n) for n in names])
    for n, g in zip(names, got):
        assert np.array_equal(g.cpu().numpy(), _outcome(PC.file(n))[0]), n
    assert dec.last_errors == {} and {k: dec.stats[k] - before[k] for k in before} == {"device": 1, "unsupported": len(names) - 1, "flagged": 0}
    for name, bits in PC.FLAGGED.items():
        data = tmp_path / (name + ".png")                                       # a path: Pillow's error names its source
        data.write_bytes(PC.file(name))
        try:
            px, text = dataio._decode(data), None
        except OSError as e:
            px, text = None, str(e)
        before = dict(dec.stats)
        if text is None:
            got = dec.decode([PC.file("grey"), data])
            assert np.array_equal(got[1].cpu().numpy(), px) and np.array_equal(got[0].cpu().numpy(), PC.pixels("grey")), name
            assert {k: dec.stats[k] - before[k] for k in before} == {"device": 1, "unsupported": 0, "flagged": 1}, name
        else:
            with pytest.raises(OSError) as mine:
                dec.decode([PC.file("grey"), data])
            assert str(mine.value) == text, name
        assert set(dec.last_errors) == {1} and (dec.last_errors[1] == bits if bits is not None else dec.last_errors[1] != 0), (name, dec.last_errors)
    (again,) = dec.decode([PC.file("dynamic")])
    assert np.array_equal(again.cpu().numpy(), PC.pixels("dynamic")) and dec.last_errors == {}
    torch.cuda.synchronize()


def test_argument_checks_return_errors_and_launch_nothing(dec):
    lib, ops = _lib.load(), HipOps(DEV)
    dec.decode([PC.file(n) for n in PC.BATCH])
    total, n = dec.last_block
    blk, host, ws = dec._dev, dec._host, dec._ws
    out, err = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    msg = lambda: lib.gan_last_error()
    isz = C.sizeof(_lib.GanPngdecImage)
    bad = host[:total].clone()
    im = _lib.GanPngdecImage.from_buffer_copy(bad[:isz].numpy().tobytes())
    im.stream_len = total
    bad[:isz] = torch.frombuffer(bytearray(bytes(im)), dtype=torch.uint8)
    for entry in (lambda *a: lib.gan_pngdec_inflate(*a, None), lambda *a: lib.gan_pngdec_pixels(*a, p(out), out.numel(), p(err), None)):
        assert entry(None, p(host), total, n, p(ws), ws.numel()) < 0 and b"null" in msg()
        assert entry(p(blk), p(host), total, 0, p(ws), ws.numel()) < 0 and b"65535" in msg()
        assert entry(p(blk), p(host), total, n, p(ws), 256) < 0 and b"workspace" in msg()
        assert entry(p(blk), p(host), total, n, C.c_void_p(ws.data_ptr() + 4), ws.numel() - 4) < 0 and b"aligned" in msg()
        assert entry(p(blk), p(host), 64, n, p(ws), ws.numel()) < 0 and b"descriptors" in msg()
        assert entry(p(blk), p(bad), total, n, p(ws), ws.numel()) < 0 and b"stream" in msg()
    assert lib.gan_pngdec_pixels(p(blk), p(host), total, n, p(ws), ws.numel(), p(out), 16, p(err), None) < 0 and b"output" in msg()
    assert lib.gan_pngdec_pixels(p(blk), p(host), total, n, p(ws), ws.numel(), None, out.numel(), p(err), None) < 0 and b"null" in msg()
    with pytest.raises(_lib.GanError, match="workspace"):
        ops.pngdec_inflate(blk, host, total, n, ws[:256])
    with pytest.raises(_lib.GanError):
        dec.decode([PC.file("grey")], out=torch.zeros(4, dtype=torch.uint8, device=DEV), offsets=[0])       # too small for 5 x 7 x 3
    with pytest.raises(_lib.GanError):
        dec.decode([PC.file("grey")], out=torch.zeros(1 << 16, dtype=torch.uint8), offsets=[0])             # not on the device
    torch.cuda.synchronize()                                                 # nothing above launched anything that could fault


def _mixed_folder(root):
    """PNG, baseline JPEG, progressive JPEG, PNGs from FALLBACK and a flagged PNG, suffixes that do not all tell the truth."""
    root.mkdir(parents=True, exist_ok=True)
    items = [("a.png", PC.file("rgba"), PC.pixels("rgba")), ("b.jpg", JC.file("gray"), JC.pixels("gray")), ("c.jpg", JC.file("progressive"), JC.pixels("progressive")),
             ("d.png", PC.file("rgb16"), PC.pixels("rgb16")), ("e.png", PC.file("pal2.w5"), PC.pixels("pal2.w5")), ("f.png", JC.file("rst"), JC.pixels("rst")),
             ("g.jpg", PC.file("filter.all"), PC.pixels("filter.all")), ("h.png", PC.file("surplus"), PC.pixels("surplus")), ("i.png", PC.file("interlaced"), PC.pixels("interlaced")),
             ("j.png", PC.file("dynamic"), PC.pixels("dynamic")), ("k.png", PC.file("mixed"), PC.pixels("mixed"))]
    paths = []
    for name, data, _ in items:
        paths.append(root / name)
        paths[-1].write_bytes(data)
    return paths, [px for _, _, px in items]


def test_device_decoder_takes_both_formats_in_one_call(tmp_path):
    paths, want = _mixed_folder(tmp_path / "mixed")
    both = dataio.DeviceDecoder(DEV, ops=HipOps(DEV))
    got = both.decode(paths)
    for g, w in zip(got, want):
        assert g.device == DEV and np.array_equal(g.cpu().numpy(), w)
    assert got[0].untyped_storage().data_ptr() == got[-1].untyped_storage().data_ptr()
    assert both.png.stats == {"device": 5, "unsupported": 2, "flagged": 1} and both.jpeg.stats == {"device": 2, "unsupported": 1, "flagged": 0}
    assert both.stats == {"device": 7, "unsupported": 3, "flagged": 1} and both.last_errors == {7: R.MORE}
    torch.cuda.synchronize()


@pytest.mark.parametrize("both", [False, True], ids=["png", "png+jpeg"])
@pytest.mark.parametrize("budget", [None, 0], ids=["resident", "streaming"])
def test_image_store_holds_identical_bytes(tmp_path, monkeypatch, budget, both):
    paths, want = _mixed_folder(tmp_path / "imgs")
    monkeypatch.setattr(dataio, "DECODE_CHUNK", 4)
    plain = dataio.ImageStore(paths, DEV, budget_bytes=budget, workers=4)
    store = dataio.ImageStore(paths, DEV, budget_bytes=budget, workers=4, device_png=True, device_decode=both)
    assert store.resident == plain.resident == (budget is None) and store.offsets == plain.offsets and store.sizes == plain.sizes
    for i, w in enumerate(want):
        assert store[i].device == DEV and torch.equal(store[i], plain[i]) and np.array_equal(store[i].cpu().numpy(), w), i
    order = [7, 0, 3, 3, 10]
    for a, b in zip(store.fetch(order), plain.fetch(order)):
        assert torch.equal(a, b)
    if budget is None:
        assert store._decoder.stats == ({"device": 7, "unsupported": 3, "flagged": 1} if both else {"device": 5, "unsupported": 5, "flagged": 1})
    pipe = dataio.InputPipeline(16, DEV, max_batch=4)                          # the pipeline reads what the decoder wrote, where it wrote it
    jobs = [dataio.eval_job(*store.sizes[i], 16) for i in (0, 4, 10)]
    assert torch.equal(pipe.run([store[i] for i in (0, 4, 10)], jobs), pipe.run([plain[i] for i in (0, 4, 10)], jobs))
    store.close(), plain.close()
    torch.cuda.synchronize()


def _files(root):
    return {p.relative_to(root).as_posix(): p.read_bytes() for p in root.rglob("*") if p.is_file()}


def test_folder_and_command_write_the_same_files(tmp_path):
    """Mixed-size PNGs of four formats, a baseline and a progressive JPEG and a 16-bit PNG: every mode writes the files the Pillow decode
    writes, in process and through the command line."""
    from PIL import Image
    torch.manual_seed(3)
    ck = tmp_path / "ckpt.pt"
    torch.save({"generator": cut.ResNetGenerator(3, 3, ngf=8, n_blocks=1).state_dict()}, ck)
    G = I.load_generator(str(ck), device="cuda:0", ngf=8, n_blocks=1)
    photos = tmp_path / "photos"
    (photos / "sub").mkdir(parents=True)
    rng = np.random.default_rng(1)
    for name, shape in (("a.png", (20, 24, 3)), ("sub/b.png", (33, 17, 4)), ("sub/c.png", (24, 24)), ("d.png", (40, 31, 3))):
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8)).save(photos / name)
    Image.fromarray(rng.integers(0, 256, (9, 50, 3), dtype=np.uint8)).quantize(16).save(photos / "e.png")
    Image.fromarray(rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)).save(photos / "f.jpg", quality=90)
    Image.fromarray(rng.integers(0, 256, (16, 30, 3), dtype=np.uint8)).save(photos / "sub" / "g.jpg", progressive=True)
    (photos / "h.png").write_bytes(PC.file("rgb16"))
    run = lambda out, **kw: I.stylize_folder(G, str(photos), str(tmp_path / out), device="cuda", img_size=24, batch=2, device_io=True, **kw)
    assert run("pil") == 8
    want = _files(tmp_path / "pil")
    assert len(want) == 8 and len(set(want.values())) == 8
    assert run("png", device_png=True) == 8 and _files(tmp_path / "png") == want
    assert G._png_dec.stats == {"device": 5, "unsupported": 3, "flagged": 0}
    assert run("both", device_png=True, device_decode=True) == 8 and _files(tmp_path / "both") == want
    assert G._device_dec.stats == {"device": 6, "unsupported": 2, "flagged": 0}
    assert run("png3", device_png=True, decode_chunk=3, device_jpeg=True, io_threads=4) == 8 and _files(tmp_path / "png3") == want
    cmd = [sys.executable, "-m", "gan_variant_research_amd.generate_folder", "--ckpt", str(ck), "--photos", str(photos), "--out", str(tmp_path / "cmd"),
           "--device", "cuda", "--size", "24", "--batch", "2", "--ngf", "8", "--n-blocks", "1", "--device-png", "--device-decode", "--decode-chunk", "4", "--device-jpeg"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device=cuda" in out.stdout and out.stdout.rstrip().endswith("Done.")
    assert _files(tmp_path / "cmd") == want
    torch.cuda.synchronize()
