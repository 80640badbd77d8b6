"""The JPEG encoder off the GPU: tests.jpeg_ref (the statement csrc/jpeg.hip is held to) against Pillow itself, the table builder on
histograms Pillow cannot easily be driven to, the host side of `inference.JpegEncoder`, `stylize_folder(device_jpeg=True)` and the command
line on the emulator, and the argument checks of the C entry points (they fail in validation: no launch)."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from gan_variant_research_amd import _lib, autograd as AG, cut, dataio, inference as I
from tests import jpeg_cases as JC, jpeg_ref as R
from tests.emulator_jpeg import EmuInputPipeline, JpegEmuOps


@pytest.fixture(scope="module")
def staged():
    """jpeg_ref's stages of every case image, computed once."""
    return {(name, q): [R.stages(im, q) for im in JC.rgb(name)] for name, q in JC.CASE_IDS}


@pytest.mark.parametrize("name,q", JC.CASE_IDS)
def test_ref_equals_golden_and_live_pillow(staged, name, q):
    assert JC.rgb(name).shape == JC.CASES[name][0] + (3,)
    for st, im, want in zip(staged[(name, q)], JC.rgb(name), JC.golden(name, q)):
        assert st.file == want
        assert R.pillow_bytes(im, q) == want, "live Pillow differs from the golden file"


def test_cases_hit_what_they_are_for(staged):
    pads = {st.nbits % 8 == 0 for sts in staged.values() for st in sts}
    assert pads == {True, False}                                  # a scan with and a scan without padding bits
    assert staged[("mcu", 95)][0].nbits % 8 == 0
    for q in (30, 1):
        tabs = R.split_file(JC.golden("runs", q)[0]).tables
        assert any(cls_id >> 4 == 1 and 0xF0 in vals for cls_id, _, vals in tabs), q
    assert b"\xff\x00" in R.split_file(JC.golden("stuffing", 95)[0]).scan
    st = staged[("const", 95)][0]
    assert all(len(v) <= 2 for _, v in st.tables) and set(st.hist[1].nonzero()[0]) == {0}      # EOB only
    assert [len(R.split_file(f).scan) for f in JC.golden("batch", 95)] == sorted((len(R.split_file(f).scan) for f in JC.golden("batch", 95)), reverse=True)


def _huffman_depth(freq) -> int:
    """Longest code libjpeg's merges give before limiting (the pseudo-symbol included)."""
    return max(R.merged_code_sizes(freq))


def _check_table(freq, bits, vals):
    used = np.flatnonzero(freq)
    assert bits[0] == 0 and int(bits.sum()) == len(vals) == len(used) and sorted(vals.tolist()) == used.tolist()
    assert sum(int(bits[L]) << (16 - L) for L in range(1, 17)) + 1 <= 1 << 16          # Kraft, the all-ones code of the last length reserved
    code, size = R.canonical_codes(bits, vals)
    assert size.max() <= 16 and all((size[s] > 0) == (freq[s] > 0) for s in range(256))
    order = [(int(size[v]), int(v)) for v in vals]
    assert [s for s, _ in order] == sorted(s for s, _ in order)                       # lengths never decrease along huffval
    return size


def test_table_builder_limits_fibonacci_lengths():
    hists = JC.fibonacci_hists()
    for h in hists:
        assert _huffman_depth(h) > 16
        bits, vals = R.optimal_table(h)
        size = _check_table(h, bits, vals)
        # the reserved code included, a limited table is complete: Kraft sum exactly 1
        assert sum(int(bits[L]) << (16 - L) for L in range(1, 17)) + (1 << (16 - int(size.max()))) == 1 << 16
        # within one length the limiter keeps libjpeg's order: symbols by (length before limiting, value), so rarer symbols never get
        # shorter codes than more frequent ones
        f = h[vals]
        assert all(size[a] <= size[b] for a, b in zip(vals[:-1], vals[1:]))
        assert all(f[i] >= f[j] for i in range(len(vals)) for j in range(i + 1, len(vals)) if size[vals[i]] < size[vals[j]])
    # the unlimited case keeps Huffman's lengths: cost equals the optimum
    h = np.zeros(256, np.int64)
    h[[0, 3, 9, 200]] = [50, 20, 20, 5]
    bits, vals = R.optimal_table(h)
    size = _check_table(h, bits, vals)
    assert [int(size[s]) for s in (0, 3, 9, 200)] == [1, 2, 3, 4] and vals.tolist() == [0, 3, 9, 200]
    # ties go to the larger index: of two equal frequencies the larger symbol is merged first and sits deeper
    h = np.zeros(256, np.int64)
    h[[5, 6, 7]] = [1, 1, 4]
    size = R.canonical_codes(*R.optimal_table(h))[1]
    assert [int(size[s]) for s in (5, 6, 7)] == [2, 3, 1]


def test_stream_under_a_limited_table_decodes_to_the_same_pixels():
    """A real image's symbols coded with tables built from Fibonacci-like counts on those same symbols (lengths above 16 before limiting):
    Pillow must decode that file to exactly the pixels of the file coded with the image's own tables -- same coefficients."""
    from PIL import Image
    im = JC.rgb("stuffing")[0]
    own = R.stages(im, 95)
    fib = JC.fib_like(30)
    over = np.zeros((4, 256), np.int64)
    for t in range(4):
        used = np.flatnonzero(own.hist[t])
        over[t, used] = 1
        top = used[np.argsort(own.hist[t][used])][-30:]
        over[t, top] = fib[:len(top)]
    assert _huffman_depth(over[1]) > 16 and _huffman_depth(over[3]) > 16
    lim = R.stages(im, 95, hist_override=over)
    assert lim.file != own.file and max(int(R.canonical_codes(b, v)[1].max()) for b, v in lim.tables) == 16
    for b, v in lim.tables:
        _check_table(np.isin(np.arange(256), v).astype(int), b, v)
    a, b = (np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in (own.file, lim.file))
    assert np.array_equal(a, b)


def _sof(data: bytes):
    i = data.index(b"\xff\xc0")
    return int.from_bytes(data[i + 5:i + 7], "big"), int.from_bytes(data[i + 7:i + 9], "big"), data[i + 9:i + 19]


@pytest.mark.parametrize("name,q", [("pixel", 95), ("ragged", 95), ("batch", 95), ("checker", 100), ("runs", 1)])
def test_encoder_host_side_on_the_emulator(name, q):
    """JpegEncoder's header assembly, table download and stream slicing, with the stages emulated: complete files equal Pillow's."""
    (B, H, W), _ = JC.CASES[name]
    enc = I.JpegEncoder("cpu", B + 1, H, W, quality=q, ops=JpegEmuOps())
    files = enc.encode(torch.from_numpy(JC.rgb(name)))
    assert files == JC.golden(name, q)
    for f in files:
        assert _sof(f) == (H, W, bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))      # the true size, not the padded one
        assert f[:20] == b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
        assert [t[0] for t in R.split_file(f).tables] == [0x00, 0x10, 0x01, 0x11]
        assert f[f.index(b"\xff\xda"):][:14] == b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert enc.encode(torch.from_numpy(JC.rgb(name))[:1]) == files[:1]                 # a smaller batch through the same encoder
    with pytest.raises(ValueError):
        enc.encode(torch.zeros(1, H + 1, W, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        enc.encode(torch.zeros(B + 2, H, W, 3, dtype=torch.uint8))


def test_encoder_refuses_bad_arguments():
    with pytest.raises(ValueError):
        I.JpegEncoder("cpu", 1, 8, 8, quality=0, ops=JpegEmuOps())
    with pytest.raises(ValueError):
        I.JpegEncoder("cpu", 1, 8, 65536, ops=JpegEmuOps())
    with pytest.raises(_lib.GanError):
        I.JpegEncoder("cpu", 1, 8, 8)                      # the HIP ops need a GPU: no CPU fallback


@pytest.fixture
def folder(monkeypatch, tmp_path):
    from PIL import Image
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: JpegEmuOps())
    monkeypatch.setattr(dataio, "InputPipeline", EmuInputPipeline)
    torch.manual_seed(3)
    G = cut.ResNetGenerator(3, 3, ngf=8, n_blocks=1).eval()
    for p in G.parameters():
        p.requires_grad_(False)
    photos = tmp_path / "photos"
    (photos / "sub").mkdir(parents=True)
    rng = np.random.default_rng(1)
    for name, (h, w) in (("a.png", (20, 24)), ("sub/b.png", (33, 17)), ("sub/c.png", (24, 24)), ("d.jpg", (40, 31)), ("e.png", (9, 50))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(photos / name)
    return G, photos, tmp_path


def _files(root):
    return {p.relative_to(root).as_posix(): p.read_bytes() for p in root.rglob("*") if p.is_file()}


def test_stylize_folder_device_jpeg_on_the_emulator(folder):
    G, photos, tmp = folder
    run = lambda out, **kw: I.stylize_folder(G, str(photos), str(tmp / out), device="cpu", img_size=24, batch=2, **kw)
    assert run("host") == 5 and run("dev", device_io=True) == 5
    want = _files(tmp / "dev")
    assert sorted(want) == ["a.jpg", "d.jpg", "e.jpg", "sub/b.jpg", "sub/c.jpg"] and want == _files(tmp / "host")
    assert run("jpeg", device_io=True, device_jpeg=True) == 5 and _files(tmp / "jpeg") == want
    assert isinstance(G._jpeg_enc, I.JpegEncoder) and (G._jpeg_enc.H, G._jpeg_enc.W, G._jpeg_enc.quality) == (24, 24, 95)
    enc = G._jpeg_enc
    assert run("jpeg4", device_io=True, device_jpeg=True, io_threads=4) == 5 and _files(tmp / "jpeg4") == want
    assert G._jpeg_enc is enc                                                       # cached on the generator, like the input pipeline
    assert run("dev4", device_io=True, io_threads=4) == 5 and _files(tmp / "dev4") == want
    assert run("host4", io_threads=4) == 5 and _files(tmp / "host4") == want
    with pytest.raises(ValueError, match="device_io"):
        run("bad", device_jpeg=True)
    with pytest.raises(ValueError, match="io_threads"):
        run("bad", io_threads=0)


def test_command_line_flags(folder, monkeypatch, capsys):
    """--device-jpeg / --io-threads reach stylize_folder; the run itself is put on the CPU emulator behind the command's back."""
    from gan_variant_research_amd import generate_folder as GF
    G, photos, tmp = folder
    ck = tmp / "ckpt.pt"
    torch.save({"generator": G.state_dict()}, ck)
    seen = []
    real_load, real_folder = I.load_generator, I.stylize_folder
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(I, "load_generator", lambda ckpt, device, **kw: real_load(ckpt, device="cpu", **kw))
    monkeypatch.setattr(I, "stylize_folder", lambda G, **kw: seen.append(dict(kw)) or real_folder(G, **dict(kw, device="cpu")))
    base = ["--ckpt", str(ck), "--photos", str(photos), "--size", "24", "--batch", "3", "--ngf", "8", "--n-blocks", "1", "--fp32"]
    assert GF.main(base + ["--out", str(tmp / "plain")]) == 5
    assert GF.main(base + ["--out", str(tmp / "jpeg"), "--device-jpeg", "--io-threads", "4"]) == 5
    assert [(k["device"], k["device_io"], k["device_jpeg"], k["io_threads"]) for k in seen] == [("cuda", True, False, 1), ("cuda", True, True, 4)]
    assert _files(tmp / "jpeg") == _files(tmp / "plain") and len(_files(tmp / "jpeg")) == 5
    a = GF.parse_args(["--ckpt", "c", "--photos", "p", "--out", "o"])
    assert (a.device_jpeg, a.io_threads) == (False, 1)
    for bad in (["--device-jpeg", "--host-io"], ["--device-jpeg", "--device", "cpu"], ["--io-threads", "0"]):
        with pytest.raises(SystemExit):
            GF.parse_args(["--ckpt", "c", "--photos", "p", "--out", "o"] + bad)
    assert "--device-jpeg" in capsys.readouterr().err
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)                   # no quiet fallback to PIL
    with pytest.raises(SystemExit, match="device-jpeg"):
        GF.main(base + ["--out", str(tmp / "x"), "--device-jpeg"])
    assert "Falling back" not in capsys.readouterr().out                             # refused before the fallback is announced


def test_entry_points_validate_before_they_launch():
    lib = _lib.load()
    ws, out = C.c_int64(0), C.c_int64(0)
    err = lambda: lib.gan_last_error()
    assert lib.gan_jpeg_bounds(16, 256, 256, C.byref(ws), C.byref(out)) == 0
    assert out.value == 2 * 16 * 3072 * 216 and ws.value >= 16 * 3072 * (128 + 4 + 216) and ws.value < 32 << 20
    assert lib.gan_jpeg_bounds(1, 4096, 4096, C.byref(ws), C.byref(out)) == 0       # bit offsets hold a 4096 x 4096 image
    assert lib.gan_jpeg_bounds(1, 16384, 16384, C.byref(ws), C.byref(out)) < 0 and b"32-bit" in err()
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 65536, 8), (1, 8, 65536), (-1, 8, 8), (65536, 8, 8)):     # B is a grid dimension
        assert lib.gan_jpeg_bounds(B, H, W, C.byref(ws), C.byref(out)) < 0 and b"65535" in err(), (B, H, W)
    assert lib.gan_jpeg_bounds(1, 8, 8, None, None) < 0 and b"null" in err()
    assert lib.gan_jpeg_bounds(1, 8, 8, C.byref(ws), C.byref(out)) == 0
    p = 1 << 20                                                                      # aligned, never dereferenced: validation fails first
    assert lib.gan_jpeg_blocks(None, 1, 8, 8, 95, p, ws.value, p, None) < 0 and b"null" in err()
    assert lib.gan_jpeg_blocks(p, 1, 8, 8, 95, None, ws.value, p, None) < 0 and b"null" in err()
    assert lib.gan_jpeg_blocks(p, 1, 8, 8, 95, p, ws.value, None, None) < 0 and b"null" in err()
    for q in (0, 101, -5):
        assert lib.gan_jpeg_blocks(p, 1, 8, 8, q, p, ws.value, p, None) < 0 and b"quality" in err()
    assert lib.gan_jpeg_blocks(p, 1, 8, 8, 95, p, ws.value - 1, p, None) < 0 and b"workspace" in err()
    assert lib.gan_jpeg_blocks(p, 1, 8, 8, 95, p + 4, ws.value, p, None) < 0 and b"aligned" in err()
    assert lib.gan_jpeg_blocks(p, 1, 8, 70000, 95, p, ws.value, p, None) < 0 and b"65535" in err()
    assert lib.gan_jpeg_tables(None, 4, p, p, None) < 0 and b"null" in err()
    assert lib.gan_jpeg_tables(p, 0, p, p, None) < 0 and b"tables" in err()
    assert lib.gan_jpeg_scan(p, ws.value, 1, 8, 8, p, None, out.value, p, None) < 0 and b"null" in err()
    assert lib.gan_jpeg_scan(p, ws.value, 1, 8, 8, p, p, out.value - 1, p, None) < 0 and b"output" in err()
    assert lib.gan_jpeg_scan(p, ws.value - 1, 1, 8, 8, p, p, out.value, p, None) < 0 and b"workspace" in err()
    assert lib.gan_jpeg_scan(p, ws.value, 1, 0, 8, p, p, out.value, p, None) < 0 and b"65535" in err()
