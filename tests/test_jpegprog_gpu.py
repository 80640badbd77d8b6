"""The progressive JPEG decoder on the GPU (csrc/jpegprog.hip): every case against the golden pixels, the mixed call, the flagged files
(the sanitizer program of tests/test_jpegprog_cpu.py has handled the same bytes), the refusals of the C entries, stylize_folder, and
the baseline path with the switch on."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from gan_variant_research_amd import _lib, cut, dataio, inference as I
from tests import jpegdec_cases as DC, jpegprog_cases as PC
from tests.test_jpegprog_cpu import check_mixed, expectation, mixed_call

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def equals_golden(name, t) -> bool:
    px = t.cpu().numpy()
    return tuple(px.shape) == PC.shape(name) + (3,) and hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest() == PC.pixels_sha256(name)


@pytest.fixture(scope="module")
def dec():
    return dataio.JpegDecoder(DEV, progressive=True)


def test_every_case_decodes_to_the_golden_pixels_one_by_one_and_together(dec):
    before = dict(dec.stats)
    for name in PC.ALL:
        got = dec.decode([PC.file(name)])[0]
        assert equals_golden(name, got) and dec.last_errors == {}, name
    assert dec.stats["device"] == before["device"] + len(PC.ALL) and dec.progressive_stats["device"] >= len(PC.ALL)
    first = dec.decode([PC.file(n) for n in PC.ALL])
    for name, g in zip(PC.ALL, first):
        assert equals_golden(name, g), name
    again = dec.decode([PC.file(n) for n in PC.ALL])
    assert all(torch.equal(a, b) for a, b in zip(first, again)) and dec.last_errors == {}


def test_mixed_call():
    d = dataio.DeviceDecoder(DEV, progressive=True)
    check_mixed(*mixed_call(d))
    assert d.stats == {"device": 6, "unsupported": 1, "flagged": 1} and d.progressive_stats == {"device": 3, "unsupported": 1, "flagged": 1}
    assert d.last_errors == {PC.MIXED.index("corrupt"): expectation(PC.file("corrupt"))[0]}


def test_flagged_files_come_back_with_their_words_and_pillows_outcome(dec):
    got = dec.decode([PC.file(n) for n in PC.FLAGGED])
    for i, (n, word) in enumerate(PC.FLAGGED.items()):
        assert np.array_equal(got[i].cpu().numpy(), PC.pixels(n)), n
        want = expectation(PC.file(n))[0]                          # the reference's word, lane for lane: the crafted files' is the bit they are named for
        assert dec.last_errors[i] == want != 0 and word in (None, want), (n, dec.last_errors)


def test_baseline_only_decode_with_the_switch_on_equals_todays(dec):
    plain = dataio.JpegDecoder(DEV)
    names = DC.PIXEL_CASES
    a, b = dec.decode([DC.file(n) for n in names]), plain.decode([DC.file(n) for n in names])
    for n, x, y in zip(names, a, b):
        assert torch.equal(x, y) and np.array_equal(x.cpu().numpy(), DC.pixels(n)), n
    assert plain.progressive_stats == {"device": 0, "unsupported": 0, "flagged": 0}


def test_entry_points_validate_before_they_launch():
    """Every refusal is made on the host copy of the descriptors: the device pointers are aligned numbers that are never used."""
    lib = _lib.load()
    err = lambda: lib.gan_last_error()
    off = (C.c_int64 * 6)()
    from tests.emulator_jpegprog import JpegProgEmuOps, block_offsets
    assert lib.gan_jpegprog_block_offsets(3, 30, 70, 24, off) == 0 and tuple(off) == block_offsets(3, 30, 70, 24) and all(o % 16 == 0 for o in off)
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 65, 1, 1), (1, 1, 1, 65), (65536, 1, 1, 1)):
        assert lib.gan_jpegprog_block_offsets(*bad, off) < 0 and b"outside" in err(), bad
    assert lib.gan_jpegprog_block_offsets(1, 1, 1, 1, None) < 0 and b"null" in err()
    prog = dataio.JpegDecoder("cpu", ops=JpegProgEmuOps(), progressive=True)._prog
    names = ["rst", "gray", "deep"]
    plans = [dataio.parse_jpeg_progressive(PC.file(n)) for n in names]
    offs = [sum(p["H"] * p["W"] * 3 for p in plans[:i]) for i in range(len(plans))]
    total, n, nscan, nseg, nver, ws_bytes = prog._pack(plans, offs)
    host = prog._host
    ws = C.c_int64(0)
    imgs = (_lib.GanJpegdecImage * n).from_buffer_copy(host[:n * C.sizeof(_lib.GanJpegdecImage)].numpy().tobytes())
    assert lib.gan_jpegprog_bounds(C.cast(imgs, C.c_void_p), n, nver, C.byref(ws)) == 0 and ws.value == ws_bytes      # the emulator's layout is the library's
    assert lib.gan_jpegprog_bounds(None, n, nver, C.byref(ws)) < 0 and b"null" in err()
    p, hp = 1 << 20, host.data_ptr()
    o_pimg, o_scan, o_seg, o_dht, o_qt, o_data = block_offsets(n, nscan, nseg, nver)
    i32 = host.numpy()[:total].view(np.int32)
    entries = [lambda *a: lib.gan_jpegprog_tables(*a, None), lambda *a: lib.gan_jpegprog_entropy(*a, None), lambda *a: lib.gan_jpegprog_idct(*a, None),
               lambda *a: lib.gan_jpegprog_pixels(*a, p, 1 << 30, None, None)]
    good = (p, hp, total, n, nscan, nseg, nver, p, ws_bytes)
    for call in entries:
        assert call(None, *good[1:]) < 0 and b"null" in err()
        assert call(p, None, *good[2:]) < 0 and b"null" in err()
        assert call(*good[:7], None, ws_bytes) < 0 and b"null" in err()
        assert call(*good[:7], p + 4, ws_bytes) < 0 and b"aligned" in err()
        assert call(p + 8, *good[1:]) < 0 and b"aligned" in err()
        assert call(p, hp, 100, *good[3:]) < 0 and b"descriptors" in err()
        assert call(*good[:8], int(imgs[n - 1].plane_off)) < 0 and b"workspace" in err()
        assert call(p, hp, total, n, n * 64 + 1, nseg, nver, p, ws_bytes) < 0 and b"outside" in err()
        assert call(p, hp, total, n, nscan, nseg, n * 64 + 1, p, ws_bytes) < 0 and b"outside" in err()
    call = entries[1]
    pimg = lambda i, k: o_pimg // 4 + 8 * i + k
    scan = lambda j, k: o_scan // 4 + 16 * j + k
    seg = lambda j, k: o_seg // 4 + 8 * j + k
    second = len(plans[0]["scans"])                        # the first scan of image 1
    for at, value, word in ((pimg(0, 1), 65, b"scans"), (pimg(1, 0), nscan, b"scans"), (pimg(0, 5), 65, b"versions"), (pimg(2, 4), nver, b"versions"),
                            (pimg(1, 3), nseg + 1, b"segments"), (pimg(0, 6), 0, b"levels"), (scan(0, 0), 1, b"names image"), (scan(1, 1), 3, b"component"),
                            (scan(1, 2), 64, b"band"), (scan(1, 3), 64, b"band"), (scan(1, 5), 14, b"approximation"), (scan(5, 4), 3, b"approximation"),
                            (scan(1, 6), 64, b"table version"), (scan(0, 6), -1, b"table version"), (scan(5, 9), 5, b"dependency"), (scan(5, 9), 7, b"dependency"),
                            (scan(second + 3, 9), 3, b"dependency"), (scan(5, 10), 0, b"level"), (scan(5, 10), 99, b"level"),
                            (seg(0, 0), 1, b"names image"), (seg(0, 1), nscan - 1, b"names scan"), (seg(1, 4), 10 ** 6, b"units"), (seg(1, 3), -1, b"units"),
                            (seg(1, 2), 2, b"does not continue"), (seg(1, 3), 4, b"does not continue"), (seg(3, 4), 2, b"cover"),
                            (seg(2, 5), 0, b"scan area"), (seg(2, 6), total + 1, b"scan area")):
        keep, i32[at] = int(i32[at]), value
        assert call(*good) < 0 and word in err(), (at, value, err())
        i32[at] = keep
    i64 = host.numpy()[:total].view(np.int64)
    at = (2 * C.sizeof(_lib.GanJpegdecImage) + _lib.GanJpegdecImage.out_off.offset) // 8
    for value in (-1, (1 << 30) - 5):
        keep, i64[at] = int(i64[at]), value
        assert lib.gan_jpegprog_pixels(*good, p, 1 << 30, None, None) < 0 and b"output" in err()
        i64[at] = keep
    assert lib.gan_jpegprog_pixels(*good, None, 1 << 30, None, None) < 0 and b"null" in err()


def test_stylize_folder_with_the_switch_writes_the_files_of_the_pillow_path(tmp_path):
    from PIL import Image
    torch.manual_seed(3)
    G = cut.ResNetGenerator(3, 3, ngf=8, n_blocks=1).eval().to(DEV)
    for q in G.parameters():
        q.requires_grad_(False)
    photos = tmp_path / "photos"
    photos.mkdir()
    rng = np.random.default_rng(1)
    for name, (h, w), prog in (("a.jpg", (20, 24), False), ("b.jpg", (33, 17), True), ("c.jpg", (24, 24), True), ("d.jpg", (40, 31), False)):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(photos / name, quality=90, progressive=prog)
    Image.fromarray(rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)).save(photos / "f.png")
    run = lambda out, **kw: I.stylize_folder(G, str(photos), str(tmp_path / out), device=DEV, img_size=24, batch=2, device_io=True, **kw)
    files = lambda root: {q.name: q.read_bytes() for q in root.iterdir()}
    assert run("pil") == 5 and run("prog", device_decode=True, device_progressive=True, decode_chunk=3) == 5
    assert files(tmp_path / "prog") == files(tmp_path / "pil")
    assert G._jpeg_dec.stats == {"device": 4, "unsupported": 1, "flagged": 0} and G._jpeg_dec.progressive_stats == {"device": 2, "unsupported": 0, "flagged": 0}
