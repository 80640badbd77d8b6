"""The JPEG decoder off the GPU: tests.jpegdec_ref (the statement csrc/jpegdec.hip is held to) against the golden pixels and Pillow
itself; the parser's accepted class; the decoder's arithmetic (csrc/jpegdec_core.h, the text the kernels compile) as a host program
under AddressSanitizer / UBSan over every case and its corrupted variants; dataio.JpegDecoder, ImageStore(device_decode=True),
stylize_folder(device_decode=True) and the command line on the emulator; the argument checks of the C entries (no launch)."""
import ctypes as C
import hashlib
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gan_variant_research_amd import _lib, autograd as AG, cut, dataio, inference as I
from tests import jpegdec_cases as DC, jpegdec_ref as R
from tests.emulator_jpeg import EmuInputPipeline
from tests.emulator_jpegdec import JpegDecEmuOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def equals_golden(name, px) -> bool:
    return tuple(px.shape) == DC.CASES.get(name, (0, 0))[:2] + (3,) and hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest() == DC.pixels_sha256(name)


@pytest.mark.parametrize("name", list(DC.CASES))
def test_ref_equals_golden_and_live_pillow(name):
    from PIL import features
    st = R.stages(DC.file(name))
    assert equals_golden(name, st.pixels) and not st.extreme
    live = R.pillow_pixels(DC.file(name))
    if not equals_golden(name, live):
        pytest.skip(f"the reference equals the golden pixels; live Pillow (libjpeg {features.version('jpg')}) differs from them, comparison with it skipped")


def test_cases_hit_what_they_are_for():
    p = {n: R.parse(DC.file(n)) for n in DC.CASES}
    assert (len(p["rst"].segments), p["rst"].per, p["rst"].mcux * p["rst"].mcuy) == (4, 3, 12)
    assert (len(p["rst_wrap"].segments), p["rst_wrap"].per) == (64, 1)                    # lane 63 works, RSTn wraps eight times
    b, e = p["stuffing"].segments[0]
    assert b"\xff\x00" in DC.file("stuffing")[b:e]
    assert {(q.hmax, q.vmax, len(q.comps)) for q in p.values()} == {(1, 1, 3), (2, 1, 3), (2, 2, 3), (1, 1, 1)}
    assert all(sum(dc[0]) == 1 and sum(ac[0]) == 1 for *_, dc, ac in p["const"].comps)      # one-symbol tables
    assert any(0xF0 in ac[1] for *_, ac in p["runs"].comps)                                   # ZRL
    assert any(sum(ac[0][9:]) > 0 for *_, ac in p["std_tables"].comps)                        # codes longer than the lookahead width exist
    assert max(int(np.abs(c).max()) for c in R.coefficients(p["magnitudes"])) >= 512
    assert -(-p["wide"].H // 2) == 16 and p["narrow.4.420"].W == 4 and p["narrow.5.420"].W == 5
    assert R.stages(DC.file("crafted")).extreme                                             # the IDCT bounds are what sends it to Pillow
    with pytest.raises(R.Corrupt):
        R.decode(DC.file("corrupt"))
    assert sum(a != b for a, b in zip(DC.file("corrupt"), DC.file("std_tables"))) == DC.CORRUPT_BYTES
    assert set(DC.BATCH) <= set(DC.PIXEL_CASES) and len({DC.pixels(n).shape for n in DC.BATCH}) == len(DC.BATCH)


# ------------------------------------------------------------------------------------------------ the parser
def _patched(data: bytes, marker: int, at: int, value: int, nth: int = 0) -> bytes:
    """`data` with byte `at` of the body of the nth segment `marker` replaced."""
    pos, seen = 2, 0
    while True:
        m, L = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        if m == marker:
            if seen == nth:
                return data[:pos + 4 + at] + bytes([value]) + data[pos + 5 + at:]
            seen += 1
        assert m != 0xDA, "segment not found"
        pos += 2 + L


def test_parser_accepts_the_supported_class():
    for name in list(DC.CASES) + ["crafted", "corrupt"]:
        plan, p = dataio.parse_jpeg(DC.file(name)), R.parse(DC.file(name))
        assert plan is not None, name
        assert (plan["H"], plan["W"], plan["ncomp"], plan["hmax"], plan["vmax"], plan["mcux"], plan["mcuy"]) == (p.H, p.W, len(p.comps), p.hmax, p.vmax, p.mcux, p.mcuy)
        assert list(zip(plan["seg_begin"].tolist(), plan["seg_end"].tolist())) == p.segments and plan["per"] == p.per, name
        for c, (_, _, q, dc, ac) in enumerate(p.comps):
            assert np.array_equal(plan["qt"][plan["q_tab"][c]], q)
            assert list(plan["dht"][plan["dc_tab"][c]]) == dc[0] + dc[1] and list(plan["dht"][plan["ac_tab"][c]]) == ac[0] + ac[1]
    assert dataio.JpegDecoder.parse(DC.file("mcu.444")) is not None


def test_parser_refuses_everything_else():
    for name in ("progressive", "cmyk", "s411", "adobe", "png"):
        assert dataio.parse_jpeg(DC.file(name)) is None, name
        with pytest.raises((R.NotBaseline, AssertionError)):
            R.parse(DC.file(name))
    base = DC.file("mcu.420")
    assert dataio.parse_jpeg(base) is not None
    eoi = base.rindex(b"\xff\xd9")
    refused = {
        "truncated": DC.truncated(),
        "no EOI": base[:eoi],
        "empty": b"", "not a jpeg": b"\x00" * 64, "SOI only": b"\xff\xd8",
        "12-bit": _patched(base, 0xC0, 0, 12),
        "16-bit quantisation table": _patched(base, 0xDB, 0, 0x10),
        "height 0 (DNL)": _patched(_patched(base, 0xC0, 1, 0), 0xC0, 2, 0),
        "4:4:0": _patched(base, 0xC0, 7, 0x12),
        "4:1:1": _patched(base, 0xC0, 7, 0x41),
        "chroma 2x1": _patched(base, 0xC0, 10, 0x21),
        "component ids RGB": _patched(base, 0xC0, 6, ord("R")),
        "spectral selection": _patched(base, 0xDA, 7, 1),
        "successive approximation": _patched(base, 0xDA, 9, 0x10),
        "table slot 2": _patched(base, 0xDA, 2, 0x22),
        "a scan of one component": _patched(base, 0xDA, 0, 1),
        "over-subscribed DHT": _patched(base, 0xC4, 1, 3),
        "arithmetic coding": base.replace(b"\xff\xc0", b"\xff\xc9", 1),
        "extended sequential": base.replace(b"\xff\xc0", b"\xff\xc1", 1),
        "two scans": base[:eoi] + base[base.index(b"\xff\xda"):],
        "a DNL after the scan": base[:eoi] + b"\xff\xdc\x00\x04\x00\x10" + base[eoi:],
        "fill bytes in the scan": base[:eoi] + b"\xff" + base[eoi:],
        "an unknown marker": base[:2] + b"\xff\xf7\x00\x02" + base[2:],
        "a restart marker the interval does not ask": base[:eoi] + b"\xff\xd0" + base[eoi:],
        "gray sampled 2x2": _patched(DC.file("gray"), 0xC0, 7, 0x22),
    }
    rst = DC.file("rst")
    first = rst.index(b"\xff\xd0")
    refused["a missing restart marker"] = rst[:first] + rst[first + 2:]
    for what, data in refused.items():
        assert dataio.parse_jpeg(data) is None, what
    # what Pillow ignores, the parser passes: comments, APPn other than Adobe, bytes after EOI
    for data in (base[:2] + b"\xff\xfe\x00\x05abc" + base[2:], base[:2] + b"\xff\xe1\x00\x08Exif\x00\x00" + base[2:], base + b"trailing"):
        assert dataio.parse_jpeg(data) is not None and np.array_equal(R.decode(data), DC.pixels("mcu.420"))


# ------------------------------------------------------------------------------------------------ the arithmetic under sanitizers
def corrupt_variants(name: str, k: int = 6):
    """Deterministic damage to the scan of a case: bytes overwritten, the scan cut short (its EOI kept), bytes inserted."""
    d = DC.file(name)
    p = R.parse(d)
    b, e = p.segments[0][0], p.segments[-1][1]
    rng = np.random.default_rng(sum(name.encode()))
    out = []
    for i in range(k):
        v = bytearray(d)
        if e - b < 4:
            break
        if i % 3 == 0:
            for pos in rng.integers(b, e, 1 + i % 4):
                v[pos] = int(rng.integers(0, 255))
        elif i % 3 == 1:
            cut = int(rng.integers(b + 1, e))
            v = v[:cut] + v[e:]
        else:
            at = int(rng.integers(b, e))
            v = v[:at] + bytes(rng.integers(0, 255, 1 + i, dtype=np.uint8)) + v[at:]
        out.append(bytes(v))
    return out


def expectation(data: bytes):
    """(error expected, pixels otherwise) by tests.jpegdec_ref."""
    try:
        st = R.stages(data)
    except R.Corrupt:
        return True, None
    return st.extreme, st.pixels


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("HOSTCXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler (c++, g++ or clang++) or no make on this machine: the sanitizer build of csrc/jpegdec_host.cpp cannot be made")
    exe = tmp_path_factory.mktemp("jpegdec_host") / "jpegdec_host"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gan-variant-research_amd", "csrc"), "jpegdec_host", f"HOSTCXX={cxx}", f"HOSTBIN={exe}"],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip(f"{cxx} has no AddressSanitizer / UBSan runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


def run_host(exe, files, tmp_path):
    """The files (all accepted by the parser) through the host program -> (error words, pixel arrays)."""
    dec = dataio.JpegDecoder("cpu", ops=JpegDecEmuOps())
    plans = [dataio.parse_jpeg(f) for f in files]
    offs, end = [], 0
    for p in plans:
        offs.append(end)
        end += p["H"] * p["W"] * 3
    total, n, nseg, ws = dec._pack(plans, offs)
    o = dec.ops.jpegdec_block_offsets(n, nseg)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(np.array([total, n, nseg, ws, end, o[0], o[1], o[2]], np.int64).tobytes() + dec._host[:total].numpy().tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]                 # a sanitizer report ends the program with a non-zero status
    raw = np.fromfile(dst, np.uint8)
    return raw[:4 * n].view(np.int32).tolist(), [raw[4 * n + o:][:p["H"] * p["W"] * 3].reshape(p["H"], p["W"], 3) for o, p in zip(offs, plans)]


def test_host_program_under_sanitizers(host_program, tmp_path):
    """Every case, then every corrupted variant the parser still takes: no sanitizer report, the pixels or the error word that
    tests.jpegdec_ref expects.  The GPU tests decode the corrupt files only after this."""
    names = list(DC.CASES)
    err, px = run_host(host_program, [DC.file(n) for n in names], tmp_path)
    assert err == [0] * len(names)
    for n, p in zip(names, px):
        assert equals_golden(n, p), n
    err, px = run_host(host_program, [DC.file("crafted"), DC.file("corrupt")], tmp_path)
    assert err[0] == 128 and err[1] != 0 and err[1] & 128 == 0
    variants = [v for n in names if n != "long" for v in corrupt_variants(n)] + corrupt_variants("long", 3)
    taken = [v for v in variants if dataio.parse_jpeg(v) is not None]
    assert len(taken) >= len(variants) // 2 and len(variants) > 100
    want = [expectation(v) for v in taken]
    err, px = run_host(host_program, taken, tmp_path)
    flagged = 0
    for i, ((bad, pixels), e, p) in enumerate(zip(want, err, px)):
        assert bool(e) == bad, (i, e)
        flagged += bad
        if not bad:
            assert np.array_equal(p, pixels), i
    assert flagged >= len(taken) // 2 and {e for e in err if e} >= {1, 2, 4, 16}       # the kinds of irregularity the variants produce


# ------------------------------------------------------------------------------------------------ JpegDecoder on the emulator
def test_decoder_equals_pillow_and_counts_the_fallbacks(tmp_path):
    dec = dataio.JpegDecoder("cpu", ops=JpegDecEmuOps())
    names = DC.PIXEL_CASES
    got = dec.decode([DC.file(n) for n in names])
    for n, g in zip(names, got):
        assert g.dtype == torch.uint8 and np.array_equal(g.numpy(), DC.pixels(n)), n
    assert dec.stats == {"device": len(names), "unsupported": 0, "flagged": 0} and dec.last_errors == {}
    paths = []
    for n in DC.FALLBACK + DC.BATCH:                          # paths and bytes are both sources
        paths.append(tmp_path / (n + (".png" if n == "png" else ".jpg")))
        paths[-1].write_bytes(DC.file(n))
    got = dec.decode(paths)
    for n, g in zip(DC.FALLBACK + DC.BATCH, got):
        assert np.array_equal(g.numpy(), DC.pixels(n)), n
    assert dec.stats == {"device": len(names) + len(DC.BATCH), "unsupported": 5, "flagged": 2}
    assert dec.last_errors[DC.FALLBACK.index("crafted")] == 128 and dec.last_errors[DC.FALLBACK.index("corrupt")] not in (0, 128)
    assert all((g.data_ptr() - got[0].data_ptr()) % dataio.ARENA_ALIGN == 0 for g in got)


def test_decoder_reused_and_writing_into_a_callers_buffer():
    dec = dataio.JpegDecoder("cpu", ops=JpegDecEmuOps())
    for names in (DC.BATCH, DC.BATCH + ["wide", "runs", "png"], DC.BATCH[:2], DC.BATCH[::-1]):      # larger, smaller, reordered
        for n, g in zip(names, dec.decode([DC.file(n) for n in names])):
            assert np.array_equal(g.numpy(), DC.pixels(n)), n
    sizes = [DC.pixels(n).size for n in DC.BATCH]
    offsets = [7 + sum(sizes[:i]) + 3 * i for i in range(len(sizes))]                                  # packed, unaligned
    out = torch.full((offsets[-1] + sizes[-1] + 5,), 0xAB, dtype=torch.uint8)
    got = dec.decode([DC.file(n) for n in DC.BATCH], out=out, offsets=offsets)
    used = np.zeros(out.numel(), bool)
    for n, g, o, s in zip(DC.BATCH, got, offsets, sizes):
        assert g.data_ptr() == out.data_ptr() + o and np.array_equal(g.numpy(), DC.pixels(n))
        used[o:o + s] = True
    assert (out.numpy()[~used] == 0xAB).all()                                                         # nothing else was written
    with pytest.raises(_lib.GanError):
        dec.decode([DC.file("gray")], out=out)                                                        # offsets missing
    with pytest.raises(_lib.GanError):
        dataio.JpegDecoder("cpu")                                                                     # the HIP ops need a GPU: no CPU fallback


def test_truncated_file_raises_what_the_pillow_path_raises(tmp_path):
    p = tmp_path / "cut.jpg"
    p.write_bytes(DC.truncated())
    with pytest.raises(OSError) as plain:
        dataio._decode(p)
    dec = dataio.JpegDecoder("cpu", ops=JpegDecEmuOps())
    with pytest.raises(OSError) as mine:
        dec.decode([DC.file("gray"), p])
    assert str(mine.value) == str(plain.value) and str(p) in str(mine.value)


# ------------------------------------------------------------------------------------------------ the store, the folder path, the command line
@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: JpegDecEmuOps())
    monkeypatch.setattr(dataio, "InputPipeline", EmuInputPipeline)


def _write_folder(root, names):
    root.mkdir(parents=True, exist_ok=True)
    paths = []
    for n in names:
        paths.append(root / (n.replace(".", "_") + (".png" if n == "png" else ".jpg")))
        paths[-1].write_bytes(DC.file(n))
    return paths


@pytest.mark.parametrize("budget", [None, 0], ids=["resident", "streaming"])
def test_image_store_device_decode_holds_the_same_bytes(emulated, tmp_path, monkeypatch, budget):
    names = DC.BATCH + ["png", "progressive", "corrupt", "crafted", "wide"]
    paths = _write_folder(tmp_path / "imgs", names)
    monkeypatch.setattr(dataio, "DECODE_CHUNK", 4)                       # several chunks
    plain = dataio.ImageStore(paths, "cpu", budget_bytes=budget, workers=2)
    store = dataio.ImageStore(paths, "cpu", budget_bytes=budget, workers=2, device_decode=True)
    assert store.resident == plain.resident == (budget is None)
    assert store.sizes == plain.sizes and store.offsets == plain.offsets and store.nbytes == plain.nbytes
    for i, n in enumerate(names):
        assert np.array_equal(store[i].numpy(), DC.pixels(n)) and torch.equal(store[i], plain[i]), n
    order = [7, 0, 3, 3, 9]
    for a, b in zip(store.fetch(order), plain.fetch(order)):
        assert torch.equal(a, b)
    st = store._decoder.stats
    assert st["unsupported"] > 0 and st["flagged"] > 0 and st["device"] > 0
    if budget is None:
        assert st == {"device": 7, "unsupported": 2, "flagged": 2}
    store.close(), plain.close()


def test_image_store_reports_an_undecodable_file_as_before(emulated, tmp_path):
    paths = _write_folder(tmp_path / "imgs", ["gray", "rst"])
    paths[1].write_bytes(DC.truncated())
    errors = []
    for dd in (False, True):
        with pytest.raises(OSError) as e:
            dataio.ImageStore(paths, "cpu", workers=2, device_decode=dd)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and errors[0].startswith(f"cannot decode image {paths[1]}")


def test_trainers_pass_the_config_key_to_their_stores(emulated, tmp_path):
    from gan_variant_research_amd import train_cutpp
    paths = _write_folder(tmp_path / "imgs", ["gray", "wide"])
    off = train_cutpp.build_store(paths, "cpu", {}, "A", quiet=True)
    on = train_cutpp.build_store(paths, "cpu", {"mi355x": {"device_decode": True}}, "A", quiet=True)
    assert off._decoder is None and on._decoder.stats["device"] == 2 and all(torch.equal(on[i], off[i]) for i in range(2))


@pytest.fixture
def folder(emulated, tmp_path):
    from PIL import Image
    torch.manual_seed(3)
    G = cut.ResNetGenerator(3, 3, ngf=8, n_blocks=1).eval()
    for p in G.parameters():
        p.requires_grad_(False)
    photos = tmp_path / "photos"
    (photos / "sub").mkdir(parents=True)
    rng = np.random.default_rng(1)
    for name, (h, w) in (("a.jpg", (20, 24)), ("sub/b.jpg", (33, 17)), ("sub/c.jpg", (24, 24)), ("d.jpg", (40, 31)), ("e.jpg", (9, 50))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(photos / name, quality=90)
    Image.fromarray(rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)).save(photos / "f.png")
    Image.fromarray(rng.integers(0, 256, (16, 30, 3), dtype=np.uint8)).save(photos / "sub" / "g.jpg", progressive=True)
    return G, photos, tmp_path


def _files(root):
    return {p.relative_to(root).as_posix(): p.read_bytes() for p in root.rglob("*") if p.is_file()}


def test_stylize_folder_device_decode_on_the_emulator(folder):
    G, photos, tmp = folder
    run = lambda out, **kw: I.stylize_folder(G, str(photos), str(tmp / out), device="cpu", img_size=24, batch=2, device_io=True, **kw)
    assert run("pil") == 7
    want = _files(tmp / "pil")
    assert len(want) == 7
    assert run("dec", device_decode=True) == 7 and _files(tmp / "dec") == want
    assert G._jpeg_dec.stats == {"device": 5, "unsupported": 2, "flagged": 0}
    dec = G._jpeg_dec
    for chunk in (1, 3, 16):                                                   # chunks smaller than, across and larger than the batches
        assert run(f"dec{chunk}", device_decode=True, decode_chunk=chunk, io_threads=3, device_jpeg=True) == 7 and _files(tmp / f"dec{chunk}") == want
    assert G._jpeg_dec is dec                                                  # cached on the generator, like the input pipeline
    assert run("lim", device_decode=True, limit=3) == 3 and _files(tmp / "lim") == {k: want[k] for k in sorted(want)[:3]}
    with pytest.raises(ValueError, match="device_io"):
        I.stylize_folder(G, str(photos), str(tmp / "bad"), device="cpu", img_size=24, device_decode=True)
    with pytest.raises(ValueError, match="decode_chunk"):
        run("bad", device_decode=True, decode_chunk=0)


def test_command_line_flags(folder, monkeypatch, capsys):
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
    assert GF.main(base + ["--out", str(tmp / "plain")]) == 7
    assert GF.main(base + ["--out", str(tmp / "dec"), "--device-decode", "--decode-chunk", "4"]) == 7
    assert "device_decode" not in seen[0] and "decode_chunk" not in seen[0]          # with the flag off the call is the parent's
    assert (seen[1]["device_decode"], seen[1]["decode_chunk"], seen[1]["device_io"]) == (True, 4, True)
    assert _files(tmp / "dec") == _files(tmp / "plain") and len(_files(tmp / "dec")) == 7
    a = GF.parse_args(["--ckpt", "c", "--photos", "p", "--out", "o"])
    assert (a.device_decode, a.decode_chunk) == (False, 256)
    for bad in (["--device-decode", "--host-io"], ["--device-decode", "--device", "cpu"], ["--decode-chunk", "0"]):
        with pytest.raises(SystemExit):
            GF.parse_args(["--ckpt", "c", "--photos", "p", "--out", "o"] + bad)
    assert "--device-decode" in capsys.readouterr().err
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)                   # no quiet fallback to PIL
    with pytest.raises(SystemExit, match="device-decode"):
        GF.main(base + ["--out", str(tmp / "x"), "--device-decode"])
    assert "Falling back" not in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ the C entries
def packed(names, out_offsets=None):
    """A valid upload block of the named cases in host memory -> (keep-alive decoder, block tensor, bytes, n, nseg, ws bytes)."""
    dec = dataio.JpegDecoder("cpu", ops=JpegDecEmuOps())
    plans = [dataio.parse_jpeg(DC.file(n)) for n in names]
    offs = out_offsets or [sum(p["H"] * p["W"] * 3 for p in plans[:i]) for i in range(len(plans))]
    total, n, nseg, ws = dec._pack(plans, offs)
    return dec, dec._host, total, n, nseg, ws


def test_entry_points_validate_before_they_launch():
    """Every refusal below is made on the host copy of the descriptors: the device pointers are aligned numbers that are never used."""
    lib = _lib.load()
    err = lambda: lib.gan_last_error()
    off = (C.c_int64 * 4)()
    assert lib.gan_jpegdec_block_offsets(3, 7, off) == 0
    from tests.emulator_jpegdec import block_offsets
    assert tuple(off) == block_offsets(3, 7) and off[2] % 16 == 0 and off[3] % 16 == 0
    for n, nseg in ((0, 1), (1, 0), (65536, 1), (-1, 1)):
        assert lib.gan_jpegdec_block_offsets(n, nseg, off) < 0 and b"65535" in err()
    assert lib.gan_jpegdec_block_offsets(1, 1, None) < 0 and b"null" in err()
    # bounds: the library's layout is the emulator's; geometry outside the class is refused
    dec, host, total, n, nseg, ws_bytes = packed(DC.BATCH)
    imgs = (_lib.GanJpegdecImage * n).from_buffer_copy(host[:n * C.sizeof(_lib.GanJpegdecImage)].numpy().tobytes())
    mine = [(im.coef_off, im.plane_off) for im in imgs]
    ws = C.c_int64(0)
    assert lib.gan_jpegdec_bounds(C.cast(imgs, C.c_void_p), n, C.byref(ws)) == 0 and ws.value == ws_bytes
    assert [(im.coef_off, im.plane_off) for im in imgs] == mine
    assert lib.gan_jpegdec_bounds(None, n, C.byref(ws)) < 0 and b"null" in err()
    for field, value, word in (("H", 0, b"65535"), ("W", 65536, b"65535"), ("ncomp", 2, b"class"), ("hmax", 4, b"class"), ("mcux", 99, b"MCUs")):
        bad = (_lib.GanJpegdecImage * 1).from_buffer_copy(bytes(imgs)[:C.sizeof(_lib.GanJpegdecImage)])
        setattr(bad[0], field, value)
        assert lib.gan_jpegdec_bounds(C.cast(bad, C.c_void_p), 1, C.byref(ws)) < 0 and word in err(), field
    # the launching entries
    p = 1 << 20                                    # aligned, never dereferenced: validation fails first
    hp = host.data_ptr()
    img_at = lambda i, field: i * C.sizeof(_lib.GanJpegdecImage) + getattr(_lib.GanJpegdecImage, field).offset
    seg_at = lambda j, k: n * C.sizeof(_lib.GanJpegdecImage) + 20 * j + 4 * k
    assert total % 16 == 0
    i32, i64 = host.numpy()[:total].view(np.int32), host.numpy()[:total].view(np.int64)
    last_end = int(i32[seg_at(nseg - 1, 4) // 4])
    entries = [lambda *a: lib.gan_jpegdec_tables(*a, None), lambda *a: lib.gan_jpegdec_entropy(*a, None), lambda *a: lib.gan_jpegdec_idct(*a, None),
               lambda *a: lib.gan_jpegdec_pixels(*a, p, 1 << 30, None, None)]
    good = (p, hp, total, n, nseg, p, ws_bytes)
    for call in entries:
        assert call(None, hp, total, n, nseg, p, ws_bytes) < 0 and b"null" in err()
        assert call(p, None, total, n, nseg, p, ws_bytes) < 0 and b"null" in err()
        assert call(p, hp, total, n, nseg, None, ws_bytes) < 0 and b"null" in err()
        assert call(p, hp, total, 0, nseg, p, ws_bytes) < 0 and b"65535" in err()
        assert call(p, hp, total, n, 0, p, ws_bytes) < 0 and b"segments" in err()
        assert call(p, hp, total, n, nseg, p, int(imgs[n - 1].plane_off)) < 0 and b"workspace" in err()
        assert call(p, hp, total, n, nseg, p + 4, ws_bytes) < 0 and b"aligned" in err()
        assert call(p + 8, hp, total, n, nseg, p, ws_bytes) < 0 and b"aligned" in err()
        assert call(p, hp, 100, n, nseg, p, ws_bytes) < 0 and b"descriptors" in err()
        assert call(p, hp, last_end - 1, n, nseg, p, ws_bytes) < 0 and b"scan area" in err()  # the block ends inside the last segment
    call = entries[1]
    for at, value, word in ((img_at(1, "H") // 4, 70000, b"65535"), (img_at(2, "ncomp") // 4, 4, b"class"), (img_at(0, "mcuy") // 4, 1000, b"MCUs"),
                            (img_at(0, "dc_tab") // 4 + 1, 2, b"slots"), (img_at(3, "q_tab") // 4, 4, b"slots"), (img_at(2, "seg_count") // 4, 9, b"segments"),
                            (img_at(0, "seg_first") // 4, -1, b"segments"), (seg_at(0, 0) // 4, 1, b"names image"), (seg_at(1, 2) // 4, 10 ** 6, b"MCUs"),
                            (seg_at(1, 1) // 4, -1, b"MCUs"), (seg_at(2, 3) // 4, 0, b"scan area"), (seg_at(2, 4) // 4, total + 1, b"scan area"),
                            (seg_at(nseg - 1, 4) // 4, 5, b"scan area")):
        keep, i32[at] = int(i32[at]), value
        assert call(*good) < 0 and word in err(), (at, value, err())
        i32[at] = keep
    for field, value, word in (("coef_off", 0, b"coefficient"), ("coef_off", ws_bytes, b"coefficient"), ("coef_off", 1 << 40, b"coefficient"),
                               ("plane_off", 8, b"plane"), ("plane_off", ws_bytes - 8, b"plane")):
        at = img_at(n - 1, field) // 8
        keep, i64[at] = int(i64[at]), value
        assert call(*good) < 0 and word in err(), (field, value)
        i64[at] = keep
    at = img_at(n - 1, "out_off") // 8
    for value in (-1, (1 << 30) - 5):
        keep, i64[at] = int(i64[at]), value
        assert lib.gan_jpegdec_pixels(*good, p, 1 << 30, None, None) < 0 and b"output" in err()
        i64[at] = keep
    assert lib.gan_jpegdec_pixels(*good, None, 1 << 30, None, None) < 0 and b"null" in err()
    assert lib.gan_jpegdec_pixels(*good, p, 100, None, None) < 0 and b"output" in err()
