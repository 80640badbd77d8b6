"""The submission archive off the GPU: tests.zip_ref (CRC-32 from its definition, with the combine identity) against zlib on the case
table, `inference.ZipWriter` against live zipfile byte for byte, `JpegEncoder.encode_block`, `stylize_folder(zip_path=...)` and both
command lines on the emulator, the argument checks of the C entry points (they fail in validation: no launch), and csrc/crc32_core.h
as a host program under AddressSanitizer and UBSan."""
import ctypes as C
import io
import json
import os
import shutil
import subprocess
import zipfile
import zlib

import numpy as np
import pytest
import torch

from gan_variant_research_amd import _lib, autograd as AG, cut, dataio, inference as I
from tests import jpeg_cases as JC, zip_cases as ZC, zip_ref as ZR
from tests.emulator_jpeg import EmuInputPipeline
from tests.emulator_zip import ZipEmuOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATE = (1980, 1, 1, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ the reference CRC
def test_ref_equals_zlib_on_the_case_table():
    buf, off, ids, want = ZC.table()
    assert len(ids) == 3 * len(ZC.LENGTHS) and want[0] == 0                      # an empty range gives 0
    for i, name in enumerate(ids):
        data = buf[off[i]:off[i + 1]].tobytes()
        assert ZR.crc(data) == int(want[i]), name
    assert ZR.crc_bitwise(b"123456789") == 0xCBF43926 == zlib.crc32(b"123456789")


def test_ref_combine_identity_on_random_splits():
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    for _ in range(20):
        lo, hi = sorted(int(v) for v in rng.integers(0, 3001, 2))
        mid = int(rng.integers(lo, hi + 1))
        assert ZR.combine(zlib.crc32(data[lo:mid]), zlib.crc32(data[mid:hi]), hi - mid) == zlib.crc32(data[lo:hi])
    assert ZR.x_to(0) == 1 << 31 and ZR.x_to(1) == 1 << 30 and ZR.x_to(32) == ZR.P and ZR.x_to(2 ** 32 - 1) == 1 << 31


# ------------------------------------------------------------------------------------------------ ZipWriter against zipfile
def _zipfile_bytes(entries, date_time=DATE) -> bytes:
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name, data in entries:
            z.writestr(zipfile.ZipInfo(name, date_time=date_time), data)
    return buf.getvalue()


def _blob(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


ARCHIVES = {
    "empty": [],
    "one-empty-entry": [("nothing.jpg", b"")],
    "nested": [("a.jpg", _blob(10, 1)), ("sub/b.jpg", _blob(11, 2)), ("sub/deeper/still/c.jpg", _blob(12, 3))],
    "non-ascii": [("héron/水.jpg", _blob(40, 4)), ("plain.jpg", _blob(7, 5))],
    "sizes": [("one.jpg", _blob(1, 6)), ("k.jpg", _blob(1001, 7)), ("2k.jpg", _blob(2001, 8))],
}


def _check_archive(path, entries, date_time=DATE):
    got = open(path, "rb").read()
    assert got == _zipfile_bytes(entries, date_time)
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
        assert [i.filename for i in z.infolist()] == [n for n, _ in entries]
        assert all(z.read(n) == d for n, d in entries)
        assert all(i.compress_type == zipfile.ZIP_STORED and i.extract_version == 20 and i.external_attr == 0o600 << 16 and not i.flag_bits & 8
                   and bool(i.flag_bits & 0x800) == (not i.filename.isascii()) for i in z.infolist())
    assert not os.path.exists(str(path) + ".part")


@pytest.mark.parametrize("how", ["add", "add-with-crc", "add_block", "add_block-host-crc"])
@pytest.mark.parametrize("name", list(ARCHIVES))
def test_writer_equals_zipfile(tmp_path, name, how):
    entries, path = ARCHIVES[name], tmp_path / "images.zip"
    with I.ZipWriter(path) as zw:
        assert not path.exists() and os.path.exists(str(path) + ".part")         # nothing at `path` before a clean close
        if how.startswith("add_block"):
            block = b"".join(d for _, d in entries)
            off = np.concatenate([[0], np.cumsum([len(d) for _, d in entries])]).astype(int).tolist()
            zw.add_block([n for n, _ in entries], memoryview(block), off, [zlib.crc32(d) for _, d in entries] if how == "add_block" else None)
        else:
            for n, d in entries:
                zw.add(n, d, zlib.crc32(d) if how == "add-with-crc" else None)
        assert len(zw) == len(entries)
    _check_archive(path, entries)


def test_writer_takes_the_crc_it_is_given_and_the_date(tmp_path):
    path = tmp_path / "z.zip"
    with I.ZipWriter(path, date_time=(2024, 2, 29, 23, 59, 58)) as zw:
        zw.add("a.bin", np.arange(5, dtype=np.uint8))                            # any bytes-like object
        zw.add_block(["b.bin"], b"xyz", [0, 3], [zlib.crc32(b"xyz")])
    _check_archive(path, [("a.bin", bytes(range(5))), ("b.bin", b"xyz")], (2024, 2, 29, 23, 59, 58))
    with I.ZipWriter(path) as zw:                                                 # a wrong CRC is written as given: zipfile finds it
        zw.add("a.bin", b"abc", crc=123)
    with zipfile.ZipFile(path) as z:
        assert z.testzip() == "a.bin"
    zw.close()                                                                    # a second close does nothing
    with pytest.raises(ValueError, match="closed"):
        zw.add("late.bin", b"")
    with pytest.raises(ValueError, match="date_time"):
        I.ZipWriter(tmp_path / "old.zip", date_time=(1979, 12, 31, 0, 0, 0))
    assert not (tmp_path / "old.zip").exists() and not (tmp_path / "old.zip.part").exists()


def test_writer_refusals_with_lowered_limits(tmp_path):
    class Small(I.ZipWriter):
        MAX_ENTRIES = 3
        MAX_BYTES = 1000

    assert (I.ZipWriter.MAX_ENTRIES, I.ZipWriter.MAX_BYTES) == (65535, 1 << 32)
    path = tmp_path / "s.zip"
    with pytest.raises(ValueError, match="already"):
        with Small(path) as zw:
            zw.add("a", b"1")
            zw.add("a", b"2")
    assert not path.exists() and not (tmp_path / "s.zip.part").exists()
    with pytest.raises(ValueError, match="entries"):
        with Small(path) as zw:
            for i in range(4):
                zw.add(f"f{i}", b"")
    with pytest.raises(ValueError, match="ZIP64"):                                # a size at the limit
        with Small(path) as zw:
            zw.add("big", bytes(1000))
    with pytest.raises(ValueError, match="ZIP64"):                                # an offset at the limit: the second entry would start past it
        with Small(path) as zw:
            zw.add("a", bytes(600))
            zw.add("b", bytes(600))
    with pytest.raises(ValueError, match="ZIP64"):                                # the central directory would end past it
        with Small(path) as zw:
            zw.add("a" * 40, bytes(880))
    with pytest.raises(ValueError, match="offsets"):
        with Small(path) as zw:
            zw.add_block(["a", "b"], b"abcdef", [0, 4, 3], [0, 0])
    with pytest.raises(ValueError, match="names"):
        with Small(path) as zw:
            zw.add_block(["a", "b"], b"abcdef", [0, 4], [0, 0])
    assert not path.exists() and not (tmp_path / "s.zip.part").exists()
    with Small(path) as zw:                                                       # inside the limits it is an archive like any other
        for i in range(3):
            zw.add(f"f{i}", bytes(100))
    _check_archive(path, [(f"f{i}", bytes(100)) for i in range(3)])


def test_exception_inside_with_leaves_nothing(tmp_path):
    path = tmp_path / "x.zip"
    with pytest.raises(RuntimeError, match="stop"):
        with I.ZipWriter(path) as zw:
            zw.add("a.jpg", b"abc")
            raise RuntimeError("stop")
    assert list(tmp_path.iterdir()) == []


# ------------------------------------------------------------------------------------------------ encode_block on the emulator
@pytest.mark.parametrize("name,q", [("pixel", 95), ("ragged", 95), ("batch", 95), ("const", 95), ("runs", 1)])
def test_encode_block_on_the_emulator(name, q):
    (B, H, W), _ = JC.CASES[name]
    enc = I.JpegEncoder("cpu", B + 1, H, W, quality=q, ops=ZipEmuOps())
    x = torch.from_numpy(JC.rgb(name))
    block, off, crcs = enc.encode_block(x)
    files = JC.golden(name, q)
    assert off[0] == 0 and off[B] == len(block) and len(off) == B + 1 and len(crcs) == B
    assert [bytes(block[off[b]:off[b + 1]]) for b in range(B)] == files == enc.encode(x)
    assert crcs == [zlib.crc32(f) for f in files]
    block1, off1, crcs1 = enc.encode_block(x[:1])                                 # a smaller batch through the same buffers
    assert bytes(block1) == files[0] and off1 == [0, len(files[0])] and crcs1 == crcs[:1]
    with pytest.raises(ValueError):
        enc.encode_block(torch.zeros(B + 2, H, W, 3, dtype=torch.uint8))


def test_encode_block_raises_on_a_set_flag():
    class Short(ZipEmuOps):
        def jpeg_files_bounds(self, *a, **kw):
            return 100                                                            # no file fits: the stand-in sets bit 1, as the kernel does

    enc = I.JpegEncoder("cpu", 1, 8, 8, ops=Short())
    with pytest.raises(_lib.GanError, match="flag = 2"):
        enc.encode_block(torch.from_numpy(JC.rgb("mcu")))


# ------------------------------------------------------------------------------------------------ the folder path and the command lines
@pytest.fixture
def folder(monkeypatch, tmp_path):
    from PIL import Image
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: ZipEmuOps())
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


def _entries(path):
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
        return [(i.filename, z.read(i)) for i in z.infolist()]


def test_stylize_folder_zip_on_the_emulator(folder):
    G, photos, tmp = folder
    run = lambda **kw: I.stylize_folder(G, str(photos), device="cpu", img_size=24, batch=2, **kw)
    assert run(out_dir=str(tmp / "dir"), device_io=True, device_jpeg=True) == 5
    want = _files(tmp / "dir")
    order = ["a.jpg", "d.jpg", "e.jpg", "sub/b.jpg", "sub/c.jpg"]                 # the order of the sorted source paths
    assert sorted(want) == order
    calls = []
    real_block, real_encode = I.JpegEncoder.encode_block, I.JpegEncoder.encode
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(I.JpegEncoder, "encode_block", lambda self, y: calls.append("block") or real_block(self, y))
        mp.setattr(I.JpegEncoder, "encode", lambda self, y: calls.append("files") or real_encode(self, y))
        mp.setattr(I.ZipWriter, "add", lambda *a, **kw: pytest.fail("the device route adds whole blocks, with the device's CRCs"))
        assert run(zip_path=str(tmp / "dev.zip"), device_io=True, device_jpeg=True) == 5
    assert calls == ["block"] * 3                                                 # batches of 2, 2, 1; no per-file assembly
    got = _entries(tmp / "dev.zip")
    assert [n for n, _ in got] == order and dict(got) == want
    archive = (tmp / "dev.zip").read_bytes()
    assert archive == _zipfile_bytes([(n, want[n]) for n in order])
    assert run(zip_path=str(tmp / "pil.zip"), device_io=True) == 5 and (tmp / "pil.zip").read_bytes() == archive          # PIL into memory
    assert run(zip_path=str(tmp / "host.zip")) == 5 and (tmp / "host.zip").read_bytes() == archive
    assert run(zip_path=str(tmp / "pool.zip"), device_io=True, io_threads=4) == 5 and (tmp / "pool.zip").read_bytes() == archive
    for tag, kw in (("both", dict(device_io=True, device_jpeg=True)), ("both-pil", dict(device_io=True, io_threads=4))):
        assert run(out_dir=str(tmp / tag), zip_path=str(tmp / f"{tag}.zip"), **kw) == 5
        assert _files(tmp / tag) == want and (tmp / f"{tag}.zip").read_bytes() == archive
    with pytest.raises(ValueError, match="out_dir"):
        run(device_io=True)
    assert not any(p.name.endswith(".part") for p in tmp.iterdir())


def test_stylize_folder_failure_leaves_no_archive(folder):
    G, photos, tmp = folder
    (photos / "a.jpg").write_bytes((photos / "d.jpg").read_bytes())              # a.png and a.jpg both become a.jpg
    with pytest.raises(ValueError, match="already"):
        I.stylize_folder(G, str(photos), device="cpu", img_size=24, batch=2, device_io=True, zip_path=str(tmp / "dup.zip"))
    assert not (tmp / "dup.zip").exists() and not (tmp / "dup.zip.part").exists()


def test_generate_folder_zip_flag(folder, monkeypatch, capsys):
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
    assert GF.main(base + ["--zip", str(tmp / "only.zip"), "--device-jpeg"]) == 5
    assert GF.main(base + ["--zip", str(tmp / "both.zip"), "--out", str(tmp / "both")]) == 5
    assert [(k.get("out_dir"), k.get("zip_path"), k["device_jpeg"]) for k in seen] == [
        (str(tmp / "plain"), None, False), (None, str(tmp / "only.zip"), True), (str(tmp / "both"), str(tmp / "both.zip"), False)]
    assert "zip_path" not in seen[0]                                              # without the flag the call is what it was
    want = _files(tmp / "plain")
    assert dict(_entries(tmp / "only.zip")) == want == _files(tmp / "both") and (tmp / "both.zip").read_bytes() == (tmp / "only.zip").read_bytes()
    assert f"-> '{tmp / 'only.zip'}'" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        GF.parse_args(["--ckpt", "c", "--photos", "p"])                           # neither --out nor --zip
    assert "--out and --zip" in capsys.readouterr().err
    a = GF.parse_args(["--ckpt", "c", "--photos", "p", "--zip", "z"])
    assert (a.out, a.zip) == (None, "z")


def test_select_7k_zip_from_feature_files(tmp_path, capsys):
    """Two candidate roots that share file names: the archive holds what OUT/images holds (the last candidate of a name), sorted by
    name, with and without the copy."""
    from PIL import Image
    from gan_variant_research_amd import select_7k as S
    from tests.emulator_select import SelectEmuOps
    mp = pytest.MonkeyPatch()
    mp.setattr(AG, "_OPS_FACTORY", lambda device: SelectEmuOps())
    try:
        a, b = tmp_path / "cand_a", tmp_path / "cand_b"
        rng = np.random.default_rng(8)
        for d, names in ((a, [f"img_{i}.png" for i in range(6)]), (b, [f"img_{i}.png" for i in range(3)] + ["x.png", "y.png", "z.png"])):
            d.mkdir()
            for n in names:
                Image.fromarray(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)).save(d / n)
        for n, rows in (("real", 9), ("a", 6), ("b", 6)):
            np.save(tmp_path / f"{n}.npy", rng.standard_normal((rows, 16)).astype(np.float32))
        common = ["--cand_roots", str(a), str(b), "--real-features", str(tmp_path / "real.npy"), "--cand-features", str(tmp_path / "a.npy"),
                  str(tmp_path / "b.npy"), "--tau", "0.0", "--k", "2", "--target", "12", "--device", "cpu"]
        out = tmp_path / "out"
        assert S.main([*common, "--outdir", str(out), "--zip", str(tmp_path / "images.zip")]) == 0
        held = _files(out / "images")
        assert len(held) == 9                                                     # 12 selected, three names twice
        got = _entries(tmp_path / "images.zip")
        assert [n for n, _ in got] == sorted(held) and dict(got) == held
        assert (tmp_path / "images.zip").read_bytes() == _zipfile_bytes(sorted(held.items()))
        meta = json.load(open(out / "selection_meta.json"))
        assert meta["zip"] == str(tmp_path / "images.zip") and meta["zip_entries"] == 9 and meta["collisions"] == 3
        dry = tmp_path / "dry"
        assert S.main([*common, "--outdir", str(dry), "--no-copy", "--zip", str(tmp_path / "dry.zip")]) == 0
        assert not (dry / "images").exists() and (tmp_path / "dry.zip").read_bytes() == (tmp_path / "images.zip").read_bytes()
        assert f"into {tmp_path / 'dry.zip'}" in capsys.readouterr().out
        plain = tmp_path / "plain"
        assert S.main([*common, "--outdir", str(plain)]) == 0                     # without the flag the meta file has no new keys
        assert "zip" not in json.load(open(plain / "selection_meta.json"))
    finally:
        mp.undo()


# ------------------------------------------------------------------------------------------------ the C side
def test_entry_points_validate_before_they_launch():
    lib = _lib.load()
    err = lambda: lib.gan_last_error()
    p = 1 << 20                                                                   # aligned, never dereferenced: validation fails first
    for args in ((None, 10, p, 1, p, p), (p, 10, None, 1, p, p), (p, 10, p, 1, None, p), (p, 10, p, 1, p, None)):
        assert lib.gan_crc32_ranges(*args, None) < 0 and b"null" in err()
    assert lib.gan_crc32_ranges(p, 10, p, -1, p, p, None) < 0 and b"n=-1" in err()
    assert lib.gan_crc32_ranges(p, -1, p, 1, p, p, None) < 0 and b"negative" in err()
    assert lib.gan_crc32_ranges(p, 10, p, 0, p, p, None) == 0                     # no range: success, nothing launched
    out, ws, scan = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert lib.gan_jpeg_bounds(16, 256, 256, C.byref(ws), C.byref(scan)) == 0
    assert lib.gan_jpeg_files_bounds(16, 256, 256, 177, 14, C.byref(out)) == 0
    assert out.value == scan.value + 16 * (177 + 4 * (5 + 16 + 256) + 14 + 2)
    assert lib.gan_jpeg_files_bounds(16, 256, 256, 177, 14, None) < 0 and b"null" in err()
    assert lib.gan_jpeg_files_bounds(0, 256, 256, 177, 14, C.byref(out)) < 0 and b"65535" in err()
    assert lib.gan_jpeg_files_bounds(1, 0, 256, 177, 14, C.byref(out)) < 0 and b"65535" in err()
    assert lib.gan_jpeg_files_bounds(1, 16384, 16384, 177, 14, C.byref(out)) < 0 and b"32-bit" in err()
    assert lib.gan_jpeg_files_bounds(1, 8, 8, 1, 14, C.byref(out)) < 0 and b"head" in err()
    assert lib.gan_jpeg_files_bounds(1, 8, 8, 177, 70000, C.byref(out)) < 0 and b"SOS" in err()
    good = [p, 177, p, 14, p, p, 1000, p, 2, p, 5000, p, p, p]
    assert len(good) == 14
    for i in (0, 2, 4, 5, 7, 9, 11, 12, 13):
        args = list(good)
        args[i] = None
        assert lib.gan_jpeg_files(*args, None) < 0 and b"null" in err(), i
    for i, v, word in ((8, 0, b"65535"), (8, 65536, b"65535"), (1, 0, b"head"), (3, 1, b"SOS"), (6, -1, b"negative"), (10, -5, b"negative")):
        args = list(good)
        args[i] = v
        assert lib.gan_jpeg_files(*args, None) < 0 and word in err(), (i, v)


def test_hipops_bounds_is_the_emulators():
    from gan_variant_research_amd.runtime import HipOps
    ops = HipOps(torch.device("cpu"))                                             # no launch is built or run: a host query
    for B, H, W, head in ((16, 256, 256, 177), (1, 1, 1, 177), (3, 9, 33, 200)):
        assert ops.jpeg_files_bounds(B, H, W, head) == ZipEmuOps().jpeg_files_bounds(B, H, W, head)
    with pytest.raises(_lib.GanError):
        ops.jpeg_files_bounds(0, 8, 8, 177)


def test_crc32_host_program_under_sanitizers(tmp_path):
    cxx = os.environ.get("HOSTCXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler (c++, g++ or clang++) or no make on this machine: the sanitizer build of csrc/crc32_host.cpp cannot be made")
    exe = tmp_path / "crc32_host"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gan-variant-research_amd", "csrc"), "crc32_host", f"HOSTCXX={cxx}", f"CRCHOSTBIN={exe}"],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip(f"{cxx} has no AddressSanitizer / UBSan runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stdout + r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]                   # a sanitizer report ends the program with a non-zero status
    assert "agrees" in run.stdout
