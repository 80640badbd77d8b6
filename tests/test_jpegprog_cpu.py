"""The progressive JPEG decoder off the GPU: tests.jpegprog_ref (the statement csrc/jpegprog.hip is held to) against the golden pixels and
Pillow itself, with the paths the cases must reach; the parser's accepted class and its dependency indices; the entropy stage
(csrc/jpegprog_core.h, the text the kernel compiles) as a host program under AddressSanitizer / UBSan over every case, the flagged files
and seeded corruptions; dataio.JpegDecoder(progressive=True), ImageStore, the trainers' config key, stylize_folder and the command
lines on the emulator."""
import hashlib
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gan_variant_research_amd import _lib, autograd as AG, cut, dataio, inference as I
from tests import jpegdec_cases as DC, jpegprog_cases as PC, jpegprog_ref as P
from tests.emulator_jpeg import EmuInputPipeline
from tests.emulator_jpegprog import JpegProgEmuOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASELINE = {"base.a": "ragged.9x33.420", "base.b": "rst", "png": "png"}         # the mixed call's files from the baseline decoder's golden data


def source(name: str) -> bytes:
    return DC.file(BASELINE[name]) if name in BASELINE else PC.file(name)


def expected(name: str) -> np.ndarray:
    return DC.pixels(BASELINE[name]) if name in BASELINE else PC.pixels(name)


def equals_golden(name, px) -> bool:
    return tuple(px.shape) == PC.shape(name) + (3,) and hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest() == PC.pixels_sha256(name)


@pytest.fixture(scope="module")
def ref_runs():
    """name -> (stages, counters) of the reference over every case, computed once."""
    out = {}
    for name in PC.ALL:
        cnt = {}
        out[name] = (P.stages(PC.file(name), cnt), cnt)
    return out


def test_ref_equals_golden_and_live_pillow(ref_runs):
    from PIL import features
    differs = []
    for name, (st, _) in ref_runs.items():
        assert equals_golden(name, st.pixels) and not st.extreme, name
        if not equals_golden(name, P.pillow_pixels(PC.file(name))):
            differs.append(name)
    if differs:
        pytest.skip(f"the reference equals the golden pixels; live Pillow (libjpeg {features.version('jpg')}) differs from them for {differs}, comparison with it skipped")


def test_cases_reach_every_path(ref_runs):
    total = {k: sum(c[k] for _, c in ref_runs.values()) for k in P.COUNTERS}
    assert all(v > 0 for v in total.values()), total
    c = lambda n: ref_runs[n][1]
    assert c("const.gray")["eobrun_across_blocks"] >= 1 and c("rst")["eobrun_cut_by_restart"] >= 1 and c("runs")["zrl_refine"] >= 1
    assert c("ragged.9x33.420")["grid_narrower"] and c("ragged.17x15.420")["grid_shorter"]
    gray = P.parse(PC.file("const.gray"))
    assert gray.mcux * gray.mcuy == 1024
    assert any(b"\xff\x00" in PC.file("stuffing")[b:e] for b, e in PC.scan_ranges(PC.file("stuffing")))
    rst = P.parse(PC.file("rst"))
    assert {(sc.comp < 0, sc.per) for sc in rst.scans} == {(True, 3), (False, 3)} and len(rst.scans[0].segments) == 4 and len(rst.scans[1].segments) == 12
    assert all(len(sc.segments) == 64 for sc in P.parse(PC.file("rst_wrap")).scans)
    assert len({sc.per for sc in P.parse(PC.file("dri_change")).scans}) > 2
    assert [sc.comp for sc in P.parse(PC.file("dc_split")).scans[:3]] == [0, 1, 2]
    assert max(sc.Al for sc in P.parse(PC.file("deep")).scans) == 3
    t20 = dataio.parse_jpeg_progressive(PC.file("tables20"))      # table versions on both sides of the 16 the device keeps on chip, side by side on each level
    assert len(t20["versions"]) == 25 and t20["nlevel"] == 2
    for level in (0, 1):
        used = [max(s["tab"]) for s in t20["scans"] if s["level"] == level]
        assert min(used) < 16 <= max(used), (level, used)


# ------------------------------------------------------------------------------------------------ the parser
PILLOW_CHAINS = {3: [(-1, 0), (-1, 0), (-1, 0), (-1, 0), (-1, 0), (4, 1), (0, 1), (2, 1), (3, 1), (5, 2)], 1: [(-1, 0), (-1, 0), (-1, 0), (2, 1), (0, 1), (3, 2)]}


def test_parser_accepts_every_case_and_states_the_dependencies():
    for name in PC.ALL + list(PC.FLAGGED):
        data = PC.file(name)
        plan, p = dataio.parse_jpeg_progressive(data), P.parse(data)
        assert plan is not None and dataio.parse_jpeg(data) is None, name
        assert (plan["H"], plan["W"], plan["ncomp"], plan["hmax"], plan["vmax"], plan["mcux"], plan["mcuy"]) == (p.H, p.W, len(p.comps), p.hmax, p.vmax, p.mcux, p.mcuy)
        assert len(plan["scans"]) == len(p.scans) <= dataio.PROG_MAX_SCANS and len(plan["versions"]) <= dataio.PROG_MAX_TABLES
        for a, b in zip(plan["scans"], p.scans):
            assert (a["comp"], a["Ss"], a["Se"], a["Ah"], a["Al"], a["per"], a["units"]) == (b.comp, b.Ss, b.Se, b.Ah, b.Al, b.per, b.units), name
            assert list(zip(a["seg_begin"].tolist(), a["seg_end"].tolist())) == b.segments, name
            for c, t in b.tables.items():
                assert list(plan["versions"][a["tab"][c]]) == t[0] + t[1], name
        if name in PC.CASES:                                  # Pillow's own script: the chains DC, Y-AC (two bands side by side), Cb-AC, Cr-AC
            assert [(s["dep"], s["level"]) for s in plan["scans"]] == PILLOW_CHAINS[plan["ncomp"]], name
    order = dataio.parse_jpeg_progressive(PC.file("order"))
    assert [(s["comp"], s["dep"], s["level"]) for s in order["scans"]] == [(-1, -1, 0), (1, -1, 0), (2, -1, 0), (0, -1, 0), (2, 2, 1), (1, 1, 1), (0, 3, 1)]
    deep = dataio.parse_jpeg_progressive(PC.file("deep"))
    assert deep["nlevel"] == 4 and [s["dep"] for s in deep["scans"][4:7]] == [0, 4, 5]


def test_parser_refuses_the_fallback_files_and_baseline():
    for name in PC.FALLBACK:
        assert dataio.parse_jpeg_progressive(PC.file(name)) is None and dataio.parse_jpeg(PC.file(name)) is None, name
    for name in list(DC.CASES) + ["cmyk", "s411", "adobe", "png", "crafted", "corrupt"]:
        assert dataio.parse_jpeg_progressive(DC.file(name)) is None, name
    base = PC.file("mcu.420")
    eoi = base.rindex(b"\xff\xd9")
    sos = [i for i in range(len(base) - 1) if base[i] == 0xFF and base[i + 1] == 0xDA]
    refused = {
        "no EOI": base[:eoi], "empty": b"", "SOI only": b"\xff\xd8", "12-bit": base.replace(b"\xff\xc2\x00\x11\x08", b"\xff\xc2\x00\x11\x0c", 1),
        "a DQT between scans": base[:sos[1]] + b"\xff\xdb\x00\x43\x00" + bytes([1] * 64) + base[sos[1]:],
        "fill bytes": base[:eoi] + b"\xff" + base[eoi:], "an unknown marker": base[:2] + b"\xff\xf7\x00\x02" + base[2:],
        "a restart marker the interval does not ask": base[:eoi] + b"\xff\xd0" + base[eoi:],
        "the last scan missing": base[:sos[-1]] + base[eoi:],
    }
    for what, data in refused.items():
        assert dataio.parse_jpeg_progressive(data) is None, what
    for data in (base[:2] + b"\xff\xfe\x00\x05abc" + base[2:], base[:sos[2]] + b"\xff\xe1\x00\x08Exif\x00\x00" + base[sos[2]:], base + b"trailing"):
        assert dataio.parse_jpeg_progressive(data) is not None and np.array_equal(P.decode(data), PC.pixels("mcu.420"))


# ------------------------------------------------------------------------------------------------ the arithmetic under sanitizers
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("HOSTCXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler (c++, g++ or clang++) or no make on this machine: the sanitizer build of csrc/jpegprog_host.cpp cannot be made")
    exe = tmp_path_factory.mktemp("jpegprog_host") / "jpegprog_host"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gan-variant-research_amd", "csrc"), "jpegprog_host", f"HOSTCXX={cxx}", f"PROGHOSTBIN={exe}"],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip(f"{cxx} has no AddressSanitizer / UBSan runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


def run_host(exe, files, tmp_path):
    """The files (all accepted by the parser) through the host program -> (error words, pixel arrays)."""
    prog = dataio.JpegDecoder("cpu", ops=JpegProgEmuOps(), progressive=True)._prog
    plans = [dataio.parse_jpeg_progressive(f) for f in files]
    offs, end = [], 0
    for p in plans:
        offs.append(end)
        end += p["H"] * p["W"] * 3
    total, n, nscan, nseg, nver, ws = prog._pack(plans, offs)
    o = prog.ops.jpegprog_block_offsets(n, nscan, nseg, nver)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(np.array([total, n, nscan, nseg, nver, ws, end, *o[:5]], np.int64).tobytes() + prog._host[:total].numpy().tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]                 # a sanitizer report ends the program with a non-zero status
    raw = np.fromfile(dst, np.uint8)
    return raw[:4 * n].view(np.int32).tolist(), [raw[4 * n + o:][:p["H"] * p["W"] * 3].reshape(p["H"], p["W"], 3) for o, p in zip(offs, plans)]


expectation = P.expectation          # (error word, pixels) by tests.jpegprog_ref


def test_host_program_under_sanitizers(host_program, tmp_path):
    """Every case, the flagged files, then 200 seeded corruptions of each of three cases: no sanitizer report, and the pixels or the error
    word the reference expects.  Where the reference's word is 0 on a corrupted file, its pixels are Pillow's: nothing libjpeg warns about
    goes unflagged.  The GPU tests decode the flagged files only after this."""
    err, px = run_host(host_program, [PC.file(n) for n in PC.ALL], tmp_path)
    assert err == [0] * len(PC.ALL)
    for n, p in zip(PC.ALL, px):
        assert equals_golden(n, p), n
    err, px = run_host(host_program, [PC.file(n) for n in PC.FLAGGED], tmp_path)
    for (n, word), e in zip(PC.FLAGGED.items(), err):
        assert e == (expectation(PC.file(n))[0] if word is None else word) and e != 0, (n, e)
    assert PC.corrupted(PC.file("rst"), PC.corrupt_seed()) == PC.file("corrupt")
    variants = [PC.corrupted(PC.file(n), 1000 + s) for n in ("rst", "runs", "ragged.17x15.420") for s in range(200)]
    taken = [v for v in variants if dataio.parse_jpeg_progressive(v) is not None]
    assert len(taken) >= len(variants) // 2
    want = [expectation(v) for v in taken]
    err, px = run_host(host_program, taken, tmp_path)
    clean = 0
    for i, ((word, pixels), e, p, v) in enumerate(zip(want, err, px, taken)):
        assert e == word, (i, e, word)
        if not word:
            clean += 1
            assert np.array_equal(p, pixels) and np.array_equal(pixels, P.pillow_pixels(v)), i
    assert clean >= 1 and len(taken) - clean >= len(taken) // 2


# ------------------------------------------------------------------------------------------------ JpegDecoder on the emulator
def mixed_call(dec):
    """The mixed call into a caller's buffer with packed, unaligned offsets -> (images, buffer, offsets)."""
    sizes = [expected(n).size for n in PC.MIXED]
    offsets = [5 + sum(sizes[:i]) + 3 * i for i in range(len(sizes))]
    out = torch.full((offsets[-1] + sizes[-1] + 7,), 0xAB, dtype=torch.uint8, device=dec.device)
    return dec.decode([source(n) for n in PC.MIXED], out=out, offsets=offsets), out, offsets


def check_mixed(got, out, offsets):
    used = np.zeros(out.numel(), bool)
    for n, g, o in zip(PC.MIXED, got, offsets):
        assert np.array_equal(g.cpu().numpy(), expected(n)), n
        used[o:o + expected(n).size] = True
    assert (out.cpu().numpy()[~used] == 0xAB).all()


def test_mixed_call_on_the_emulator():
    dec = dataio.DeviceDecoder("cpu", ops=JpegProgEmuOps(), progressive=True)
    check_mixed(*mixed_call(dec))
    assert dec.stats == {"device": 6, "unsupported": 1, "flagged": 1}
    assert dec.jpeg.stats == {"device": 5, "unsupported": 1, "flagged": 1} and dec.progressive_stats == {"device": 3, "unsupported": 1, "flagged": 1}
    assert dec.last_errors == {PC.MIXED.index("corrupt"): expectation(PC.file("corrupt"))[0]}
    plain = dataio.DeviceDecoder("cpu", ops=JpegProgEmuOps())
    check_mixed(*mixed_call(plain))
    assert plain.stats == {"device": 3, "unsupported": 5, "flagged": 0} and plain.jpeg.stats == {"device": 2, "unsupported": 5, "flagged": 0}
    assert plain.progressive_stats == {"device": 0, "unsupported": 0, "flagged": 0}
    jd = dataio.JpegDecoder("cpu", ops=JpegProgEmuOps(), progressive=True)                  # the PNG is then one more file for Pillow
    check_mixed(*mixed_call(jd))
    assert jd.stats == {"device": 5, "unsupported": 2, "flagged": 1} and jd.progressive_stats == {"device": 3, "unsupported": 1, "flagged": 1}
    names = PC.PIXEL_CASES
    for n, g in zip(names, jd.decode([PC.file(n) for n in names])):
        assert np.array_equal(g.numpy(), PC.pixels(n)), n
    for n, g in zip(PC.FLAGGED, jd.decode([PC.file(n) for n in PC.FLAGGED])):
        assert np.array_equal(g.numpy(), PC.pixels(n)), n
    assert len(jd.last_errors) == 4 and all(jd.last_errors[i] == (w or jd.last_errors[i]) for i, w in enumerate(PC.FLAGGED.values()))
    for n in PC.FALLBACK:
        if PC.raises(n):
            with pytest.raises(OSError):
                jd.decode([PC.file(n)])
        else:
            assert np.array_equal(jd.decode([PC.file(n)])[0].numpy(), PC.pixels(n)), n


def test_truncated_file_raises_what_the_pillow_path_raises(tmp_path):
    p = tmp_path / "cut.jpg"
    p.write_bytes(PC.file("truncated"))
    with pytest.raises(OSError) as plain:
        dataio._decode(p)
    dec = dataio.JpegDecoder("cpu", ops=JpegProgEmuOps(), progressive=True)
    with pytest.raises(OSError) as mine:
        dec.decode([PC.file("gray"), p])
    assert str(mine.value) == str(plain.value) and str(p) in str(mine.value)


# ------------------------------------------------------------------------------------------------ the store, the folder path, the command lines
@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: JpegProgEmuOps())
    monkeypatch.setattr(dataio, "InputPipeline", EmuInputPipeline)


def _write_folder(root, names):
    root.mkdir(parents=True, exist_ok=True)
    paths = []
    for n in names:
        paths.append(root / (n.replace(".", "_") + (".png" if n == "png" else ".jpg")))
        paths[-1].write_bytes(source(n))
    return paths


@pytest.mark.parametrize("budget", [None, 0], ids=["resident", "streaming"])
@pytest.mark.parametrize("png", [False, True], ids=["jpeg", "jpeg+png"])
def test_image_store_device_progressive_holds_the_same_bytes(emulated, tmp_path, monkeypatch, budget, png):
    paths = _write_folder(tmp_path / "imgs", PC.MIXED)
    monkeypatch.setattr(dataio, "DECODE_CHUNK", 3)
    plain = dataio.ImageStore(paths, "cpu", budget_bytes=budget, workers=2)
    store = dataio.ImageStore(paths, "cpu", budget_bytes=budget, workers=2, device_decode=True, device_png=png, device_progressive=True)
    for i, n in enumerate(PC.MIXED):
        assert np.array_equal(store[i].numpy(), expected(n)) and torch.equal(store[i], plain[i]), n
    for a, b in zip(store.fetch([7, 1, 1, 4]), plain.fetch([7, 1, 1, 4])):
        assert torch.equal(a, b)
    if budget is None:
        assert store._decoder.stats == {"device": 5 + png, "unsupported": 2 - png, "flagged": 1}
        assert store._decoder.progressive_stats == {"device": 3, "unsupported": 1, "flagged": 1}
    with pytest.raises(ValueError, match="device_decode"):
        dataio.ImageStore(paths, "cpu", device_progressive=True)
    store.close(), plain.close()


def test_trainers_pass_the_config_key_to_their_stores(emulated, tmp_path):
    from gan_variant_research_amd import train_basic, train_cutpp
    assert train_basic.build_store is train_cutpp.build_store                  # both trainers build their stores, and read the key, here
    paths = _write_folder(tmp_path / "imgs", ["gray", "base.a", "dc_split"])
    off = train_cutpp.build_store(paths, "cpu", {"mi355x": {"device_decode": True}}, "A", quiet=True)
    on = train_cutpp.build_store(paths, "cpu", {"mi355x": {"device_decode": True, "device_progressive": True}}, "A", quiet=True)
    assert off._decoder.stats == {"device": 1, "unsupported": 2, "flagged": 0} and on._decoder.stats == {"device": 3, "unsupported": 0, "flagged": 0}
    assert on._decoder.progressive_stats["device"] == 2 and all(torch.equal(on[i], off[i]) for i in range(3))
    with pytest.raises(ValueError, match="device_decode"):
        train_cutpp.build_store(paths, "cpu", {"mi355x": {"device_progressive": True}}, "A", quiet=True)


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
    for name, (h, w), prog in (("a.jpg", (20, 24), False), ("sub/b.jpg", (33, 17), True), ("sub/c.jpg", (24, 24), True), ("d.jpg", (40, 31), False), ("e.jpg", (9, 50), True)):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(photos / name, quality=90, progressive=prog)
    Image.fromarray(rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)).save(photos / "f.png")
    (photos / "g.jpg").write_bytes(PC.file("s411"))
    return G, photos, tmp_path


def _files(root):
    return {p.relative_to(root).as_posix(): p.read_bytes() for p in root.rglob("*") if p.is_file()}


def test_stylize_folder_device_progressive_on_the_emulator(folder):
    G, photos, tmp = folder
    run = lambda out, **kw: I.stylize_folder(G, str(photos), str(tmp / out), device="cpu", img_size=24, batch=2, device_io=True, **kw)
    assert run("pil") == 7
    want = _files(tmp / "pil")
    assert run("dec", device_decode=True) == 7 and _files(tmp / "dec") == want
    assert G._jpeg_dec.stats == {"device": 2, "unsupported": 5, "flagged": 0}
    assert run("prog", device_decode=True, device_progressive=True, decode_chunk=3) == 7 and _files(tmp / "prog") == want
    assert G._jpeg_dec.stats == {"device": 5, "unsupported": 2, "flagged": 0} and G._jpeg_dec.progressive_stats == {"device": 3, "unsupported": 1, "flagged": 0}
    with pytest.raises(ValueError, match="device_decode"):
        run("bad", device_progressive=True)


def test_command_line_flags(folder, monkeypatch, capsys):
    from gan_variant_research_amd import evaluate as EV, generate_folder as GF, select_7k as SK
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
    assert GF.main(base + ["--out", str(tmp / "dec"), "--device-decode"]) == 7
    assert GF.main(base + ["--out", str(tmp / "prog"), "--device-decode", "--device-progressive"]) == 7
    assert "device_progressive" not in seen[0] and "device_progressive" not in seen[1] and seen[2]["device_progressive"] is True
    assert _files(tmp / "prog") == _files(tmp / "plain") and len(_files(tmp / "prog")) == 7
    a = GF.parse_args(["--ckpt", "c", "--photos", "p", "--out", "o"])
    assert a.device_progressive is False
    with pytest.raises(SystemExit):
        GF.parse_args(["--ckpt", "c", "--photos", "p", "--out", "o", "--device-progressive"])
    assert "--device-decode" in capsys.readouterr().err
    for mod in (EV, SK):                                       # the flag is accepted where --device-decode is, and needs it
        parser = mod.build_parser()
        flags = {s for act in parser._actions for s in act.option_strings}
        assert {"--device-decode", "--device-progressive"} <= flags, mod.__name__
        with pytest.raises(SystemExit):
            mod.main([a for a in ("--device-progressive",)] + ["--real", str(photos), "--fake", str(photos)] if mod is EV else ["--device-progressive"])
    assert "--device-progressive" in capsys.readouterr().err
