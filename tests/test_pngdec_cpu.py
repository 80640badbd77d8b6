"""The PNG decoder off the GPU: tests.pngdec_ref (the statement csrc/pngdec.hip is held to) against zlib, the golden pixels and Pillow
itself; the parser's accepted class; the decoder's arithmetic (csrc/pngdec_core.h, the text the kernels compile) as a host program
under AddressSanitizer / UBSan over every case and its corrupted variants; dataio.PngDecoder, DeviceDecoder, ImageStore(device_png=True),
stylize_folder(device_png=True) and the command lines on the emulator; the argument checks of the C entries (no launch)."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch

from gan_variant_research_amd import _lib, autograd as AG, cut, dataio, inference as I
from tests import jpegdec_cases as JC, pngdec_cases as PC, pngdec_ref as R
from tests.emulator_jpeg import EmuInputPipeline
from tests.emulator_pngdec import PngDecEmuOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def equals_golden(name, px) -> bool:
    return tuple(px.shape) == PC.shape(name) and hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest() == PC.pixels_sha256(name)


def blocks(stream: bytes):
    """The block types of a valid deflate stream, in order, with the bit position each starts at (counted in the deflate data)."""
    out, b = [], R._Bits(stream[2:-4])
    raw = zlib.decompress(stream)
    produced = 0
    while True:
        at = 8 * b.pos - b.n
        final, kind = b.take(1), b.take(2)
        out.append((kind, at))
        if kind == 0:
            b.take(b.n & 7)
            n = b.take(16)
            b.take(16)
            pos = b.pos - b.n // 8
            b.pos, b.buf, b.n, produced = pos + n, 0, 0, produced + n
        else:                                    # walk the block with the reference's own pieces
            sub = R._Bits(b.data)
            sub.pos, sub.buf, sub.n = b.pos, b.buf, b.n
            produced = _skip_block(sub, kind, produced)
            b.pos, b.buf, b.n = sub.pos, sub.buf, sub.n
        if final:
            assert produced == len(raw)
            return out


def _skip_block(b, kind, produced):
    if kind == 1:
        lit, dist = R._Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False), R._Code([5] * 32, False)
    else:
        hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
        cl = [0] * 19
        for k in range(hclen):
            cl[R.ORDER[k]] = b.take(3)
        cc, lens = R._Code(cl, True), []
        while len(lens) < hlit + hdist:
            s = b.symbol(cc)
            lens += [s] if s < 16 else [lens[-1]] * (3 + b.take(2)) if s == 16 else [0] * (3 + b.take(3)) if s == 17 else [0] * (11 + b.take(7))
        lit, dist = R._Code(lens[:hlit], False), R._Code(lens[hlit:], False)
    while True:
        s = b.symbol(lit)
        if s == 256:
            return produced
        if s < 256:
            produced += 1
            continue
        base, x = R.length_code(s)
        produced += base + b.take(x)
        base, x = R.distance_code(b.symbol(dist))
        b.take(x)


def code_length_symbols(stream: bytes):
    """HLIT and the code-length symbols [(symbol, first length it sets, how many)] of a stream whose first block is dynamic."""
    b = R._Bits(stream[2:-4])
    assert (b.take(1), b.take(2))[1] == 2
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    cl = [0] * 19
    for k in range(hclen):
        cl[R.ORDER[k]] = b.take(3)
    cc, have, out = R._Code(cl, True), 0, []
    while have < hlit + hdist:
        s = b.symbol(cc)
        rep = 1 if s < 16 else 3 + b.take(2) if s == 16 else 3 + b.take(3) if s == 17 else 11 + b.take(7)
        out.append((s, have, rep))
        have += rep
    return hlit, out


@pytest.mark.parametrize("name", PC.CASES)
def test_ref_equals_zlib_golden_and_live_pillow(name):
    data = PC.file(name)
    st = R.stages(data)
    assert st.raw == zlib.decompress(st.plan.stream)
    assert equals_golden(name, st.pixels)
    assert equals_golden(name, R.pillow_pixels(data))


@pytest.mark.parametrize("name", list(PC.FLAGGED))
def test_ref_flags_what_zlib_rejects(name):
    data = PC.file(name)
    p = R.parse(data)
    with pytest.raises(R.Flag) as e:
        R.stages(data)
    want = PC.FLAGGED[name]
    assert e.value.bits != 0 and (want is None or e.value.bits == want)
    if want is not None and want < R.MORE:         # the malformed streams proper: zlib 1.2.11 rejects them too
        with pytest.raises(zlib.error):
            zlib.decompress(p.stream)
    if PC.pillow_error(name) is None:              # Pillow gave pixels although the device flags the file: they are what the fallback returns
        assert np.array_equal(R.pillow_pixels(data), PC.pixels(name))


def test_cases_hit_what_they_are_for():
    s = {n: R.parse(PC.file(n)) for n in PC.CASES}
    kinds = {n: [k for k, _ in blocks(s[n].stream)] for n in PC.DEFLATE}
    assert kinds["stored"] == [0] and kinds["fixed"] == [1] and kinds["dynamic"] == [2]
    assert set(kinds["stored.multi"]) == {0} and len(kinds["stored.multi"]) >= 3 and b"\x00\x00\xff\xff" in s["stored.multi"].stream      # a zero-length block
    assert kinds["mixed"] == [1, 0, 0, 2] and blocks(s["mixed"].stream)[1][1] % 8 != 0                # the second block starts inside a byte
    assert len(kinds["flush.full"]) >= 2
    assert len(R.stages(PC.file("period32768")).raw) > 2 * 32768 and b"IDAT" in PC.file("period32768")
    # a stream starts at a multiple of 16 of the upload block, so this is where in its last 8-byte chunk the deflate data ends: every place, 0 = at its end
    assert {(len(p.stream) - 4) % 8 for p in s.values()} == set(range(8))
    hlit, syms = code_length_symbols(s["clsyms"].stream)
    assert {16, 17, 18} <= {sym for sym, _, _ in syms}
    assert any(sym == 16 and at < hlit < at + rep for sym, at, rep in syms)                            # a repeat that starts in the literal/length lengths and ends in the distance lengths
    assert max(R.stages(PC.file("bits15")).raw) == 14 and code_length_symbols(s["bits15"].stream)[1][14][0] == 15      # 15-bit codes exist and are used
    assert {(p.color, p.depth) for p in s.values()} >= {(0, 8), (2, 8), (4, 8), (6, 8), (3, 1), (3, 2), (3, 4), (3, 8)}
    assert all((s[n].W * s[n].depth) % 8 for n in ("pal1.w7", "pal2.w5", "pal4.w3"))                  # rows end in padding bits
    assert b"tRNS" in PC.file("pal.trns") and b"tRNS" in PC.file("rgb.trns")
    for ft in range(5):
        raw = R.stages(PC.file(f"filter.{ft}")).raw
        assert {raw[y * 16] for y in range(3)} == {ft}
    raw = R.stages(PC.file("filter.all")).raw
    assert {raw[y * 21] for y in range(7)} == {0, 1, 2, 3, 4}
    rows = R.stages(PC.file("paeth.ties")).rows.astype(int)
    ties = set()
    for y in range(1, 8):
        for x in range(1, 8):
            a, b, c = rows[y, x - 1], rows[y - 1, x], rows[y - 1, x - 1]
            pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
            ties |= {("ab" if pa == pb else ""), ("ac" if pa == pc else ""), ("bc" if pb == pc else "")}
    assert ties >= {"ab", "ac", "bc"}
    st = R.stages(PC.file("avg.carry"))
    rows = st.rows.astype(int)
    assert {st.raw[y * 13] for y in range(4)} == {3} and (rows[1:, :-2] + rows[:-1, 2:]).max() >= 256      # filter 3 with left + up (bpp 2) carrying into bit 8
    assert PC.file("idat.bytes").count(b"IDAT") == len(s["rgb"].stream) and PC.file("idat.empty").count(b"IDAT") == 3
    assert PC.file("long").count(b"IDAT") >= 2 and s["long"].raw_bytes > 4 * 32768
    assert set(PC.BATCH) <= set(PC.PIXEL_CASES) and len({PC.pixels(n).shape for n in PC.BATCH} | {s[n].color for n in PC.BATCH}) >= 6


# ------------------------------------------------------------------------------------------------ the parser
def _rechunk(data: bytes, edit) -> bytes:
    """The file with its chunk list [(type, body)] passed through `edit` and every CRC recomputed."""
    pos, chunks = 8, []
    while pos < len(data):
        L = int.from_bytes(data[pos:pos + 4], "big")
        chunks.append((data[pos + 4:pos + 8], data[pos + 8:pos + 8 + L]))
        pos += 12 + L
    return data[:8] + b"".join(PC.chunk(t, b) for t, b in edit(chunks))


def test_parser_accepts_the_supported_class():
    for name in PC.CASES + list(PC.FLAGGED):
        plan, p = dataio.parse_png(PC.file(name)), R.parse(PC.file(name))
        assert plan is not None, name
        assert (plan["H"], plan["W"], plan["color"], plan["depth"], plan["bpp"], plan["rowbytes"], plan["wbits"]) == (p.H, p.W, p.color, p.depth, p.bpp, p.rowbytes, p.wbits)
        assert plan["stream"] == p.stream and plan["palette"] == (p.palette if p.color == 3 else b"") and plan["format"] == "png", name
    assert dataio.PngDecoder.parse(PC.file("rgb")) is not None
    # what Pillow ignores for the pixels, the parser passes over: ancillary chunks, a suggested palette in an RGB file
    base = PC.file("rgb")
    for extra in ((b"tEXt", b"k\x00v"), (b"gAMA", (45455).to_bytes(4, "big")), (b"PLTE", bytes(9))):
        data = _rechunk(base, lambda ch: ch[:1] + [extra] + ch[1:])
        assert dataio.parse_png(data) is not None and np.array_equal(R.pillow_pixels(data), PC.pixels("rgb")), extra[0]


def test_parser_refuses_everything_else():
    for name in PC.FALLBACK:
        assert dataio.parse_png(PC.file(name)) is None, name
    base, pal = PC.file("rgb"), PC.file("pal4.w3")
    assert dataio.parse_png(base) is not None and dataio.parse_png(pal) is not None
    ihdr = lambda at, v: (lambda ch: [(ch[0][0], ch[0][1][:at] + bytes([v]) + ch[0][1][at + 1:])] + ch[1:])
    stream = R.parse(base).stream
    restream = lambda s: (lambda ch: [c if c[0] != b"IDAT" else (b"IDAT", s) for c in ch])
    wide = dataio._lib.PNGDEC_MAX_ROWBYTES // 4 + 1
    refused = {
        "empty": b"", "signature only": base[:8], "not a png": b"\x00" * 64,
        "truncated": base[:len(base) * 6 // 10], "no IEND": base[:-12], "data after IEND": base + b"\x00",
        "bad IHDR crc": base[:29] + bytes([base[29] ^ 1]) + base[30:],
        "bad IEND crc": base[:-1] + bytes([base[-1] ^ 1]),
        "16-bit": _rechunk(base, ihdr(8, 16)), "compression 1": _rechunk(base, ihdr(10, 1)), "filter method 1": _rechunk(base, ihdr(11, 1)),
        "interlace": _rechunk(base, ihdr(12, 1)), "colour type 5": _rechunk(base, ihdr(9, 5)), "width 0": _rechunk(base, lambda ch: [(b"IHDR", bytes(4) + ch[0][1][4:])] + ch[1:]),
        "no IDAT": _rechunk(base, lambda ch: [c for c in ch if c[0] != b"IDAT"]),
        "IDAT before IHDR": _rechunk(base, lambda ch: [ch[1], ch[0]] + ch[2:]),
        "IDATs apart": _rechunk(PC.file("idat.empty"), lambda ch: ch[:2] + [(b"tEXt", b"k\x00v")] + ch[2:]),
        "acTL": _rechunk(base, lambda ch: ch[:1] + [(b"acTL", bytes(8))] + ch[1:]),
        "unknown critical chunk": _rechunk(base, lambda ch: ch[:1] + [(b"ABCD", b"")] + ch[1:]),
        "two IHDR": _rechunk(base, lambda ch: ch[:1] + ch[:1] + ch[1:]),
        "palette without PLTE": _rechunk(pal, lambda ch: [c for c in ch if c[0] != b"PLTE"]),
        "PLTE shorter than the depth's indices": _rechunk(pal, lambda ch: [c if c[0] != b"PLTE" else (b"PLTE", c[1][:45]) for c in ch]),
        "PLTE not a multiple of 3": _rechunk(pal, lambda ch: [c if c[0] != b"PLTE" else (b"PLTE", c[1] + b"\x00") for c in ch]),
        "PLTE after IDAT": _rechunk(pal, lambda ch: [ch[0], ch[2], ch[1]] + ch[3:]),
        "PLTE in a grey file": _rechunk(PC.file("grey"), lambda ch: ch[:1] + [(b"PLTE", bytes(9))] + ch[1:]),
        "zlib CM 7": _rechunk(base, restream(b"\x77\x05" + stream[2:])),
        "zlib CINFO 8": _rechunk(base, restream(b"\x88\x1c" + stream[2:])),
        "zlib FDICT": _rechunk(base, restream(b"\x78\x20" + stream[2:])),
        "zlib FCHECK": _rechunk(base, restream(bytes([stream[0], stream[1] ^ 1]) + stream[2:])),
        "stream of 6 bytes": _rechunk(base, restream(stream[:2] + stream[-4:])),
        "a row longer than the kernel's rows": PC.write_png(wide, 1, 6, 8, zlib.compress(bytes(1 + 4 * wide))),
        "more pixels than Pillow opens": PC.write_png(16384, 16384, 0, 8, stream),
        "raw bytes past 31 bits": PC.write_png(4096, 140000, 6, 8, stream),
    }
    for what, data in refused.items():
        assert dataio.parse_png(data) is None, what
    assert dataio.parse_png(PC.write_png(wide - 1, 1, 6, 8, zlib.compress(bytes(1 + 4 * (wide - 1))))) is not None      # the cap itself is taken: 4096 pixels of RGBA
    assert dataio.parse_jpeg(base) is None and dataio.parse_png(JC.file("mcu.444")) is None


def _with_chunk(base: bytes, typ: bytes, body: bytes, after_idat: bool) -> bytes:
    """`base` with one more CRC-valid chunk, in front of its first IDAT or in front of its IEND."""
    def edit(ch):
        at = len(ch) - 1 if after_idat else next(i for i, c in enumerate(ch) if c[0] == b"IDAT")
        return ch[:at] + [(typ, body)] + ch[at:]
    return _rechunk(base, edit)


# one CRC-valid ancillary chunk added to the golden `rgb` (or the named) file: what Pillow 12.2.0 raises for it, in dataio._decode's OSError
MALFORMED_ANCILLARY = [
    ("rgb", b"pHYs", 4, False, "Truncated pHYs chunk"), ("rgb", b"pHYs", 4, True, "Truncated pHYs chunk"), ("rgb", b"sRGB", 0, False, "Truncated sRGB chunk"),
    ("rgb", b"gAMA", 1, False, "cannot identify image file"), ("rgb", b"cHRM", 2, False, "cannot identify image file"),
    ("rgb", b"tRNS", 1, False, "cannot identify image file"), ("grey", b"tRNS", 1, False, "cannot identify image file"),
    ("rgb", b"fdAT", 8, False, "cannot identify image file"), ("rgb", b"fcTL", 26, False, "tile cannot extend outside image"),
]


@pytest.mark.parametrize("name,typ,length,after,text", MALFORMED_ANCILLARY, ids=[f"{n}-{t.decode()}{L}{'-after' if a else ''}" for n, t, L, a, _ in MALFORMED_ANCILLARY])
def test_parser_refuses_ancillary_chunks_pillow_raises_for(name, typ, length, after, text):
    import io
    data = _with_chunk(PC.file(name), typ, bytes(length), after)
    assert dataio.parse_png(data) is None
    with pytest.raises(OSError, match=text) as plain:
        dataio._decode(io.BytesIO(data))
    dec = dataio.PngDecoder("cpu", ops=PngDecEmuOps())
    with pytest.raises(OSError, match=text):
        dec.decode([data])                                         # with the decoder the caller sees the same failure, not pixels
    assert "cannot decode image" in str(plain.value) and dec.stats["unsupported"] == 0      # it raised before anything was counted


def test_whatever_chunk_the_parser_passes_over_pillow_passes_over_too():
    """Every chunk type Pillow has a handler for and some it has none for, at lengths below, at and above what Pillow needs, in front of the
    IDATs and behind them: wherever the parser still takes the file, Pillow decodes it to the same pixels."""
    types = [b"gAMA", b"cHRM", b"sRGB", b"pHYs", b"tRNS", b"tEXt", b"zTXt", b"iTXt", b"iCCP", b"eXIf", b"acTL", b"fcTL", b"fdAT", b"bKGD", b"tIME", b"sBIT",
             b"hIST", b"sPLT", b"prVt", b"ab1d", b"a_cd"]
    taken, refused = set(), 0
    for name in ("rgb", "grey", "rgba", "pal4.w3"):
        base, want = PC.file(name), PC.pixels(name)
        for typ in types:
            for length in (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 16, 17, 26, 32, 33, 40):
                for after in (False, True):
                    for body in (bytes(length), bytes(range(1, length + 1))):
                        data = _with_chunk(base, typ, body, after)
                        if dataio.parse_png(data) is None:
                            refused += 1
                            continue
                        taken.add((typ, length))
                        assert np.array_equal(R.pillow_pixels(data), want), (name, typ, length, after)
    assert refused > 1000 and {t for t, _ in taken} == {b"gAMA", b"cHRM", b"sRGB", b"pHYs", b"tRNS", b"tEXt", b"bKGD", b"tIME", b"sBIT", b"hIST", b"sPLT", b"prVt"}
    assert {L for t, L in taken if t == b"pHYs"} == {9} and {L for t, L in taken if t == b"gAMA"} == {4} and {L for t, L in taken if t == b"cHRM"} == {32}
    assert {L for t, L in taken if t == b"sRGB"} == {1} and {L for t, L in taken if t == b"tRNS"} == {1, 2, 3, 4, 5, 6, 8, 9, 10, 16}      # RGB: 6; 16 palette entries
    big = _with_chunk(PC.file("rgb"), b"tEXt", b"k\x00" + bytes(70000), False)
    assert dataio.parse_png(big) is None and np.array_equal(R.pillow_pixels(big), PC.pixels("rgb"))      # refused for its size alone: Pillow still decodes it


# ------------------------------------------------------------------------------------------------ the arithmetic under sanitizers
def corrupt_variants(name: str, k: int = 4):
    """Deterministic damage to the zlib stream of a case inside a valid container: bytes overwritten, the stream cut short, bits of the
    first block's header flipped."""
    p = R.parse(PC.file(name))
    s = p.stream
    rng = np.random.default_rng(sum(name.encode()))
    out = []
    for i in range(k):
        v = bytearray(s)
        if i % 4 == 0:
            for pos in rng.integers(2, len(s), 1 + i % 3):
                v[pos] = int(rng.integers(0, 255))
        elif i % 4 == 1:
            v = v[:int(rng.integers(3, len(s)))] + v[-4:]
        elif i % 4 == 2:
            v[2] ^= 1 << int(rng.integers(0, 8))                # BFINAL, BTYPE, HLIT
        else:
            at = int(rng.integers(2, min(len(s), 12)))
            v[at] ^= 1 << int(rng.integers(0, 8))               # HDIST, HCLEN, the code-length code; LEN / NLEN of a stored block
        if len(v) >= 7:
            out.append(PC.write_png(p.W, p.H, p.color, p.depth, bytes(v), palette=p.palette or None))
    return out


def expectation(data: bytes):
    """(error bits expected, pixels otherwise) by tests.pngdec_ref."""
    try:
        return 0, R.decode(data)
    except R.Flag as e:
        return e.bits, None


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = os.environ.get("HOSTCXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler (c++, g++ or clang++) or no make on this machine: the sanitizer build of csrc/pngdec_host.cpp cannot be made")
    exe = tmp_path_factory.mktemp("pngdec_host") / "pngdec_host"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "gan-variant-research_amd", "csrc"), "pngdec_host", f"HOSTCXX={cxx}", f"PNGHOSTBIN={exe}"],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip(f"{cxx} has no AddressSanitizer / UBSan runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


def run_host(exe, files, tmp_path):
    """The files (all accepted by the parser) through the host program -> (error words, pixel arrays)."""
    dec = dataio.PngDecoder("cpu", ops=PngDecEmuOps())
    plans = [dataio.parse_png(f) for f in files]
    offs, end = [], 0
    for p in plans:
        offs.append(end)
        end += p["H"] * p["W"] * 3
    total, n, ws = dec._pack(plans, offs)
    o_pal, _ = dec.ops.pngdec_block_offsets(n)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(np.array([total, n, ws, end, o_pal], np.int64).tobytes() + dec._host[:total].numpy().tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]                 # a sanitizer report ends the program with a non-zero status
    raw = np.fromfile(dst, np.uint8)
    return raw[:4 * n].view(np.int32).tolist(), [raw[4 * n + o:][:p["H"] * p["W"] * 3].reshape(p["H"], p["W"], 3) for o, p in zip(offs, plans)]


def test_host_program_under_sanitizers(host_program, tmp_path):
    """Every case, every flagged file, then every corrupted variant: no sanitizer report, and the pixels or the very error word that
    tests.pngdec_ref expects.  The GPU tests decode the corrupt files only after this."""
    err, px = run_host(host_program, [PC.file(n) for n in PC.CASES], tmp_path)
    assert err == [0] * len(PC.CASES)
    for n, p in zip(PC.CASES, px):
        assert equals_golden(n, p), n
    names = list(PC.FLAGGED)
    err, px = run_host(host_program, [PC.file(n) for n in names], tmp_path)
    for n, e in zip(names, err):
        assert e == expectation(PC.file(n))[0] != 0 and (PC.FLAGGED[n] is None or e == PC.FLAGGED[n]), (n, e)
    variants = [v for n in PC.CASES if n != "long" for v in corrupt_variants(n)] + corrupt_variants("long", 3)
    taken = [v for v in variants if dataio.parse_png(v) is not None]
    assert len(taken) == len(variants) > 100                   # the container is intact: the parser takes them all
    want = [expectation(v) for v in taken]
    err, px = run_host(host_program, taken, tmp_path)
    flagged = 0
    for i, ((bits, pixels), e, p) in enumerate(zip(want, err, px)):
        assert e == bits, (i, e, bits)
        flagged += bool(bits)
        if not bits:
            assert np.array_equal(p, pixels), i
    assert flagged >= len(taken) // 2 and len({e for e in err if e}) >= 6       # many kinds of irregularity


# ------------------------------------------------------------------------------------------------ the decoders on the emulator
def _pillow_outcome(name):
    """What dataio._decode gives for the file: pixels, or the OSError's text."""
    import io
    try:
        return dataio._decode(io.BytesIO(PC.file(name))), None
    except OSError as e:
        return None, str(e)


def test_decoder_equals_pillow_and_counts_the_fallbacks(tmp_path):
    dec = dataio.PngDecoder("cpu", ops=PngDecEmuOps())
    got = dec.decode([PC.file(n) for n in PC.PIXEL_CASES])
    for n, g in zip(PC.PIXEL_CASES, got):
        assert g.dtype == torch.uint8 and np.array_equal(g.numpy(), PC.pixels(n)), n
    assert dec.stats == {"device": len(PC.PIXEL_CASES), "unsupported": 0, "flagged": 0} and dec.last_errors == {}
    assert all(equals_golden(n, g.numpy()) for n, g in zip(PC.HASHED, dec.decode([PC.file(n) for n in PC.HASHED])))
    decodable = [n for n in PC.FALLBACK + list(PC.FLAGGED) if _pillow_outcome(n)[1] is None]
    assert set(decodable) >= {"rgb16", "grey2", "interlaced", "jpeg", "surplus"}
    names, paths = decodable + PC.BATCH, []
    for n in names:                                               # paths and bytes are both sources
        paths.append(tmp_path / (n + (".jpg" if n == "jpeg" else ".png")))
        paths[-1].write_bytes(PC.file(n))
    before = dict(dec.stats)
    got = dec.decode(paths)
    for n, g in zip(names, got):
        assert np.array_equal(g.numpy(), _pillow_outcome(n)[0]), n
    nflag = sum(n in PC.FLAGGED for n in decodable)
    assert dec.stats == {"device": before["device"] + len(PC.BATCH), "unsupported": len(decodable) - nflag, "flagged": nflag}
    assert dec.last_errors[names.index("surplus")] == R.MORE
    assert all((g.data_ptr() - got[0].data_ptr()) % dataio.ARENA_ALIGN == 0 for g in got)


@pytest.mark.parametrize("name", [n for n in PC.FLAGGED])
def test_flagged_files_give_pillows_pixels_or_its_error(name, tmp_path):
    p = tmp_path / "f.png"
    p.write_bytes(PC.file(name))
    dec = dataio.PngDecoder("cpu", ops=PngDecEmuOps())
    try:
        want, text = dataio._decode(p), None
    except OSError as e:
        want, text = None, str(e)
    if text is None:
        got = dec.decode([PC.file("grey"), p])
        assert np.array_equal(got[1].numpy(), want) and dec.stats == {"device": 1, "unsupported": 0, "flagged": 1}
    else:
        with pytest.raises(OSError) as mine:
            dec.decode([PC.file("grey"), p])
        assert str(mine.value) == text and str(p) in text
    assert set(dec.last_errors) == {1} and (PC.FLAGGED[name] is None or dec.last_errors[1] == PC.FLAGGED[name])
    assert np.array_equal(dec.decode([PC.file("grey")])[0].numpy(), PC.pixels("grey")) and dec.last_errors == {}      # a good file afterwards


def test_decoder_reused_and_writing_into_a_callers_buffer():
    dec = dataio.PngDecoder("cpu", ops=PngDecEmuOps())
    for names in (PC.BATCH, PC.BATCH + ["dynamic", "const", "jpeg"], PC.BATCH[:2], PC.BATCH[::-1]):      # larger, smaller, reordered
        for n, g in zip(names, dec.decode([PC.file(n) for n in names])):
            assert np.array_equal(g.numpy(), PC.pixels(n)), n
    sizes = [PC.pixels(n).size for n in PC.BATCH]
    offsets = [7 + sum(sizes[:i]) + 3 * i for i in range(len(sizes))]                                  # packed, unaligned
    out = torch.full((offsets[-1] + sizes[-1] + 5,), 0xAB, dtype=torch.uint8)
    got = dec.decode([PC.file(n) for n in PC.BATCH], out=out, offsets=offsets)
    used = np.zeros(out.numel(), bool)
    for n, g, o, s in zip(PC.BATCH, got, offsets, sizes):
        assert g.data_ptr() == out.data_ptr() + o and np.array_equal(g.numpy(), PC.pixels(n))
        used[o:o + s] = True
    assert (out.numpy()[~used] == 0xAB).all()                                                         # nothing else was written
    with pytest.raises(_lib.GanError, match="PngDecoder"):
        dec.decode([PC.file("grey")], out=out)                                                        # offsets missing
    with pytest.raises(_lib.GanError):
        dataio.PngDecoder("cpu")                                                                      # the HIP ops need a GPU: no CPU fallback


def _mixed_folder(root):
    """PNG, baseline JPEG, progressive JPEG and a PNG from FALLBACK, suffixes that do not all tell the truth."""
    root.mkdir(parents=True, exist_ok=True)
    items = [("a.png", PC.file("rgba"), PC.pixels("rgba")), ("b.jpg", JC.file("gray"), JC.pixels("gray")), ("c.jpg", JC.file("progressive"), JC.pixels("progressive")),
             ("d.png", PC.file("rgb16"), PC.pixels("rgb16")), ("e.png", PC.file("pal2.w5"), PC.pixels("pal2.w5")), ("f.png", JC.file("rst"), JC.pixels("rst")),
             ("g.jpg", PC.file("filter.all"), PC.pixels("filter.all")), ("h.png", PC.file("surplus"), PC.pixels("surplus")), ("i.png", PC.file("interlaced"), PC.pixels("interlaced"))]
    paths = []
    for name, data, _ in items:
        paths.append(root / name)
        paths[-1].write_bytes(data)
    return paths, [px for _, _, px in items]


def test_device_decoder_routes_by_content(tmp_path):
    paths, want = _mixed_folder(tmp_path / "mixed")
    dec = dataio.DeviceDecoder("cpu", ops=PngDecEmuOps())
    reads = []
    load = dec.load
    dec.load = lambda s: reads.append(s) or load(s)
    got = dec.decode(paths)
    assert len(reads) == len(paths)                                      # every source is read once
    for g, w in zip(got, want):
        assert np.array_equal(g.numpy(), w)
    assert got[0].untyped_storage().data_ptr() == got[-1].untyped_storage().data_ptr()      # one arena
    assert dec.png.stats == {"device": 3, "unsupported": 2, "flagged": 1} and dec.jpeg.stats == {"device": 2, "unsupported": 1, "flagged": 0}
    assert dec.stats == {"device": 5, "unsupported": 3, "flagged": 1} and dec.last_errors == {7: R.MORE}
    assert dec._err is not None and dec.jpeg._err is None and dec.png._err is None      # one buffer of error words, so one download, for both formats
    only = dataio.DeviceDecoder("cpu", jpeg=False, ops=PngDecEmuOps())
    for g, w in zip(only.decode(paths), want):
        assert np.array_equal(g.numpy(), w)
    assert only.jpeg is None and only.stats == {"device": 3, "unsupported": 5, "flagged": 1}
    with pytest.raises(ValueError):
        dataio.DeviceDecoder("cpu", jpeg=False, png=False, ops=PngDecEmuOps())


# ------------------------------------------------------------------------------------------------ the store, the folder path, the command lines
@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: PngDecEmuOps())
    monkeypatch.setattr(dataio, "InputPipeline", EmuInputPipeline)


@pytest.mark.parametrize("both", [False, True], ids=["png", "png+jpeg"])
@pytest.mark.parametrize("budget", [None, 0], ids=["resident", "streaming"])
def test_image_store_device_png_holds_the_same_bytes(emulated, tmp_path, monkeypatch, budget, both):
    paths, want = _mixed_folder(tmp_path / "imgs")
    monkeypatch.setattr(dataio, "DECODE_CHUNK", 4)                       # several chunks
    plain = dataio.ImageStore(paths, "cpu", budget_bytes=budget, workers=2)
    store = dataio.ImageStore(paths, "cpu", budget_bytes=budget, workers=2, device_png=True, device_decode=both)
    assert isinstance(store._decoder, dataio.DeviceDecoder if both else dataio.PngDecoder)
    assert store.resident == plain.resident == (budget is None)
    assert store.sizes == plain.sizes and store.offsets == plain.offsets and store.nbytes == plain.nbytes
    for i, w in enumerate(want):
        assert np.array_equal(store[i].numpy(), w) and torch.equal(store[i], plain[i]), i
    order = [7, 0, 3, 3, 8]
    for a, b in zip(store.fetch(order), plain.fetch(order)):
        assert torch.equal(a, b)
    if budget is None:
        assert store._decoder.stats == ({"device": 5, "unsupported": 3, "flagged": 1} if both else {"device": 3, "unsupported": 5, "flagged": 1})
    store.close(), plain.close()


def test_image_store_reports_an_undecodable_file_as_before(emulated, tmp_path):
    paths = [tmp_path / "a.png", tmp_path / "b.png"]
    paths[0].write_bytes(PC.file("grey")), paths[1].write_bytes(PC.file("bad.adler"))
    errors = []
    for on in (False, True):
        with pytest.raises(OSError) as e:
            dataio.ImageStore(paths, "cpu", workers=2, device_png=on)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and errors[0].startswith(f"cannot decode image {paths[1]}") and "broken data stream" in errors[0]


def test_trainers_pass_the_config_key_to_their_stores(emulated, tmp_path):
    from gan_variant_research_amd import train_basic, train_cutpp
    assert train_basic.build_store is train_cutpp.build_store
    paths = [tmp_path / "a.png", tmp_path / "b.png"]
    paths[0].write_bytes(PC.file("grey")), paths[1].write_bytes(PC.file("rgba"))
    off = train_cutpp.build_store(paths, "cpu", {}, "A", quiet=True)
    on = train_cutpp.build_store(paths, "cpu", {"mi355x": {"device_png": True}}, "A", quiet=True)
    both = train_cutpp.build_store(paths, "cpu", {"mi355x": {"device_png": True, "device_decode": True}}, "A", quiet=True)
    assert off._decoder is None and isinstance(on._decoder, dataio.PngDecoder) and on._decoder.stats["device"] == 2
    assert isinstance(both._decoder, dataio.DeviceDecoder) and all(torch.equal(on[i], off[i]) and torch.equal(both[i], off[i]) for i in range(2))


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
    for name, shape in (("a.png", (20, 24, 3)), ("sub/b.png", (33, 17, 4)), ("sub/c.png", (24, 24)), ("d.png", (40, 31, 3))):
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8)).save(photos / name)
    Image.fromarray(rng.integers(0, 256, (9, 50, 3), dtype=np.uint8)).quantize(16).save(photos / "e.png")       # 4-bit indices, 16 entries
    Image.fromarray(rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)).save(photos / "f.jpg", quality=90)
    Image.fromarray(rng.integers(0, 256, (16, 30, 3), dtype=np.uint8)).save(photos / "sub" / "g.jpg", progressive=True)
    (photos / "h.png").write_bytes(PC.file("rgb16"))
    return G, photos, tmp_path


def _files(root):
    return {p.relative_to(root).as_posix(): p.read_bytes() for p in root.rglob("*") if p.is_file()}


def test_stylize_folder_device_png_on_the_emulator(folder):
    G, photos, tmp = folder
    run = lambda out, **kw: I.stylize_folder(G, str(photos), str(tmp / out), device="cpu", img_size=24, batch=2, device_io=True, **kw)
    assert run("pil") == 8
    want = _files(tmp / "pil")
    assert len(want) == 8
    assert run("png", device_png=True) == 8 and _files(tmp / "png") == want
    assert G._png_dec.stats == {"device": 5, "unsupported": 3, "flagged": 0} and not hasattr(G, "_jpeg_dec")
    dec = G._png_dec
    for chunk in (1, 3, 16):                                                   # chunks smaller than, across and larger than the batches
        assert run(f"png{chunk}", device_png=True, decode_chunk=chunk, io_threads=3, device_jpeg=True) == 8 and _files(tmp / f"png{chunk}") == want
    assert G._png_dec is dec                                                   # cached on the generator, like the input pipeline
    assert run("both", device_png=True, device_decode=True) == 8 and _files(tmp / "both") == want
    assert G._device_dec.stats == {"device": 6, "unsupported": 2, "flagged": 0} and G._device_dec.jpeg.stats["device"] == 1
    assert run("lim", device_png=True, limit=3) == 3 and _files(tmp / "lim") == {k: want[k] for k in sorted(want)[:3]}
    with pytest.raises(ValueError, match="device_io"):
        I.stylize_folder(G, str(photos), str(tmp / "bad"), device="cpu", img_size=24, device_png=True)
    with pytest.raises(ValueError, match="decode_chunk"):
        run("bad", device_png=True, decode_chunk=0)


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
    assert GF.main(base + ["--out", str(tmp / "plain")]) == 8
    assert GF.main(base + ["--out", str(tmp / "png"), "--device-png", "--decode-chunk", "4"]) == 8
    assert GF.main(base + ["--out", str(tmp / "both"), "--device-png", "--device-decode"]) == 8
    assert "device_png" not in seen[0] and "decode_chunk" not in seen[0]               # with the flag off the call is the parent's
    assert (seen[1]["device_png"], seen[1]["decode_chunk"], seen[1]["device_io"]) == (True, 4, True) and "device_decode" not in seen[1]
    assert (seen[2]["device_png"], seen[2]["device_decode"], seen[2]["decode_chunk"]) == (True, True, 256)
    assert _files(tmp / "png") == _files(tmp / "plain") == _files(tmp / "both") and len(_files(tmp / "png")) == 8
    assert GF.parse_args(["--ckpt", "c", "--photos", "p", "--out", "o"]).device_png is False
    for bad in (["--device-png", "--host-io"], ["--device-png", "--device", "cpu"]):
        with pytest.raises(SystemExit):
            GF.parse_args(["--ckpt", "c", "--photos", "p", "--out", "o"] + bad)
    assert "--device-png" in capsys.readouterr().err
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)                     # no quiet fallback to PIL
    with pytest.raises(SystemExit, match="device-png"):
        GF.main(base + ["--out", str(tmp / "x"), "--device-png"])
    assert "Falling back" not in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ the C entries
def packed(names, out_offsets=None):
    """A valid upload block of the named cases in host memory -> (keep-alive decoder, block tensor, bytes, n, ws bytes)."""
    dec = dataio.PngDecoder("cpu", ops=PngDecEmuOps())
    plans = [dataio.parse_png(PC.file(n)) for n in names]
    offs = out_offsets or [sum(p["H"] * p["W"] * 3 for p in plans[:i]) for i in range(len(plans))]
    total, n, ws = dec._pack(plans, offs)
    return dec, dec._host, total, n, ws


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmi355x_gan.so is not built")
    return _lib.load()


def test_c_layout_entries_agree_with_the_emulator(lib):
    from tests.emulator_pngdec import block_offsets
    err = lambda: lib.gan_last_error()
    off = (C.c_int64 * 2)()
    assert lib.gan_pngdec_block_offsets(3, off) == 0 and tuple(off) == block_offsets(3)
    for n in (0, 65536):
        assert lib.gan_pngdec_block_offsets(n, off) < 0 and b"65535" in err()
    assert lib.gan_pngdec_block_offsets(1, None) < 0 and b"null" in err()
    dec, host, total, n, ws_bytes = packed(PC.BATCH)
    imgs = (_lib.GanPngdecImage * n).from_buffer_copy(host[:n * C.sizeof(_lib.GanPngdecImage)].numpy().tobytes())
    want = [im.raw_off for im in imgs]
    for im in imgs:
        im.raw_off = -1
    ws = C.c_int64(0)
    assert lib.gan_pngdec_bounds(C.cast(imgs, C.c_void_p), n, C.byref(ws)) == 0 and ws.value == ws_bytes and [im.raw_off for im in imgs] == want
    assert lib.gan_pngdec_bounds(None, n, C.byref(ws)) < 0 and b"null" in err()
    for field, value, word in (("H", 0, b"below 1"), ("color", 5, b"colour type"), ("depth", 16, b"colour type"), ("rowbytes", 3, b"rowbytes"), ("bpp", 9, b"bpp"),
                               ("pal_count", 3, b"palette"), ("wbits", 16, b"window"), ("wbits", 7, b"window")):
        bad = (_lib.GanPngdecImage * 1).from_buffer_copy(bytes(imgs[0]))
        setattr(bad[0], field, value)
        assert lib.gan_pngdec_bounds(C.cast(bad, C.c_void_p), 1, C.byref(ws)) < 0 and word in err(), field
    pal = (_lib.GanPngdecImage * 1).from_buffer_copy(bytes(imgs[PC.BATCH.index("pal2.w5")]))
    pal[0].pal_count = 3
    assert lib.gan_pngdec_bounds(C.cast(pal, C.c_void_p), 1, C.byref(ws)) < 0 and b"palette" in err()
    big = (_lib.GanPngdecImage * 1).from_buffer_copy(bytes(imgs[0]))
    big[0].W, big[0].rowbytes = 4097, 4 * 4097
    assert lib.gan_pngdec_bounds(C.cast(big, C.c_void_p), 1, C.byref(ws)) < 0 and b"rows hold" in err()
    big[0].W, big[0].rowbytes, big[0].H = 4096, 4 * 4096, 140000
    assert lib.gan_pngdec_bounds(C.cast(big, C.c_void_p), 1, C.byref(ws)) < 0 and b"too large" in err()


def test_c_entries_refuse_inconsistent_blocks_before_any_launch(lib):
    """No launch happens: every call below is refused on the host copy of the descriptors (the device pointer is never followed)."""
    err = lambda: lib.gan_last_error()
    dec, host, total, n, ws_bytes = packed(PC.BATCH)
    p = C.c_void_p(host.data_ptr())
    isz = C.sizeof(_lib.GanPngdecImage)
    entries = [lambda *a: lib.gan_pngdec_inflate(*a, None), lambda *a: lib.gan_pngdec_pixels(*a, p, 1 << 30, None, None)]
    good = (p, p, total, n, p, ws_bytes)

    def with_field(i, field, value):
        blk = host[:total].clone()
        im = _lib.GanPngdecImage.from_buffer_copy(blk[i * isz:(i + 1) * isz].numpy().tobytes())
        setattr(im, field, value)
        blk[i * isz:(i + 1) * isz] = torch.frombuffer(bytearray(bytes(im)), dtype=torch.uint8)
        return blk

    for entry in entries:
        assert entry(None, p, total, n, p, ws_bytes) < 0 and b"null" in err()
        assert entry(p, None, total, n, p, ws_bytes) < 0 and b"null" in err()
        assert entry(p, p, total, n, None, ws_bytes) < 0 and b"null" in err()
        assert entry(p, p, total, 0, p, ws_bytes) < 0 and b"65535" in err()
        assert entry(p, p, 64, n, p, ws_bytes) < 0 and b"descriptors" in err()
        assert entry(p, p, total - 8, n, p, ws_bytes) < 0 and b"multiple of 16" in err()
        assert entry(C.c_void_p(host.data_ptr() + 4), p, total, n, p, ws_bytes) < 0 and b"aligned" in err()
        assert entry(p, p, total, n, C.c_void_p(host.data_ptr() + 8), ws_bytes) < 0 and b"aligned" in err()
        assert entry(p, p, total, n, p, ws_bytes - 256) < 0 and b"workspace" in err()
        assert entry(p, p, total, n, p, 16) < 0 and b"workspace" in err()
        for field, value, word in (("stream_off", 8, b"stream"), ("stream_off", total, b"stream"), ("stream_len", total, b"stream"), ("stream_len", 6, b"stream"),
                                   ("stream_off", None, b"stream"), ("raw_off", 0, b"raw offset"), ("raw_off", ws_bytes, b"raw offset"), ("raw_off", None, b"raw offset"),
                                   ("W", 9, b"rowbytes"), ("depth", 4, b"colour type"), ("wbits", 0, b"window")):
            i = 2
            im = _lib.GanPngdecImage.from_buffer_copy(host[i * isz:(i + 1) * isz].numpy().tobytes())
            blk = with_field(i, field, getattr(im, field) + 4 if value is None else value)
            assert entry(p, C.c_void_p(blk.data_ptr()), total, n, p, ws_bytes) < 0 and word in err(), (field, value)
    assert lib.gan_pngdec_pixels(*good, None, 1 << 30, None, None) < 0 and b"null" in err()
    assert lib.gan_pngdec_pixels(*good, p, 100, None, None) < 0 and b"output" in err()
    blk = with_field(1, "out_off", -1)
    assert lib.gan_pngdec_pixels(p, C.c_void_p(blk.data_ptr()), total, n, p, ws_bytes, p, 1 << 30, None, None) < 0 and b"output" in err()
