"""TEST INFRASTRUCTURE: the progressive decoder's test cases, read from tests/golden/jpegprog_cases.npz (written by
tools/make_golden_jpegprog.py with Pillow 12.2.0 / libjpeg-turbo): per case the file's bytes and the pixels
np.array(Image.open(..).convert("RGB")) gave (a SHA-256 for `long`; a `.raises` entry where Pillow raised).  Also the tests' own
progressive writer (coefficients + a scan script -> file), which makes the scripts Pillow cannot be asked for."""
from __future__ import annotations

import hashlib
import os
from functools import lru_cache

import numpy as np

from tests.jpegdec_cases import S420, S422, S444, _seg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpegprog_cases.npz")

# name -> (H, W, mode / subsampling, quality, save options), all saved with progressive=True: the smallest shapes at which each part can go wrong
CASES = {
    "pixel.444": (1, 1, S444, 95, {}), "pixel.420": (1, 1, S420, 95, {}), "pixel.gray": (1, 1, "L", 95, {}),
    "mcu.444": (8, 8, S444, 95, {}), "mcu.420": (16, 16, S420, 95, {}),
    # the real luma grid of a single-component scan is narrower (W = 33: 5 of 6 block columns) or shorter (H = 17: 3 of 4 rows) than the padded one
    "ragged.9x33.444": (9, 33, S444, 95, {}), "ragged.9x33.422": (9, 33, S422, 95, {}), "ragged.9x33.420": (9, 33, S420, 95, {}),
    "ragged.17x15.444": (17, 15, S444, 95, {}), "ragged.17x15.422": (17, 15, S422, 95, {}), "ragged.17x15.420": (17, 15, S420, 95, {}),
    "narrow.5.420": (7, 5, S420, 95, {}),
    "gray": (24, 40, "L", 95, {}),
    "const.gray": (256, 256, "L", 95, {}),                 # 1024 blocks in one EOB run: category 10, extra bits across a byte boundary
    "runs": (64, 64, S420, 1, {}),                         # ZRL in first and in refinement scans
    "magnitudes": (16, 16, S444, 100, {}),                 # checkerboard: corrections on large positive and negative values
    "stuffing": (64, 64, S444, 95, {}),                    # 0xFF bytes in the scans
    "rst": (40, 50, S420, 95, {"restart_marker_blocks": 3}),           # MCUs in the DC scans, blocks in the AC scans; ends EOB runs
    "rst_wrap": (64, 64, S444, 60, {"restart_marker_blocks": 1}),      # RSTn wraps within every scan
    "long": (256, 256, S420, 90, {}),                      # the dataset's shape; pixels kept as a SHA-256
}
WRITER = ["dc_split", "spectral_only", "deep", "tables4", "dri_change", "order", "tables20"]
ALL = list(CASES) + WRITER
PIXEL_CASES = [n for n in ALL if n != "long"]
FALLBACK = ["short_of_al0", "no_ac_scan", "ac_before_dc", "ac_two_components", "scans65", "s411", "adobe", "arithmetic", "truncated"]
FLAGGED = {"crafted.s2": 256, "crafted.eobrun": 512, "crafted.range": 1024, "corrupt": None}       # name -> the error word (None: whatever the reference says)
CORRUPT_BYTES = 3
MIXED = ["base.a", "ragged.9x33.422", "base.b", "gray", "dc_split", "png", "s411", "corrupt"]      # two baseline, three progressive, a PNG, a fallback, a flagged one


@lru_cache(maxsize=None)
def _npz():
    return dict(np.load(GOLDEN))


def file(name: str) -> bytes:
    return _npz()[f"{name}.file"].tobytes()


def raises(name: str) -> bool:
    """Whether Pillow raised for the file when the golden data was written."""
    return f"{name}.raises" in _npz()


def pixels(name: str) -> np.ndarray:
    return _npz()[f"{name}.rgb"]


def pixels_sha256(name: str) -> bytes:
    z = _npz()
    return z[f"{name}.sha256"].tobytes() if f"{name}.sha256" in z else hashlib.sha256(np.ascontiguousarray(z[f"{name}.rgb"]).tobytes()).digest()


def shape(name: str):
    return CASES[name][:2] if name in CASES else tuple(int(v) for v in _npz()[f"{name}.rgb"].shape[:2])


def corrupt_seed() -> int:
    return int(_npz()["corrupt.seed"][0])


def scan_ranges(data: bytes):
    """[(first byte, end)] of the entropy-coded bytes of every scan, RSTn included."""
    from tests import jpegprog_ref as P
    return [(sc.segments[0][0], sc.segments[-1][1]) for sc in P.parse(data).scans]


def corrupted(data: bytes, seed: int, k: int = CORRUPT_BYTES) -> bytes:
    """`data` with k bytes inside the entropy-coded bytes of one scan replaced (never by 0xFF, never a 0xFF or the byte behind one)."""
    r = np.random.default_rng(seed)
    ranges = [(b, e) for b, e in scan_ranges(data) if e - b >= 2 * k + 2]
    b, e = ranges[int(r.integers(len(ranges)))]
    v = bytearray(data)
    cand = [p for p in range(b, e) if v[p] != 0xFF and (p == 0 or v[p - 1] != 0xFF)]
    for p in r.choice(cand, k, replace=False):
        v[int(p)] = int(r.integers(0, 255))
    return bytes(v)


# ------------------------------------------------------------------------------------------------ the tests' own writer
def _value(v: int):
    n = int(abs(v)).bit_length()
    return n, (v if v >= 0 else v + (1 << n) - 1)


class _Scan:
    """The token stream of one scan: ("sym", symbol) | ("bits", value, count) | ("rst",)."""

    def __init__(self):
        self.tok = []

    def sym(self, s):
        self.tok.append(("sym", s))

    def bits(self, v, n):
        if n:
            self.tok.append(("bits", v, n))

    def table(self):
        """(counts, symbols): every used symbol at one length that leaves the all-ones code free."""
        used = sorted({t[1] for t in self.tok if t[0] == "sym"}) or [0]
        L = max(1, int(len(used)).bit_length())
        counts = [0] * 16
        counts[L - 1] = len(used)
        return counts, used

    def encode(self) -> bytes:
        counts, used = self.table()
        L = counts.index(len(used)) + 1
        code = {s: i for i, s in enumerate(used)}
        out, cur = b"", []

        def flush():
            s = "".join(cur)
            s += "1" * (-len(s) % 8)
            cur.clear()
            return int(s, 2).to_bytes(len(s) // 8, "big").replace(b"\xff", b"\xff\x00") if s else b""
        nrst = 0
        for t in self.tok:
            if t[0] == "sym":
                cur.append(f"{code[t[1]]:0{L}b}")
            elif t[0] == "bits":
                cur.append(f"{t[1]:0{t[2]}b}")
            else:
                out += flush() + bytes((0xFF, 0xD0 + nrst % 8))
                nrst += 1
        return out + flush()


def write_progressive(H, W, samp, coefs, qts, script, adobe=False, s2=False, extra_eobrun=0) -> bytes:
    """A progressive file from quantised coefficients.  samp: (h, v) per component; coefs: per component int (blocks down, blocks across,
    64) in natural order over the MCU-padded component; qts: per component a (64,) table in natural order.  script: per scan a dict
    comps (indices), Ss, Se, Ah, Al and optionally dc / ac (table slot, default 0), ri (a DRI in front of the scan).  Every scan gets a DHT
    of its own in front of it (a slot that is used again is redefined).  s2: the first new coefficient of the first AC refinement is
    coded with size 2; extra_eobrun: the last EOB run of the first AC scan claims that many more blocks than its segment has."""
    from tests.jpegdec_ref import ZIGZAG
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    out = b"\xff\xd8"
    if adobe:
        out += b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
    for i, q in enumerate(qts):
        out += _seg(0xDB, bytes([i]) + bytes(int(q[z]) for z in ZIGZAG))
    out += _seg(0xC2, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([len(samp)]) + b"".join(bytes([c + 1, h << 4 | v, c]) for c, (h, v) in enumerate(samp)))
    ri, tamper = 0, {"s2": s2, "eob": extra_eobrun}
    for sc in script:
        comps, Ss, Se, Ah, Al = sc["comps"], sc["Ss"], sc["Se"], sc["Ah"], sc["Al"]
        if "ri" in sc:
            ri = sc["ri"]
            out += _seg(0xDD, ri.to_bytes(2, "big"))
        st = _Scan()
        if len(comps) > 1:
            units = [[(c, my * samp[c][1] + u // samp[c][0], mx * samp[c][0] + u % samp[c][0]) for c in comps for u in range(samp[c][0] * samp[c][1])]
                     for my in range(mcuy) for mx in range(mcux)]
        else:
            c = comps[0]
            bh, bw = -(-(-(-H * samp[c][1] // vmax)) // 8), -(-(-(-W * samp[c][0] // hmax)) // 8)
            units = [[(c, y, x)] for y in range(bh) for x in range(bw)]
        per = ri or len(units)
        state = {"eobrun": 0, "be": [], "pred": {}}

        def emit_eobrun():
            if state["eobrun"]:
                n = state["eobrun"].bit_length() - 1
                st.sym(n << 4)
                st.bits(state["eobrun"] - (1 << n), n)
                state["eobrun"] = 0
            for b in state["be"]:
                st.bits(b, 1)
            state["be"] = []

        for ui, unit in enumerate(units):
            if ui and ui % per == 0:
                emit_eobrun()
                st.tok.append(("rst",))
                state["pred"] = {}
            for c, y, x in unit:
                blk = [int(v) for v in coefs[c][y, x][ZIGZAG]]
                if Ss == 0:
                    if Ah:
                        st.bits((blk[0] >> Al) & 1, 1)
                    else:
                        v = blk[0] >> Al
                        n, e = _value(v - state["pred"].get(c, 0))
                        state["pred"][c] = v
                        st.sym(n)
                        st.bits(e, n)
                    continue
                mag = [abs(v) >> Al for v in blk]
                r = 0
                if not Ah:
                    for k in range(Ss, Se + 1):
                        if mag[k] == 0:
                            r += 1
                            continue
                        emit_eobrun()
                        while r > 15:
                            st.sym(0xF0)
                            r -= 16
                        n = mag[k].bit_length()
                        st.sym(r << 4 | n)
                        st.bits(mag[k] if blk[k] > 0 else (1 << n) - 1 - mag[k], n)
                        r = 0
                    if r:
                        state["eobrun"] += 1
                        if state["eobrun"] == 0x7FFF:
                            emit_eobrun()
                    continue
                last = max([k for k in range(Ss, Se + 1) if mag[k] == 1], default=-1)
                br = []
                for k in range(Ss, Se + 1):
                    if mag[k] == 0:
                        r += 1
                        continue
                    while r > 15 and k <= last:
                        emit_eobrun()
                        st.sym(0xF0)
                        r -= 16
                        for b in br:
                            st.bits(b, 1)
                        br = []
                    if mag[k] > 1:
                        br.append(mag[k] & 1)
                        continue
                    emit_eobrun()
                    st.sym(r << 4 | (2 if tamper["s2"] else 1))
                    tamper["s2"] = False
                    st.bits(0 if blk[k] < 0 else 1, 1)
                    for b in br:
                        st.bits(b, 1)
                    br, r = [], 0
                if r or br:
                    state["eobrun"] += 1
                    state["be"] += br
                    if state["eobrun"] == 0x7FFF or len(state["be"]) > 900:
                        emit_eobrun()
        if tamper["eob"] and Ss and not Ah:
            state["eobrun"] += tamper["eob"] if state["eobrun"] else 0
            tamper["eob"] = 0 if state["eobrun"] else tamper["eob"]
        emit_eobrun()
        dc_slot, ac_slot = sc.get("dc", 0), sc.get("ac", 0)
        if not (Ss == 0 and Ah):
            counts, used = st.table()
            out += _seg(0xC4, bytes([(0x10 | ac_slot) if Ss else dc_slot]) + bytes(counts) + bytes(used))
        out += _seg(0xDA, bytes([len(comps)]) + b"".join(bytes([c + 1, dc_slot << 4 | ac_slot]) for c in comps) + bytes((Ss, Se, Ah << 4 | Al)))
        out += st.encode()
    return out + b"\xff\xd9"


def script_of(ncomp: int, kind: str):
    """The scan scripts of the writer cases."""
    every = list(range(ncomp))
    S = lambda comps, Ss, Se, Ah, Al, **kw: dict(comps=comps, Ss=Ss, Se=Se, Ah=Ah, Al=Al, **kw)
    if kind == "dc_split":                      # per-component DC scans
        return [S([c], 0, 0, 0, 1) for c in every] + [S([c], 1, 63, 0, 0) for c in every] + [S([c], 0, 0, 1, 0) for c in every]
    if kind == "spectral_only":                 # no successive approximation
        return [S(every, 0, 0, 0, 0)] + [S([c], a, b, 0, 0) for c in every for a, b in ((1, 1), (2, 9), (10, 63))]
    if kind == "deep":                          # DC Al = 3 refined three times, AC Al = 3
        return ([S(every, 0, 0, 0, 3)] + [S([c], 1, 63, 0, 3) for c in every] + [S(every, 0, 0, 3, 2), S(every, 0, 0, 2, 1), S(every, 0, 0, 1, 0)]
                + [S([c], 1, 63, a + 1, a) for a in (2, 1, 0) for c in every])
    if kind == "tables4":                       # DHT ids 2 and 3, redefined before every scan
        return [S(every, 0, 0, 0, 0, dc=2)] + [S([c], 1, 63, 0, 1, ac=2 + c % 2) for c in every] + [S([c], 1, 63, 1, 0, ac=3 - c % 2) for c in every]
    if kind == "dri_change":                    # DRI differs between scans
        return [S(every, 0, 0, 0, 0, ri=2)] + [S([c], 1, 63, 0, 1, ri=3 + c) for c in every] + [S([c], 1, 63, 1, 0, ri=0 if c == 1 else 5) for c in every]
    if kind == "order":                         # Cb and Cr chains before Y's
        return [S(every, 0, 0, 0, 0)] + [S([c], 1, 63, 0, 1) for c in (1, 2, 0)] + [S([c], 1, 63, 1, 0) for c in (2, 1, 0)]
    if kind == "tables20":                      # 25 table versions: more than the device holds on chip, the later ones used beside the earlier ones on both levels
        bands = ((1, 1), (2, 3), (4, 6), (7, 10), (11, 20), (21, 40), (41, 63))
        return [S(every, 0, 0, 0, 0)] + [s for c in every for s in [S([c], a, b, 0, 1) for a, b in bands] + [S([c], 1, 63, 1, 0)]]
    raise KeyError(kind)
