"""TEST INFRASTRUCTURE: the progressive JPEG decoder's entropy stage restated in plain Python, as Pillow (libjpeg-turbo's jdphuff.c) runs
it: parse -> coefficients (every scan of the script, ITU-T T.81 Annex G) -> tests.jpegdec_ref's planes and pixels.  The device decoder
(csrc/jpegprog.hip) is held to it; it is itself held to the golden pixels and to live Pillow.  Independent of the product's parser.
`decode_all` counts the paths it takes (COUNTERS), so that the tests can show that the cases reach them.  Whatever libjpeg would only
warn about, or store where this statement does not, is an irregularity with an error bit (ERR): the device decoder flags such a file.
As on the device, an irregularity ends the work on its restart segment only: the other segments and the later scans still run, over
whatever coefficients are there, and the file's word is the bits of all of them.  Never imported by the product package."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from tests.jpegdec_ref import ZIGZAG, Corrupt, NotBaseline, _codes, pillow_pixels, pixels, planes  # noqa: F401

COUNTERS = ("eobrun_across_blocks", "eobrun_cut_by_restart", "zrl_first", "zrl_refine", "correction_positive", "correction_negative", "correction_zero",
            "new_positive", "new_negative", "dc_refine_one", "grid_narrower", "grid_shorter")


class NotProgressive(NotBaseline):
    """The file is outside the class the device decoder takes."""


# GAN_JPEGDEC_ERR_* / GAN_JPEGPROG_ERR_* of include/mi355x_gan.h
ERR = {"code": 1, "run": 2, "end": 4, "dc": 8, "left": 16, "rst": 32, "marker": 64, "range": 128, "refine": 256, "eobrun": 512, "coef": 1024}


class _Stop(Exception):
    """The work on the current restart segment ends (its bits are in the reader's `err`)."""


class _Reader:
    """The bits of one restart segment, most significant first, 0xFF 0x00 read as 0xFF.  Past the end the reader gives zeros and sets
    ERR["end"] when such bits are consumed; it goes on, and the caller looks at `err` where the decoder does.  A 0xFF that no 0x00
    follows flags the segment before anything is decoded (the device meets it only when its reader gets there; no test file has one)."""

    def __init__(self, raw: bytes):
        self.err, self.bits, self.pos = 0, "", 0
        if b"\xff" in raw.replace(b"\xff\x00", b""):
            self.err = ERR["marker"]
            return
        self.bits = "".join(f"{b:08b}" for b in raw.replace(b"\xff\x00", b"\xff"))

    def take(self, k: int) -> int:
        if k == 0:
            return 0
        v = int(self.bits[self.pos:self.pos + k].ljust(k, "0"), 2)
        if self.pos + k > len(self.bits):
            self.err |= ERR["end"]
            self.pos = len(self.bits)
        else:
            self.pos += k
        return v

    def symbol(self, table) -> int:
        for l in range(1, 17):
            s = table.get((l, int(self.bits[self.pos:self.pos + l].ljust(l, "0"), 2)))
            if s is not None:
                self.take(l)
                return s
        self.err |= ERR["code"]
        return 0

    def extend(self, s: int) -> int:
        if s == 0:
            return 0
        v = self.take(s)
        return v if v >= 1 << (s - 1) else v - (1 << s) + 1

    def check(self):
        if self.err:
            raise _Stop

    def fail(self, what: str):
        self.err |= ERR[what]
        raise _Stop


def real_grid(p, c):
    """(blocks down, blocks across) of component c without the MCU padding: what a single-component scan walks."""
    h, v = p.comps[c][:2]
    return -(-(-(-p.H * v // p.vmax)) // 8), -(-(-(-p.W * h // p.hmax)) // 8)


def parse(data: bytes) -> SimpleNamespace:
    """H, W, comps [(h, v, quant table)], and the scans in file order: comp (-1: all interleaved), Ss, Se, Ah, Al, tables {component:
    (counts, symbols)}, per (restart interval in the scan's units), units, segments [(first byte, end)]."""
    if data[:2] != b"\xff\xd8":
        raise NotProgressive("no SOI")
    pos, qt, dht, p, ri, scans = 2, {}, {}, None, 0, []
    while True:
        if pos + 2 > len(data) or data[pos] != 0xFF:
            raise NotProgressive("marker expected")
        m = data[pos + 1]
        if m == 0xD9:
            break
        L = int.from_bytes(data[pos + 2:pos + 4], "big")
        if L < 2 or pos + 2 + L > len(data):
            raise NotProgressive("truncated")
        body = data[pos + 4:pos + 2 + L]
        pos += 2 + L
        if m == 0xDB:
            while body:
                if body[0] >> 4:
                    raise NotProgressive("16-bit quantisation table")
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = list(body[1:65])
                qt[body[0] & 15], body = q, body[65:]
        elif m == 0xC4:
            while body:
                n = sum(body[1:17])
                dht[body[0]], body = (list(body[1:17]), list(body[17:17 + n])), body[17 + n:]
        elif m == 0xC2:
            if body[0] != 8:
                raise NotProgressive("not 8-bit")
            H, W, nc = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            ids = [body[6 + 3 * c] for c in range(nc)]
            samp = [(body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15) for c in range(nc)]
            if not ((nc == 1 and samp == [(1, 1)]) or (nc == 3 and samp[1:] == [(1, 1), (1, 1)] and samp[0] in ((1, 1), (2, 1), (2, 2)) and ids == [1, 2, 3])):
                raise NotProgressive(f"components {samp}")
            hmax, vmax = samp[0]
            p = SimpleNamespace(H=H, W=W, hmax=hmax, vmax=vmax, mcux=-(-W // (8 * hmax)), mcuy=-(-H // (8 * vmax)),
                                comps=[(h, v, qt[body[8 + 3 * c]]) for c, (h, v) in enumerate(samp)], scans=scans, data=data)
        elif m == 0xDD:
            ri = int.from_bytes(body[:2], "big")
        elif m == 0xEE and body[:5] == b"Adobe":
            raise NotProgressive("Adobe marker")
        elif m == 0xDA:
            if p is None:
                raise NotProgressive("no SOF2")
            ns, (Ss, Se, AhAl) = body[0], body[-3:]
            members = [ids.index(body[1 + 2 * j]) for j in range(ns)]
            if ns != 1 and (members != list(range(nc)) or Ss):
                raise NotProgressive("a scan of some of the components, or an AC scan of several")
            comp = members[0] if ns == 1 else -1
            tables = {}
            for j, c in enumerate(members):
                sel = body[2 + 2 * j]
                if Ss:
                    tables[c] = dht[0x10 | (sel & 15)]
                elif not AhAl >> 4:
                    tables[c] = dht[sel >> 4]
            begin, cuts = pos, []
            while True:                        # up to the first marker that is neither a stuffed byte nor RSTn
                pos = data.find(b"\xff", pos)
                if pos < 0 or pos + 1 >= len(data):
                    raise NotProgressive("no marker after the scan")
                if data[pos + 1] == 0:
                    pos += 2
                elif 0xD0 <= data[pos + 1] <= 0xD7:
                    cuts.append(pos)
                    pos += 2
                else:
                    break
            units = p.mcux * p.mcuy if comp < 0 else int(np.prod(real_grid(p, comp)))
            per = ri or units
            if len(cuts) != -(-units // per) - 1:
                raise NotProgressive("restart markers do not match the interval")
            scans.append(SimpleNamespace(comp=comp, Ss=Ss, Se=Se, Ah=AhAl >> 4, Al=AhAl & 15, tables=tables, per=per, units=units,
                                         segments=list(zip([begin] + [c + 2 for c in cuts], cuts + [pos]))))
        elif not (0xE0 <= m <= 0xEF or m == 0xFE):
            raise NotProgressive(f"marker {m:#x}")
    if p is None or not scans:
        raise NotProgressive("no scans")
    return p


def _int16(v) -> bool:
    return -32768 <= v <= 32767


def _correct(bits, blk, k, p1, cnt):
    """The correction bit of the already-nonzero coefficient k; a value that leaves int16 sets its bit and the block goes on."""
    if not bits.take(1):
        cnt["correction_zero"] += not bits.err
        return
    c = int(blk[ZIGZAG[k]])
    if c & p1:
        return
    v = c + p1 if c >= 0 else c - p1
    if not _int16(v):
        bits.err |= ERR["coef"]
        return
    cnt["correction_positive" if c >= 0 else "correction_negative"] += 1
    blk[ZIGZAG[k]] = v


def _dc_first(bits, table, pred, Al, blk):
    s = bits.symbol(table)
    if s > 15:
        bits.err |= ERR["code"]
    bits.check()
    pred += bits.extend(s)
    if not _int16(pred):
        bits.err |= ERR["dc"]
    bits.check()
    if not _int16(pred * (1 << Al)):
        bits.fail("coef")
    blk[0] = pred * (1 << Al)
    return pred


def _dc_refine(bits, Al, blk, cnt):
    if bits.take(1):
        cnt["dc_refine_one"] += 1
        blk[0] |= np.int16(1 << Al)
    bits.check()


def _ac_first(bits, table, sc, eobrun, blk, cnt):
    """-> the EOB run after this block."""
    if eobrun > 0:
        return eobrun - 1
    k = sc.Ss
    while k <= sc.Se:
        rs = bits.symbol(table)
        bits.check()
        r, s = rs >> 4, rs & 15
        if s:
            k += r
            if k > sc.Se:
                bits.fail("run")
            v = bits.extend(s) * (1 << sc.Al)
            bits.check()
            if not _int16(v):
                bits.fail("coef")
            blk[ZIGZAG[k]] = v
        elif r == 15:
            cnt["zrl_first"] += 1
            k += 15
        else:
            run = (1 << r) + bits.take(r) - 1
            bits.check()
            return run
        k += 1
    return 0


def _ac_refine(bits, table, sc, eobrun, blk, cnt):
    p1, k = 1 << sc.Al, sc.Ss
    if eobrun == 0:
        while k <= sc.Se:
            rs = bits.symbol(table)
            bits.check()
            r, s, new = rs >> 4, rs & 15, 0
            if s:
                if s != 1:
                    bits.fail("refine")
                new = p1 if bits.take(1) else -p1
                cnt["new_positive" if new > 0 else "new_negative"] += 1
            elif r != 15:
                eobrun = (1 << r) + bits.take(r)
                break
            else:
                cnt["zrl_refine"] += 1
            while k <= sc.Se:                  # over the nonzero coefficients (a correction bit each) and r zero ones
                if blk[ZIGZAG[k]] != 0:
                    _correct(bits, blk, k, p1, cnt)
                else:
                    r -= 1
                    if r < 0:
                        break
                k += 1
            bits.check()
            if new:
                if k > sc.Se:
                    bits.fail("run")
                blk[ZIGZAG[k]] = new
            k += 1
        bits.check()
    if eobrun > 0:
        while k <= sc.Se:
            if blk[ZIGZAG[k]] != 0:
                _correct(bits, blk, k, p1, cnt)
            k += 1
        eobrun -= 1
    bits.check()
    return eobrun


def decode_segment(p, sc, j, tables, out, cnt) -> int:
    """Restart segment j of scan sc into `out` -> its error bits."""
    b, e = sc.segments[j]
    if j and p.data[b - 2:b] != bytes((0xFF, 0xD0 + (j - 1) % 8)):
        return ERR["rst"]
    bits = _Reader(p.data[b:e])
    try:
        bits.check()
        first, last = j * sc.per, min((j + 1) * sc.per, sc.units)
        if sc.comp < 0:
            pred = [0] * len(p.comps)
            for mcu in range(first, last):
                my, mx = divmod(mcu, p.mcux)
                for c, (h, v, *_) in enumerate(p.comps):
                    for u in range(h * v):
                        blk = out[c][my * v + u // h, mx * h + u % h]
                        if sc.Ah:
                            _dc_refine(bits, sc.Al, blk, cnt)
                        else:
                            pred[c] = _dc_first(bits, tables[c], pred[c], sc.Al, blk)
        else:
            bw = real_grid(p, sc.comp)[1]
            pred = eobrun = 0
            for n in range(first, last):
                blk = out[sc.comp][n // bw, n % bw]
                if sc.Ss == 0:
                    if sc.Ah:
                        _dc_refine(bits, sc.Al, blk, cnt)
                    else:
                        pred = _dc_first(bits, tables[sc.comp], pred, sc.Al, blk)
                    continue
                before = eobrun
                eobrun = (_ac_refine if sc.Ah else _ac_first)(bits, tables[sc.comp], sc, eobrun, blk, cnt)
                if before == 0 and eobrun > 0:
                    cnt["eobrun_across_blocks"] += 1
                    cnt["eobrun_cut_by_restart"] += n + eobrun == last - 1 and last < sc.units
            if eobrun > 0:
                bits.fail("eobrun")
        if len(bits.bits) - bits.pos >= 8:
            bits.fail("left")
    except _Stop:
        pass
    return bits.err


def decode_all(p, counters=None):
    """Every segment of every scan, in file order -> (per component an int16 array (blocks down, blocks across, 64) in natural order over
    the MCU-padded component, the file's error word).  counters: a dict that receives how often each path of COUNTERS was taken."""
    out = [np.zeros((p.mcuy * v, p.mcux * h, 64), np.int16) for h, v, *_ in p.comps]
    cnt = dict.fromkeys(COUNTERS, 0)
    word = 0
    for sc in p.scans:
        tables = {c: _codes(*t) for c, t in sc.tables.items()}
        if sc.comp >= 0:
            bh, bw = real_grid(p, sc.comp)
            cnt["grid_narrower"] += bw < out[sc.comp].shape[1]
            cnt["grid_shorter"] += bh < out[sc.comp].shape[0]
        for j in range(len(sc.segments)):
            word |= decode_segment(p, sc, j, tables, out, cnt)
    if counters is not None:
        for k, v in cnt.items():
            counters[k] = counters.get(k, 0) + int(v)
    return out, word


def coefficients(p, counters=None) -> list:
    """decode_all's coefficients; Corrupt (with the word as `.word`) when the entropy stage flags the file."""
    out, word = decode_all(p, counters)
    if word:
        e = Corrupt(f"error word {word}")
        e.word = word
        raise e
    return out


def expectation(data: bytes):
    """(error word, pixels): what the device decoder must report for a file its parser takes -- the entropy stage's bits, and the IDCT's
    RANGE bit over whatever coefficients the entropy stage left.  The pixels count only where the word is 0."""
    p = parse(data)
    co, word = decode_all(p)
    pl, extreme = planes(p, co)
    return word | (ERR["range"] if extreme else 0), pixels(p, pl)


def stages(data: bytes, counters=None) -> SimpleNamespace:
    p = parse(data)
    co = coefficients(p, counters)
    pl, extreme = planes(p, co)
    return SimpleNamespace(plan=p, coefs=co, planes=pl, extreme=extreme, pixels=pixels(p, pl))


def decode(data: bytes) -> np.ndarray:
    return stages(data).pixels
