"""TEST INFRASTRUCTURE: the edge cases of the device input pipeline (csrc/input_pipeline.hip), built on the host.

Every builder returns what a test feeds to `dataio.InputPipeline` (uint8 HWC images as numpy arrays, job dicts from `dataio._job`)
and the property the case was built for, which tests/test_input_pipeline_edges_cpu.py checks.  The reference of every comparison is
Pillow itself (`pil_apply`, which is `oracle.input_ref.apply_pil` for BICUBIC); the numpy restatement `oracle.input_ref.apply` is the
second witness on the CPU.  `apply_mut` is that restatement with one arithmetic step mutated: it exists to show which case notices
which mistake (the counts are measured on it, never on a kernel).

Pure numpy, torch-CPU and Pillow: nothing here touches a GPU."""
from __future__ import annotations

import itertools
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np

from gan_variant_research_amd import dataio
from oracle import input_ref as R

BILINEAR, BICUBIC = dataio.BILINEAR, dataio.BICUBIC
f32, f64 = np.float32, np.float64

# float32 factors, held as the Python floats a job carries: Pillow, the restatement and the job struct all round to the same value
UP1 = float(np.nextafter(f32(1), f32(2)))
DOWN1 = float(np.nextafter(f32(1), f32(0)))
F095, F105 = float(f32(0.95)), float(f32(1.05))
NO_JITTER = (-1, -1, -1, -1)


def job(h, w, S, crop=None, resize=None, window=None, flip=False, order=NO_JITTER, factor=(1.0, 1.0, 1.0, 0.0)) -> Dict:
    """`dataio.eval_job(h, w, S)` (whole image -> S x S) with the fields a case sets replaced."""
    return dataio._job(h, w, crop or (0, 0, h, w), resize or (S, S), window or (0, 0, S, S), flip, order, factor)


def one_op(op: int, value: float) -> Tuple[Tuple[int, ...], Tuple[float, ...]]:
    """(order, factor) of a job that runs the single jitter op `op` with `value`."""
    factor = [1.0, 1.0, 1.0, 0.0]
    factor[op] = value
    return (op, -1, -1, -1), tuple(factor)


# ------------------------------------------------------------------------------------------------ the references
def pil_apply(img: np.ndarray, jb: Dict, filter: int = BICUBIC) -> np.ndarray:
    """One image through a job by Pillow: float32 (3, S, S).  BICUBIC is `R.apply_pil` itself; BILINEAR (the inference resize, never
    followed by jitter) is Image.resize(..., BILINEAR) then `to_tensor_normalize`, with apply_pil's crop, window and flip calls."""
    if filter == BICUBIC:
        return R.apply_pil(img, jb)
    from PIL import Image
    assert filter == BILINEAR and jb["order"] == NO_JITTER
    cy, cx, ch, cw = jb["crop"]
    im = Image.fromarray(img, "RGB").crop((cx, cy, cx + cw, cy + ch))
    im = im.resize((jb["resize"][1], jb["resize"][0]), Image.BILINEAR)
    oy, ox, oh, ow = jb["window"]
    im = im.crop((ox, oy, ox + ow, oy + oh))
    if jb["flip"]:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return R.to_tensor_normalize(np.asarray(im))


@lru_cache(maxsize=None)
def _unit_lut() -> np.ndarray:
    lut = R.to_tensor_normalize(np.arange(256, dtype=np.uint8).reshape(1, 256, 1)).reshape(-1)
    assert np.all(np.diff(lut) > 0)
    return lut


def to_bytes(x: np.ndarray) -> np.ndarray:
    """The bytes behind a `to_tensor_normalize` result: the map is strictly increasing on 0..255, so it inverts exactly.  This is how
    the uint8 output is held to `apply_pil` without restating its Pillow calls."""
    lut = _unit_lut()
    idx = np.clip(np.searchsorted(lut, x), 0, 255)
    assert np.array_equal(lut[idx], x)
    return idx.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the blend and its fused form
def blend_pairs(alpha, fused: bool) -> np.ndarray:
    """Blend.c over every (in1, in2) byte pair -> [..., in1, in2]; `alpha` a float32 or an array of them.  fused=True rounds
    in1 + alpha * (in2 - in1) once: the sum is exact in float64 (24 + 9 bits of product, aligned with an 8-bit integer)."""
    a = np.asarray(alpha, f32).reshape(-1, 1, 1)
    in1 = np.arange(256, dtype=np.int32).reshape(1, 256, 1)
    d = np.arange(256, dtype=np.int32).reshape(1, 1, 256) - in1
    if fused:
        t = (in1.astype(f64) + a.astype(f64) * d.astype(f64)).astype(f32)
    else:
        t = in1.astype(f32) + a * d.astype(f32)
    inside = (a >= 0) & (a <= 1)
    out = np.where(inside, t.astype(np.int32) & 255, np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))))
    return out.astype(np.uint8).reshape(np.shape(alpha) + (256, 256))


def sensitive_pairs(alpha) -> np.ndarray:
    """bool [..., in1, in2]: the byte pairs on which a fused multiply-add in the blend changes the output byte."""
    return blend_pairs(alpha, False) != blend_pairs(alpha, True)


SEARCH_SEED, SEARCH_DRAWS, SEARCH_CHUNK, MIN_PAIRS = 20261020, 16384, 64, 50
_IN1 = np.arange(256, dtype=f64).reshape(1, 256, 1)
_DIFF = np.arange(256, dtype=f64).reshape(1, 1, 256) - _IN1


def _differing_sums(a: np.ndarray) -> np.ndarray:
    """bool [n, in1, in2]: where the float32 sum of the two-rounding form and of the fused form differ (a superset of the sensitive
    pairs, and cheap: the search looks at bytes only where this holds)."""
    a = a.reshape(-1, 1, 1)
    two = _IN1.astype(f32) + a * _DIFF.astype(f32)
    return two != (_IN1 + a.astype(f64) * _DIFF).astype(f32)


@lru_cache(maxsize=None)
def searched_factors(count: int = 2) -> Tuple[float, ...]:
    """The seeded search: float32 factors drawn uniformly from the product's range [0.95, 1.05]; the first `count`, in draw order,
    whose fused form changes at least MIN_PAIRS byte pairs.  About one draw in 700 changes any pair at all."""
    rng = np.random.default_rng(SEARCH_SEED)
    found = []
    for _ in range(SEARCH_DRAWS // SEARCH_CHUNK):
        a = rng.uniform(0.95, 1.05, SEARCH_CHUNK).astype(f32)
        for i in np.flatnonzero(_differing_sums(a).any(axis=(1, 2))):
            if int(sensitive_pairs(a[i]).sum()) >= MIN_PAIRS:
                found.append(float(a[i]))
        if len(found) >= count:
            return tuple(found[:count])
    raise AssertionError(f"the seeded search found {len(found)} factors with {MIN_PAIRS} sensitive pairs in {SEARCH_DRAWS} draws")


def searched_for_row(in1: int, in2_present: np.ndarray) -> Optional[float]:
    """A directed search for one row of the pair table: the first float32 factor in [0.95, 1.05] with a sensitive pair (in1, in2) for
    an in2 among `in2_present`, or None.  The sensitive factors are float32 neighbours of the fractions k / |in2 - in1| (there the
    product lands within a rounding of an integer), so those are the candidates, from the widest difference down."""
    vals = np.unique(in2_present).astype(np.int64)
    for v in sorted(vals, key=lambda v: -abs(int(v) - in1)):
        d = abs(int(v) - in1)
        if d < 3:
            continue
        cand = []
        for k in range(int(np.ceil(0.95 * d)), int(np.floor(1.05 * d)) + 1):
            base = f32(k / d)
            lo, hi = base, base
            cand.append(base)
            for _ in range(3):
                lo, hi = np.nextafter(lo, f32(0)), np.nextafter(hi, f32(2))
                cand += [lo, hi]
        cand = np.array([c for c in cand if f32(0.95) <= c <= f32(1.05)], f32)
        a64, x1, dd = cand.astype(f64), f64(in1), f64(int(v) - in1)
        two = (f32(in1) + cand * f32(int(v) - in1)).astype(f32)
        one = (x1 + a64 * dd).astype(f32)
        for i in np.flatnonzero(two != one):
            if sensitive_pairs(cand[i])[in1, int(v)]:
                return float(cand[i])
    return None


def sensitive_set() -> Tuple[float, ...]:
    """Blend factors for the mixed batches: the ones a fused blend cannot survive, and the range's ends."""
    return (UP1,) + searched_factors() + (F095, F105, DOWN1)


# ------------------------------------------------------------------------------------------------ 1. the colour cube
CUBE_S = 256
HUE_SHIFTS = (0, 1, 2, 3, 4, 5, 251, 252, 253, 254, 255, 43, 128, 213)       # the eleven ColorJitter(hue=0.02) can draw, and three more
SATURATION_FIXED = {"up1": UP1, "down1": DOWN1, "0.95": F095, "1.05": F105, "0": 0.0, "2": 2.0}
SATURATION_IDS = tuple(SATURATION_FIXED) + ("searched0", "searched1")
BRIGHTNESS = {"0.95": F095, "1.05": F105, "2": 2.0}


def saturation_factor(name: str) -> float:
    return SATURATION_FIXED[name] if name in SATURATION_FIXED else searched_factors()[int(name[len("searched"):])]


def hue_factor(shift: int) -> float:
    """A hue factor that `int(f * 255) % 256` turns into `shift` (negative for the upper half, as the product's draws are)."""
    f = (shift + 0.5) / 255.0 if shift <= 128 else (shift - 256 - 0.5) / 255.0
    assert int(f * 255) % 256 == shift == R.hue_shift(f)
    return f


@lru_cache(maxsize=None)
def cube() -> np.ndarray:
    """uint8 [256][256][256][3]: image r holds every (r, g, b), g down the rows and b along them."""
    v = np.arange(256, dtype=np.uint8)
    r, g, b = np.meshgrid(v, v, v, indexing="ij")
    return np.ascontiguousarray(np.stack([r, g, b], -1))


def cube_jobs(op: int, value: float, n: int = 256) -> List[Dict]:
    """Identity geometry: at scale 1 the bicubic taps are exactly 1 << 22 at the centre, so the jitter kernel sees the cube's bytes."""
    order, factor = one_op(op, value)
    return [job(CUBE_S, CUBE_S, CUBE_S, order=order, factor=factor) for _ in range(n)]


def identity_taps_are_exact() -> bool:
    bounds, kk = R.resize_coeffs(CUBE_S, 0, CUBE_S, CUBE_S)
    centre = kk[np.arange(CUBE_S), np.arange(CUBE_S) - bounds[:, 0]]
    return bool(np.all(centre == 1 << R.PRECISION_BITS) and kk.sum() == CUBE_S << R.PRECISION_BITS and np.count_nonzero(kk) == CUBE_S)


def _as_image(c: np.ndarray):
    from PIL import Image
    return Image.fromarray(c.reshape(-1, c.shape[-2], 3), "RGB")


def cube_pil_hsv():
    """Pillow's RGB -> HSV of the whole cube (one call on the 256 images stacked: the conversion is per pixel)."""
    return _as_image(cube()).convert("HSV").split()


def cube_pil_hue(hsv, shift: int) -> np.ndarray:
    """apply_pil's hue branch on the cube, from Pillow's HSV planes: uint8 like cube()."""
    from PIL import Image
    h, s, v = hsv
    np_h = (np.array(h, dtype=np.uint8).astype(np.int32) + shift).astype(np.uint8)
    return np.asarray(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")).reshape(cube().shape)


def cube_pil_enhance(op: int, value: float, c: Optional[np.ndarray] = None) -> np.ndarray:
    """apply_pil's brightness / saturation branch on the cube (per pixel, so one call on the stacked images)."""
    from PIL import ImageEnhance
    c = cube() if c is None else c
    enh = {0: ImageEnhance.Brightness, 2: ImageEnhance.Color}[op]
    return np.asarray(enh(_as_image(c)).enhance(value)).reshape(c.shape)


def nchw(c: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.moveaxis(c, -1, -3))


# ------------------------------------------------------------------------------------------------ 2. the contrast mean at a tie
MEAN_S = 16
MEAN_TARGETS = (0, 1, 31, 127, 128, 200, 254)


def luma_sum(img: np.ndarray) -> int:
    return int(R.to_gray(img).astype(np.int64).sum())


def _luma1(p) -> int:
    return (int(p[0]) * 19595 + int(p[1]) * 38470 + int(p[2]) * 7471 + 0x8000) >> 16


def _walk_to_sum(img: np.ndarray, T: int, rng, frozen: int = -1) -> np.ndarray:
    """Single-byte steps at random pixels (never the `frozen` one) until the luma sum is exactly T."""
    flat = img.reshape(-1, 3)
    s = luma_sum(img)
    while s != T:
        i, c = int(rng.integers(len(flat))), int(rng.integers(3))
        if i == frozen:
            continue
        v = int(flat[i, c]) + (1 if s < T else -1)
        if not 0 <= v <= 255:
            continue
        before = _luma1(flat[i])
        flat[i, c] = v
        s += _luma1(flat[i]) - before
    return img


def _heavy_tail_image(T: int, rng) -> np.ndarray:
    """256 arbitrary colours whose lumas sum to T: up to twelve pixels with one bright channel (a dark image still holds large bytes,
    which the blend needs to be sensitive), random hues with a heavy-tailed split of the rest of T among the other pixels, then the
    walk."""
    n = MEAN_S * MEAN_S
    weight = np.array([0.299, 0.587, 0.114])
    flat = np.zeros((n, 3), np.uint8)
    spikes = rng.permutation(n)[:12]
    budget = 0.8 * T
    for i in spikes:
        c, v = int(rng.integers(3)), int(rng.integers(64, 256))
        if v * weight[c] <= budget:
            flat[i, c] = v
            budget -= v * weight[c]
    rest = np.setdiff1d(np.arange(n), spikes)
    w = rng.exponential(1.0, len(rest)) ** 3
    target = np.minimum(255.0, max(T - luma_sum(flat.reshape(1, n, 3)), 0) * w / w.sum())
    col = rng.integers(0, 256, (len(rest), 3)).astype(f64)
    flat[rest] = np.clip(np.rint(col * (target / np.maximum(col @ weight, 1.0))[:, None]), 0, 255).astype(np.uint8)
    return _walk_to_sum(flat.reshape(MEAN_S, MEAN_S, 3), T, rng)


def _permutation_image(T: int, rng) -> np.ndarray:
    """Every byte value once in every channel; swaps inside a channel move the luma sum by its rounding only, until it is T."""
    flat = np.stack([rng.permutation(256) for _ in range(3)], -1).astype(np.uint8)
    s = luma_sum(flat.reshape(MEAN_S, MEAN_S, 3))
    while s != T:
        i, k, c = int(rng.integers(256)), int(rng.integers(256)), int(rng.integers(3))
        before = _luma1(flat[i]) + _luma1(flat[k])
        flat[[i, k], c] = flat[[k, i], c]
        s2 = s + _luma1(flat[i]) + _luma1(flat[k]) - before
        if abs(s2 - T) <= abs(s - T):
            s = s2
        else:
            flat[[i, k], c] = flat[[k, i], c]
    return flat.reshape(MEAN_S, MEAN_S, 3)


@lru_cache(maxsize=None)
def mean_images() -> Tuple[Dict, ...]:
    """Per target mean d two 16x16 images (n = 256): luma sum 256 d + 128 (a tie: int(t / n + 0.5) = d + 1) and 256 d + 127 (one below
    it: d).  With 256 pixels every byte value can appear in every channel only where the luma sum is that of three permutations,
    32640 +- rounding, which is d = 127's pair exactly; the other images hold arbitrary colours with as wide a spread of bytes as
    their sum allows (`all_bytes` says which).

    Each image carries `searched`: an in-range factor whose sensitive pairs include (mean, in2) for a byte in2 of the image.  The
    very dark and very bright images hold too few bytes for one to exist, so the factor is searched over the whole row and its in2
    is planted in the blue channel of pixel 0 (the cheapest in luma) before the walk to the sum.  Row 0 has no sensitive pair for any
    factor (in1 = 0 leaves one rounding, as in brightness): the image with mean 0 takes its tie sibling's factor."""
    rng = np.random.default_rng(2)
    out = []
    for d in MEAN_TARGETS:
        for tie in (True, False):
            T, mean = 256 * d + (128 if tie else 127), d + 1 if tie else d
            if d == 127:
                img = _permutation_image(T, rng)
                searched = searched_for_row(mean, img)
            else:
                img = _heavy_tail_image(T, rng) if d < 128 else 255 - _heavy_tail_image(255 * 256 - T, rng)
                searched = searched_for_row(mean, np.arange(256)) if mean > 0 else out[-1]["searched"]
                if mean > 0:
                    img[0, 0, 2] = np.flatnonzero(sensitive_pairs(searched)[mean])[0]
                img = _walk_to_sum(img, T, rng, frozen=0)
            assert searched is not None, f"no factor in [0.95, 1.05] is sensitive in row {mean}"
            out.append({"d": d, "tie": tie, "sum": T, "mean": mean, "image": img, "searched": searched,
                        "all_bytes": all(len(np.unique(img[..., c])) == 256 for c in range(3))})
    return tuple(out)


def mean_batch() -> Tuple[List[np.ndarray], List[Dict], List[Dict]]:
    """(images, jobs, meta): every image of mean_images() under contrast with nextafter(1, 2), its searched factor and 0.95."""
    images, jobs, meta = [], [], []
    for m in mean_images():
        for name, a in (("up1", UP1), ("searched", m["searched"]), ("0.95", F095)):
            order, factor = one_op(1, a)
            images.append(m["image"])
            jobs.append(job(MEAN_S, MEAN_S, MEAN_S, order=order, factor=factor))
            meta.append({"d": m["d"], "tie": m["tie"], "mean": m["mean"], "factor": name})
    return images, jobs, meta


# ------------------------------------------------------------------------------------------------ 3. geometry
GEOMETRY = {1: ((1, 1), (7, 5), (300, 2), (250, 2)),
            5: ((1, 1), (2, 3), (5, 5), (4, 6), (9, 300), (300, 9), (200, 2), (201, 2)),
            17: ((16, 16), (17, 17), (18, 18), (33, 35), (2000, 17))}       # 2000 -> 17: 473 bicubic taps, more rows than the buffer's 1024
# "checker" is the one-pixel 0/255 checkerboard: its bicubic accumulator leaves [0, 255] on both sides where the image is enlarged; a
# reduction averages it to grey.  "blocks" is the same board with cells two output pixels wide, which overshoots when reduced.
CONTENTS = ("random", "zeros", "ones", "checker", "blocks")
# (300, 2), (250, 2) and (201, 2) are more than 100 times taller than wide and are lowered: Pillow makes their vertical pass first, and
# the rounded bytes between the passes make the order visible; (200, 2) is the last size in the usual order.  Tall sources that are not
# lowered, which keep the usual order, are in crop_batch().
GEOMETRY_MAX_BATCH = 96
# The tap generator holds at most 1024 taps per output pixel and refuses a longer kernel ("downscale factor too large").  300 -> 1 needs
# 1201 bicubic taps (601 bilinear), so the pipeline must refuse (300, 2) -> 1 x 1 under BICUBIC; (250, 2), with 1001, is the tall
# source that BICUBIC can take at S = 1.
MAX_TAPS = 1024


def tap_count(in_size: int, out_size: int, filter: int) -> int:
    """Resample.c precompute_coeffs' ksize."""
    support = {BILINEAR: 1.0, BICUBIC: 2.0}[filter] * max(in_size / out_size, 1.0)
    return int(np.ceil(support)) * 2 + 1


def supported(jb: Dict, filter: int) -> bool:
    return max(tap_count(jb["crop"][2], jb["resize"][0], filter), tap_count(jb["crop"][3], jb["resize"][1], filter)) <= MAX_TAPS


def content(kind: str, h: int, w: int, rng, S: int = 1) -> np.ndarray:
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "ones":
        return np.full((h, w, 3), 255, np.uint8)
    cy, cx = (1, 1) if kind == "checker" else (max(1, -(-2 * h // S)), max(1, -(-2 * w // S)))
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy // cy + xx // cx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


@lru_cache(maxsize=None)
def geometry_batch(S: int) -> Tuple[List[np.ndarray], List[Dict], List[Tuple]]:
    """(images, jobs, meta) for one output size: every source size x content x flip, whole image -> S x S, no jitter."""
    rng = np.random.default_rng(300 + S)
    images, jobs, meta = [], [], []
    for (h, w) in GEOMETRY[S]:
        for kind in CONTENTS:
            img = content(kind, h, w, rng, S)
            for flip in (False, True):
                images.append(img)
                jobs.append(job(h, w, S, flip=flip))
                meta.append((h, w, kind, flip))
    return images, jobs, meta


# ------------------------------------------------------------------------------------------------ 4. crop, stride and window
CROP_S = 16
PAD_ROWS, PAD_COLS, PAD_Y0, PAD_X0 = 7, 5, 3, 2


def embed(img: np.ndarray) -> Tuple[np.ndarray, Tuple[int, int]]:
    """(big, (y0, x0)): `img` as big[y0:y0+H, x0:x0+W] of a tensor 7 rows and 5 columns larger whose every byte outside the image is
    255 - the mirrored value, so that a read past the slice, on any side, changes the result."""
    H, W = img.shape[:2]
    yy = np.arange(-PAD_Y0, H + PAD_ROWS - PAD_Y0)
    xx = np.arange(-PAD_X0, W + PAD_COLS - PAD_X0)
    mirror = lambda i, n: np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i)) % n
    big = 255 - img[mirror(yy, H)][:, mirror(xx, W)]
    big[PAD_Y0:PAD_Y0 + H, PAD_X0:PAD_X0 + W] = img
    return np.ascontiguousarray(big), (PAD_Y0, PAD_X0)


@lru_cache(maxsize=None)
def crop_batch() -> Tuple[List[np.ndarray], List[Dict], List[str]]:
    """Train-style jobs (square crop -> 16 x 16, flip, all four jitter ops) on a 23 x 29 image: the crop in the first corner, in the
    last (touching the last row and column), and a single pixel in three places; then basic-style jobs on a 20 x 33 image resized to
    19 x 31 with the 16 x 16 window in each corner of the resized image."""
    rng = np.random.default_rng(4)
    H, W, cs = 23, 29, 13
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (20, 33, 3), dtype=np.uint8)
    fs = sensitive_set()
    perms = list(itertools.permutations(range(4)))
    images, jobs, names = [], [], []
    crops = [("crop.first", (0, 0, cs, cs)), ("crop.last", (H - cs, W - cs, cs, cs)), ("crop.pixel.first", (0, 0, 1, 1)),
             ("crop.pixel.last", (H - 1, W - 1, 1, 1)), ("crop.pixel.inside", (11, 17, 1, 1))]
    for i, (name, crop) in enumerate(crops):
        images.append(a)
        jobs.append(job(H, W, CROP_S, crop=crop, flip=i % 2 == 0, order=perms[5 * i + 3],
                        factor=(fs[i % len(fs)], fs[(i + 1) % len(fs)], fs[(i + 2) % len(fs)], hue_factor(HUE_SHIFTS[3 + i]))))
        names.append(name)
    # a crop more than 100 times taller than wide out of an image that is not: the pass order follows the crop, as Pillow's does
    tall = rng.integers(0, 256, (310, 9, 3), dtype=np.uint8)
    for name, crop in (("crop.tall.301x3", (7, 5, 301, 3)), ("crop.tall.300x3", (8, 4, 300, 3))):
        images.append(tall)
        jobs.append(job(310, 9, CROP_S, crop=crop, flip=name.endswith("301x3")))
        names.append(name)
    # tall sources whose height grows, stays, or shrinks by one row (basic-style: a window of the resized image): Pillow takes the
    # vertical pass first only for the last
    thin = rng.integers(0, 256, (201, 2, 3), dtype=np.uint8)
    for i, (rh, rw) in enumerate(((256, 17), (286, 16), (201, 16), (202, 18), (200, 16))):
        images.append(thin)
        jobs.append(job(201, 2, CROP_S, resize=(rh, rw), window=(rh - CROP_S - 3 * i, rw - CROP_S, CROP_S, CROP_S), flip=i % 2 == 0))
        names.append(f"tall.201x2.to.{rh}x{rw}")
    for i, (oy, ox) in enumerate(((0, 0), (0, 31 - CROP_S), (19 - CROP_S, 0), (19 - CROP_S, 31 - CROP_S))):
        images.append(b)
        jobs.append(job(20, 33, CROP_S, resize=(19, 31), window=(oy, ox, CROP_S, CROP_S), flip=i % 2 == 1))
        names.append(f"window.{oy}.{ox}")
    return images, jobs, names


# ------------------------------------------------------------------------------------------------ 5. the mixed batch
MIXED_S, MIXED_B = 16, 32


@lru_cache(maxsize=None)
def mixed_batch() -> Tuple[List[np.ndarray], List[Dict]]:
    """32 jobs: the 24 orders of the four jitter ops, a job without jitter at every fourth place, flips alternating, blend factors
    from the sensitive set, hue shifts from the product's eleven; sources of differing sizes with train-style square crops."""
    rng = np.random.default_rng(5)
    perms = iter(itertools.permutations(range(4)))
    fs = sensitive_set()
    images, jobs = [], []
    for i in range(MIXED_B):
        h, w = int(rng.integers(16, 41)), int(rng.integers(16, 41))
        cs = int(min(h, w) * rng.uniform(0.85, 1.0))
        cy, cx = int(rng.integers(0, h - cs + 1)), int(rng.integers(0, w - cs + 1))
        if i % 4 == 3:
            order, factor = NO_JITTER, (1.0, 1.0, 1.0, 0.0)
        else:
            order = next(perms)
            factor = (fs[i % len(fs)], fs[(i + 2) % len(fs)], fs[(i + 4) % len(fs)], hue_factor(HUE_SHIFTS[i % 11]))
        images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        jobs.append(job(h, w, MIXED_S, crop=(cy, cx, cs, cs), flip=i % 2 == 1, order=order, factor=factor))
    assert sorted(j["order"] for j in jobs if j["order"] != NO_JITTER) == sorted(itertools.permutations(range(4)))
    return images, jobs


# ------------------------------------------------------------------------------------------------ 6. reuse
REUSE_S, REUSE_MAX_BATCH, REUSE_MAX_ROWS = 16, 8, 32
FIRST_BLOCK_BYTES = 1 << 16          # InputPipeline's smallest table block


@lru_cache(maxsize=None)
def reuse_batches() -> Tuple[Tuple[List[np.ndarray], List[Dict]], ...]:
    """Three batches for one pipeline built with max_batch 8 and max_rows 32: the first fits; the second holds a 700-row image (the
    buffer between the passes grows); the third holds eight images of sixteen distinct edge lengths (its tap tables outgrow the
    first table block).  All carry contrast, so the mean workspace is shared too."""
    rng = np.random.default_rng(6)
    fs = sensitive_set()
    sizes = ([(20, 24), (32, 17), (16, 16), (25, 31)],
             [(700, 40), (30, 30), (64, 21)],
             [(520 + 23 * i, 411 + 31 * i) for i in range(8)])
    perms = list(itertools.permutations(range(4)))
    out = []
    for k, ss in enumerate(sizes):
        images, jobs = [], []
        for i, (h, w) in enumerate(ss):
            images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            jobs.append(job(h, w, REUSE_S, flip=i % 2 == 0, order=perms[(7 * k + 5 * i) % 24],
                            factor=(fs[i % len(fs)], fs[(i + k) % len(fs)], fs[(i + 3) % len(fs)], hue_factor(HUE_SHIFTS[(i + k) % 11]))))
        out.append((images, jobs))
    return tuple(out)


def table_bytes(jobs: List[Dict], job_bytes: int = 112) -> int:
    """The size of the block `InputPipeline._run` packs for a batch: the job structs and the int32 bounds and taps of every distinct
    (in, out) pair."""
    pairs = set()
    for jb in jobs:
        pairs.add((jb["crop"][3], jb["resize"][1]))
        pairs.add((jb["crop"][2], jb["resize"][0]))
    n = sum(o * (2 + R.resize_coeffs(i, 0, i, o)[1].shape[1]) for i, o in pairs)
    return job_bytes * len(jobs) + 4 * n


# ------------------------------------------------------------------------------------------------ the restatement, one step mutated
MUTATIONS = ("fused_blend", "floor_mean", "no_round_term", "no_clip8", "finish_scale")


def _resample_axis(img, bounds, kk, axis, round_term, clip):
    a = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.zeros((len(bounds),) + a.shape[1:], np.int64)
    for o, (xmin, n) in enumerate(bounds):
        acc = np.full(a.shape[1:], (1 << (R.PRECISION_BITS - 1)) if round_term else 0, np.int64)
        for k in range(int(n)):
            acc += a[xmin + k] * int(kk[o, k])
        out[o] = acc >> R.PRECISION_BITS
    out = np.clip(out, 0, 255) if clip else out & 255          # no clip: the store keeps the low byte
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def unclipped_range(img: np.ndarray, out_h: int, out_w: int) -> Tuple[int, int]:
    """(min, max) over both passes of the bicubic accumulator >> 22 before clip8 (the vertical pass reads the clipped horizontal one,
    as the kernels do)."""
    lo, hi, x = 0, 255, img
    passes = ((1, (img.shape[1], out_w)), (0, (img.shape[0], out_h)))
    for axis, (i, o) in (passes[::-1] if R.vertical_first(*img.shape[:2], out_h) else passes):
        bounds, kk = R.resize_coeffs(i, 0, i, o)
        a = np.moveaxis(x, axis, 0).astype(np.int64)
        for k, (xmin, n) in enumerate(bounds):
            acc = (1 << (R.PRECISION_BITS - 1)) + np.tensordot(kk[k, :n].astype(np.int64), a[xmin:xmin + n], 1)
            lo, hi = min(lo, int((acc >> R.PRECISION_BITS).min())), max(hi, int((acc >> R.PRECISION_BITS).max()))
        x = _resample_axis(x, bounds, kk, axis, True, True)
    return lo, hi


def _blend(in1, in2, alpha, fused):
    a = f32(alpha)
    d = in2.astype(np.int32) - in1.astype(np.int32)
    t = (in1.astype(f64) + f64(a) * d.astype(f64)).astype(f32) if fused else in1.astype(f32) + a * d.astype(f32)
    if 0.0 <= a <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def jitter_mut(x: np.ndarray, op: int, value: float, mutation: Optional[str] = None) -> np.ndarray:
    if op == 3:
        return R.adjust_hue(x, value)
    if op == 0:
        in1 = np.zeros_like(x)
    elif op == 1:
        g = R.to_gray(x)
        in1 = np.full_like(x, int(g.sum()) // g.size if mutation == "floor_mean" else R.gray_mean(x))
    else:
        in1 = np.repeat(R.to_gray(x)[..., None], 3, axis=2)
    return _blend(in1, x, value, mutation == "fused_blend")


def apply_mut(img: np.ndarray, jb: Dict, mutation: Optional[str] = None) -> np.ndarray:
    """`R.apply` with one step of its arithmetic replaced by the mistake a kernel could make; mutation=None is R.apply itself."""
    assert mutation is None or mutation in MUTATIONS + ("horizontal_first", "vertical_first")
    cy, cx, ch, cw = jb["crop"]
    x = img[cy:cy + ch, cx:cx + cw]
    rt, clip = mutation != "no_round_term", mutation != "no_clip8"
    vfirst = R.vertical_first(ch, cw, jb["resize"][0]) and mutation != "horizontal_first"
    if mutation == "vertical_first":        # half of Pillow's condition: every tall source, lowered or not
        vfirst = ch > 100 * cw
    for axis in ((0, 1) if vfirst else (1, 0)):
        i, o = ((ch, jb["resize"][0]), (cw, jb["resize"][1]))[axis]
        if o != i:
            x = _resample_axis(x, *R.resize_coeffs(i, 0, i, o), axis, rt, clip)
    oy, ox, oh, ow = jb["window"]
    x = x[oy:oy + oh, ox:ox + ow]
    if jb["flip"]:
        x = x[:, ::-1]
    for op in jb["order"]:
        if op >= 0:
            x = jitter_mut(np.ascontiguousarray(x), op, jb["factor"][op], mutation)
    if mutation == "finish_scale":
        return np.ascontiguousarray(x).transpose(2, 0, 1).astype(f32) * f32(2.0 / 255.0) - f32(1)
    return R.to_tensor_normalize(np.ascontiguousarray(x))
