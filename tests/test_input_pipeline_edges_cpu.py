"""The input pipeline's edge cases (tests/input_pipeline_cases.py), as far as they can be checked without a GPU:

* every case's restatement (`oracle.input_ref.apply`) equals Pillow (`apply_pil`), which extends the restatement's pin to the factors
  and shapes of these cases;
* every builder's property holds, so that the GPU tests in tests/test_input_pipeline_edges_gpu.py are as sharp as they claim;
* each of five mistakes a kernel could make, made in the numpy restatement (`cases.apply_mut`), changes bytes of a named case;
* Pillow's pass order: vertical first for a source more than 100 times taller than wide that is being lowered, else horizontal first;
* the library's host side: the tap generator's edges and every argument check of the launch sequence."""
import ctypes

import numpy as np
import pytest

from gan_variant_research_amd import _lib
from oracle import input_ref as R
from tests import input_pipeline_cases as C

f32 = np.float32


def _pin(images, jobs):
    for i, (im, jb) in enumerate(zip(images, jobs)):
        want = R.apply_pil(im, jb)
        assert np.array_equal(R.apply(im, jb), want), (i, jb)
        assert np.array_equal(C.apply_mut(im, jb), want), (i, jb)


def _diff(images, jobs, mutation):
    """Bytes (output elements) that differ between Pillow and the restatement with `mutation`, per job."""
    return [int((C.apply_mut(im, jb, mutation) != R.apply_pil(im, jb)).sum()) for im, jb in zip(images, jobs)]


# ------------------------------------------------------------------------------------------------ the blend's sensitive pairs
def test_sensitive_pair_counts():
    """What the existing factors cannot see and the new ones can: byte pairs whose blend a fused multiply-add changes."""
    count = lambda a: int(C.sensitive_pairs(f32(a)).sum())
    for a in (C.F095, C.F105, C.DOWN1, 0.5, 0.0, 2.0, 1 + 2.0 ** -10, 1 - 2.0 ** -10):
        assert count(a) == 0, a
    assert count(C.UP1) == 2697
    assert count(1.0222220420837402) == 127 and count(0.9596773386001587) == 122
    found = C.searched_factors()
    assert len(set(found)) == 2
    for a in found:
        assert f32(0.95) <= f32(a) <= f32(1.05) and float(f32(a)) == a and count(a) >= C.MIN_PAIRS, a
    # in1 = 0 leaves a single rounding: brightness, and a contrast mean of 0, cannot tell the two forms apart
    assert not C.sensitive_pairs(np.array((C.UP1,) + found, f32))[:, 0].any()
    print("sensitive pairs:", {a: count(a) for a in (C.UP1,) + found})


def test_hue_factors_give_their_shifts():
    assert [R.hue_shift(C.hue_factor(s)) for s in C.HUE_SHIFTS] == list(C.HUE_SHIFTS)
    drawn = {R.hue_shift(float(f)) for f in np.linspace(-0.02, 0.02, 4001)}         # ColorJitter(hue=0.02)'s range
    assert drawn == set(C.HUE_SHIFTS[:11])


def test_to_bytes_inverts_the_normalisation():
    v = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    assert np.array_equal(C.to_bytes(R.to_tensor_normalize(v)), v.transpose(2, 0, 1))
    with pytest.raises(AssertionError):
        C.to_bytes(np.array([0.3], f32))


def test_finish_scale_mutation_is_visible():
    c = np.arange(256, dtype=np.uint8).reshape(1, 256, 1)
    bad = c.transpose(2, 0, 1).astype(f32) * f32(2.0 / 255.0) - f32(1)
    n = int((bad != R.to_tensor_normalize(c)).sum())
    print("finish: c*(2/255)-1 differs from (c/255-0.5)/0.5 on", n, "of 256 bytes")
    assert n >= 1


# ------------------------------------------------------------------------------------------------ 1. the colour cube
def test_cube_holds_every_colour_and_reaches_the_jitter_unchanged():
    c = C.cube()
    assert c.shape == (256, 256, 256, 3) and all(np.all(c[r, ..., 0] == r) for r in (0, 77, 255))
    flat = c.reshape(-1, 3).astype(np.int64)
    assert np.array_equal(flat[:, 0] << 16 | flat[:, 1] << 8 | flat[:, 2], np.arange(1 << 24))
    assert C.identity_taps_are_exact()
    jb = C.cube_jobs(2, C.UP1, 1)[0]
    assert jb["crop"] == (0, 0, 256, 256) and jb["resize"] == (256, 256) and jb["window"] == (0, 0, 256, 256) and jb["order"] == (2, -1, -1, -1)
    im = c[200]
    assert np.array_equal(R.apply_pil(im, C.job(256, 256, 256)), R.to_tensor_normalize(im))


@pytest.fixture(scope="module")
def hsv_tables():
    """Pillow's HSV planes of the cube, and the restatement's RGB of every HSV triple (indexed h << 16 | s << 8 | v)."""
    v = np.arange(256, dtype=np.uint8)
    h, s, vv = np.meshgrid(v, v, v, indexing="ij")
    return C.cube_pil_hsv(), R.hsv_to_rgb(np.stack([h, s, vv], -1).reshape(-1, 3))


def test_cube_hue_restatement_equals_pillow(hsv_tables):
    """R.adjust_hue on the whole cube for every shift of the GPU test; hsv_to_rgb is evaluated once over all 2^24 HSV triples and
    looked up, which is the same function."""
    hsv, rgb_of = hsv_tables
    mine = R.rgb_to_hsv(C.cube().reshape(-1, 3)).astype(np.int64)
    assert np.array_equal(mine, np.stack([np.asarray(p).reshape(-1) for p in hsv], -1))
    for shift in C.HUE_SHIFTS:
        key = ((mine[:, 0] + shift) & 255) << 16 | mine[:, 1] << 8 | mine[:, 2]
        assert np.array_equal(rgb_of[key], C.cube_pil_hue(hsv, shift).reshape(-1, 3)), shift


@pytest.mark.parametrize("name", C.SATURATION_IDS)
def test_cube_saturation_restatement_equals_pillow(name):
    a = C.saturation_factor(name)
    flat = C.cube().reshape(4096, 4096, 3)
    want = C.cube_pil_enhance(2, a).reshape(flat.shape)
    assert np.array_equal(R.adjust_saturation(flat, a), want)
    if name in ("up1", "searched0", "searched1"):        # the factors that are there to catch a fused blend: they do, on this image
        n = int((C.jitter_mut(flat, 2, a, "fused_blend") != want).sum())
        print(f"fused blend, cube saturation {name} = {a!r}: {n} bytes differ")
        assert n > 0


@pytest.mark.parametrize("name", list(C.BRIGHTNESS))
def test_cube_brightness_restatement_equals_pillow(name):
    a = C.BRIGHTNESS[name]
    flat = C.cube().reshape(4096, 4096, 3)[:1024]           # images 0..63: every byte in g and b, which is all brightness looks at
    assert np.array_equal(R.adjust_brightness(flat, a), C.cube_pil_enhance(0, a, C.cube()[:64]).reshape(flat.shape))


# ------------------------------------------------------------------------------------------------ 2. the contrast mean
def test_mean_images_sit_on_the_tie_and_one_below():
    ims = C.mean_images()
    assert [(m["d"], m["tie"]) for m in ims] == [(d, t) for d in C.MEAN_TARGETS for t in (True, False)]
    for m in ims:
        img, d = m["image"], m["d"]
        assert img.shape == (16, 16, 3) and C.luma_sum(img) == m["sum"] == 256 * d + (128 if m["tie"] else 127)
        assert R.gray_mean(img) == m["mean"] == (d + 1 if m["tie"] else d)
        assert (2 * m["sum"] + 256) // 512 == m["mean"]
        assert m["all_bytes"] == (d == 127)
        a = m["searched"]
        assert f32(0.95) <= f32(a) <= f32(1.05) and float(f32(a)) == a
        if m["mean"] > 0:
            assert C.sensitive_pairs(f32(a))[m["mean"], np.unique(img)].any(), (d, m["tie"])
    assert len({tuple(m["image"].reshape(-1)) for m in ims}) == len(ims)


def test_mean_batch_restatement_equals_pillow_and_is_sharp():
    images, jobs, meta = C.mean_batch()
    assert len(jobs) == 42 and all(jb["order"] == (1, -1, -1, -1) for jb in jobs)
    _pin(images, jobs)
    fused, floor = _diff(images, jobs, "fused_blend"), _diff(images, jobs, "floor_mean")
    for n_fused, n_floor, m in zip(fused, floor, meta):
        if m["factor"] == "searched" and m["mean"] > 0:        # searched for this image's mean and bytes
            assert n_fused > 0, m
        if m["factor"] == "0.95":                   # a floored mean is d instead of d + 1 on every tie image, and right below it
            assert (n_floor > 0) == m["tie"], m
        assert m["tie"] or n_floor == 0, m
    assert sum(n for n, m in zip(fused, meta) if m["factor"] == "up1") > 0 and not any(n for n, m in zip(fused, meta) if m["factor"] == "0.95")
    print(f"contrast-mean batch: fused blend {sum(fused)} bytes in {sum(n > 0 for n in fused)} jobs; "
          f"floor(t/n) {sum(floor)} bytes in {sum(n > 0 for n in floor)} jobs")
    assert all(any(n > 0 for n, m in zip(floor, meta) if m["d"] == d and m["tie"]) for d in C.MEAN_TARGETS)


# ------------------------------------------------------------------------------------------------ 3. geometry
@pytest.mark.parametrize("S", list(C.GEOMETRY))
def test_geometry_restatement_equals_pillow_and_is_sharp(S):
    images, jobs, meta = C.geometry_batch(S)
    assert len(jobs) == len(C.GEOMETRY[S]) * len(C.CONTENTS) * 2 <= C.GEOMETRY_MAX_BATCH
    lib = _lib.load()
    for jb, (h, w, _, _) in zip(jobs, meta):
        for filter in (C.BICUBIC, C.BILINEAR):
            assert C.tap_count(h, S, filter) == lib.gan_resize_ksize_filter(h, S, filter)
            assert C.supported(jb, filter) == ((h, w, filter) != (300, 2, C.BICUBIC))       # 1201 taps: the one job the library refuses
    _pin(images, jobs)
    for mutation in ("no_round_term", "no_clip8", "finish_scale"):
        n = _diff(images, jobs, mutation)
        print(f"geometry S={S}: {mutation} {sum(n)} bytes in {sum(v > 0 for v in n)} of {len(n)} jobs")
        assert sum(n) > 0 or (mutation == "no_clip8" and S == 1)        # a single output pixel of these sources never overshoots
    n = _diff(images, jobs, "horizontal_first")         # the pass order Pillow does not use for a tall source
    tall = [R.vertical_first(h, w, S) for h, w, _, _ in meta]
    print(f"geometry S={S}: horizontal_first {sum(n)} bytes in {sum(v > 0 for v in n)} of {sum(tall)} tall jobs")
    assert all(v == 0 for v, t in zip(n, tall) if not t) and (sum(n) > 0) == (S in (1, 5))


def test_checkerboards_leave_the_byte_range():
    """clip8 bites on both sides: the one-pixel board where the image is enlarged, the two-output-pixel board where it is reduced."""
    both = lambda lo, hi: lo < 0 and hi > 255
    up = [(2, 3, 5), (16, 16, 17)]
    down = [(9, 300, 5), (300, 9, 5), (18, 18, 17), (33, 35, 17), (2000, 17, 17)]
    for h, w, S in up:
        assert both(*C.unclipped_range(C.content("checker", h, w, None, S), S, S)), (h, w, S)
    for h, w, S in down:
        assert both(*C.unclipped_range(C.content("blocks", h, w, None, S), S, S)), (h, w, S)
        assert C.unclipped_range(C.content("checker", h, w, None, S), S, S) == (0, 255)


def test_pillow_pass_order_for_tall_sources():
    """Image.resize equals its own vertical-then-horizontal pair of single-axis resizes when the source is more than 100 times taller
    than wide AND the target is lower than the source (Image.py: `size[1] > size[0] * 100 and new_height < size[1]`), and the
    horizontal-then-vertical pair otherwise, for both filters.  Each half of the condition is crossed: the aspect at h = 100 w and
    100 w + 1, the height at oh = h - 1, h and above.  The restatement and the kernels follow R.vertical_first."""
    from PIL import Image
    rng = np.random.default_rng(8)
    sizes = ((200, 2, 1, 1), (201, 2, 1, 1), (300, 3, 5, 4), (301, 3, 5, 4), (700, 7, 2, 9), (701, 7, 2, 9), (2, 300, 1, 1), (7, 701, 9, 2),
             (201, 2, 200, 1), (201, 2, 200, 5), (201, 2, 202, 1), (201, 2, 256, 17), (250, 2, 286, 3), (301, 3, 400, 5), (301, 3, 300, 2), (301, 3, 302, 2))
    for flt in (Image.BICUBIC, Image.BILINEAR):
        for (h, w, oh, ow) in sizes:
            bad = {"h": 0, "v": 0}
            for _ in range(8):
                img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                want = np.asarray(Image.fromarray(img).resize((ow, oh), flt))
                hv = Image.fromarray(img).resize((ow, h), flt).resize((ow, oh), flt)
                vh = Image.fromarray(img).resize((w, oh), flt).resize((ow, oh), flt)
                bad["h"] += int((np.asarray(hv) != want).sum())
                bad["v"] += int((np.asarray(vh) != want).sum())
                if flt == Image.BICUBIC:
                    assert np.array_equal(R.resize_bicubic(img, oh, ow), want), (h, w, oh, ow)
            first = "v" if R.vertical_first(h, w, oh) else "h"
            assert bad[first] == 0 < bad["h" if first == "v" else "v"], (flt, h, w, oh, ow, bad)
    # oh == h has one pass only, so no order to tell apart: the restatement must still equal Pillow
    for (h, w, oh, ow) in ((201, 2, 201, 1), (201, 2, 201, 16)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(R.resize_bicubic(img, oh, ow), np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC)))
    assert R.vertical_first(201, 2, 200) and not R.vertical_first(200, 2, 1) and not R.vertical_first(201, 2, 201) and not R.vertical_first(201, 2, 256)


# ------------------------------------------------------------------------------------------------ 4..6
def test_crop_batch_restatement_equals_pillow():
    images, jobs, names = C.crop_batch()
    _pin(images, jobs)
    # tall sources: vertical first where Pillow goes horizontal first (height not lowered) is noticed, and so is the reverse
    wrong_v = dict(zip(names, _diff(images, jobs, "vertical_first")))
    wrong_h = dict(zip(names, _diff(images, jobs, "horizontal_first")))
    print("crop batch: vertical_first", {n: v for n, v in wrong_v.items() if v}, "horizontal_first", {n: v for n, v in wrong_h.items() if v})
    raised = ("tall.201x2.to.256x17", "tall.201x2.to.286x16", "tall.201x2.to.202x18")
    assert all(wrong_v[n] > 0 for n in raised) and set(n for n, v in wrong_v.items() if v) == set(raised)
    assert wrong_h["crop.tall.301x3"] > 0 and wrong_h["tall.201x2.to.200x16"] > 0
    assert set(n for n, v in wrong_h.items() if v) <= {"crop.tall.301x3", "tall.201x2.to.200x16"}
    H, W = images[0].shape[:2]
    crops = {n: jb["crop"] for n, jb in zip(names, jobs)}
    assert crops["crop.first"][:2] == (0, 0) and crops["crop.last"][0] + crops["crop.last"][2] == H and crops["crop.last"][1] + crops["crop.last"][3] == W
    assert crops["crop.pixel.last"] == (H - 1, W - 1, 1, 1)
    wins = sorted(jb["window"][:2] for n, jb in zip(names, jobs) if n.startswith("window"))
    assert wins == [(0, 0), (0, 15), (3, 0), (3, 15)] and all(jb["resize"] == (19, 31) for n, jb in zip(names, jobs) if n.startswith("window"))
    for im in (images[0], images[-1]):
        big, (y0, x0) = C.embed(im)
        h, w = im.shape[:2]
        assert big.shape == (h + 7, w + 5, 3) and np.array_equal(big[y0:y0 + h, x0:x0 + w], im)
        assert np.array_equal(big[y0 - 1, x0:x0 + w], 255 - im[0]) and np.array_equal(big[y0 + h, x0:x0 + w], 255 - im[-1])
        assert np.array_equal(big[y0:y0 + h, x0 - 1], 255 - im[:, 0]) and np.array_equal(big[y0:y0 + h, x0 + w], 255 - im[:, -1])


def test_mixed_batch_restatement_equals_pillow_and_is_sharp():
    images, jobs = C.mixed_batch()
    assert len(jobs) == C.MIXED_B and [jb["flip"] for jb in jobs] == [i % 2 == 1 for i in range(C.MIXED_B)]
    assert [i for i, jb in enumerate(jobs) if jb["order"] == C.NO_JITTER] == list(range(3, 32, 4))
    _pin(images, jobs)
    for mutation in C.MUTATIONS:
        n = _diff(images, jobs, mutation)
        print(f"mixed batch: {mutation} {sum(n)} bytes in {sum(v > 0 for v in n)} of {len(n)} jobs")
        assert sum(n) > 0, mutation


def test_reuse_batches_force_each_growth_once():
    (_, j1), (_, j2), (_, j3) = C.reuse_batches()
    assert ctypes.sizeof(_lib.GanInputJob) == 112
    rows = [max(jb["crop"][2] for jb in jobs) for jobs in (j1, j2, j3)]
    assert rows[0] <= C.REUSE_MAX_ROWS < rows[1] and rows[2] <= -(-rows[1] // 256) * 256        # the second grows the rows, the third does not
    block = max(2 * C.table_bytes(j1), C.FIRST_BLOCK_BYTES)
    assert C.table_bytes(j2) <= block < C.table_bytes(j3)                                       # the third outgrows the table block
    assert all(len(jobs) <= C.REUSE_MAX_BATCH for jobs in (j1, j2, j3))
    for images, jobs in C.reuse_batches():
        _pin(images, jobs)


# ------------------------------------------------------------------------------------------------ the library's host side
def test_tap_generator_edges():
    lib = _lib.load()
    assert lib.gan_resize_ksize(4353, 17) == 1027
    b, k = np.zeros((17, 2), np.int32), np.zeros((17, 1027), np.int32)
    assert lib.gan_resize_coeffs(4353, 17, b.ctypes.data, k.ctypes.data, 1027) != 0
    assert b"downscale factor too large" in lib.gan_last_error()
    assert not b.any() and not k.any()
    for (i, o) in ((1, 8), (8, 1), (1, 1)):
        bounds, kk = R.resize_coeffs(i, 0, i, o)
        n = lib.gan_resize_ksize(i, o)
        assert n == kk.shape[1]
        b, k = np.zeros((o, 2), np.int32), np.zeros((o, n), np.int32)
        assert lib.gan_resize_coeffs(i, o, b.ctypes.data, k.ctypes.data, n) == 0
        assert np.array_equal(b, bounds) and np.array_equal(k, kk), (i, o)


def _good_job():
    """A job that would pass every check (and launch): each test below breaks exactly one field of it."""
    lib = _lib.load()
    j = _lib.GanInputJob()
    j.src, j.src_stride = 0x1000, 3 * 20
    j.crop_y, j.crop_x, j.crop_h, j.crop_w = 2, 4, 12, 16
    j.res_h, j.res_w, j.win_y, j.win_x = 18, 17, 2, 1
    for s in range(4):
        j.order[s], j.factor[s] = -1, 1.0
    j.hksize = lib.gan_resize_ksize_filter(16, 17, C.BICUBIC)
    j.vksize = lib.gan_resize_ksize_filter(12, 18, C.BICUBIC)
    return j


ARGUMENT_CHECKS = {
    "crop_right_of_row": (dict(crop_x=5), {}, b"outside a row of 60 bytes"),
    "crop_negative": (dict(crop_y=-1), {}, b"outside a row"),
    "crop_empty": (dict(crop_h=0), {}, b"outside a row"),
    "window_below": (dict(win_y=3), {}, b"outside the 18x17 resized image"),
    "window_right": (dict(win_x=2), {}, b"outside the 18x17 resized image"),
    "window_negative": (dict(win_x=-1), {}, b"outside the 18x17 resized image"),
    "taps_h": (dict(hksize=7), {}, b"tap counts do not match"),
    "taps_v": (dict(vksize=3), {}, b"tap counts do not match"),
    "taps_of_other_filter": ({}, dict(filter=C.BILINEAR), b"tap counts do not match"),
    "rows": ({}, dict(tmp_rows=11), b"12 source rows > tmp_rows 11"),
    "op_high": (dict(order=(0, 1, 2, 4)), {}, b"jitter op 4"),
    "op_low": (dict(order=(-2, -1, -1, -1)), {}, b"jitter op -2"),
    "filter": ({}, dict(filter=1), b"unknown filter 1"),
    "empty_batch": ({}, dict(B=0), b"null pointer or empty batch"),
    "null_output": ({}, dict(out=0), b"null pointer or empty batch"),
}


@pytest.mark.parametrize("name", list(ARGUMENT_CHECKS))
def test_launch_refuses_bad_arguments(name):
    """Every GAN_CHECK of input_pipeline_launch: nonzero, its own message, and nothing launched -- the pointers are dummies and this
    machine has no GPU, so a launch could only fail with another message.  Only failing jobs are passed: a good one would launch."""
    lib = _lib.load()
    fields, args, message = ARGUMENT_CHECKS[name]
    jobs = (_lib.GanInputJob * 1)(_good_job())
    for k, v in fields.items():
        if k == "order":
            for s in range(4):
                jobs[0].order[s] = v[s]
        else:
            setattr(jobs[0], k, v)
    a = dict(B=1, S=16, filter=C.BICUBIC, tmp_rows=12, out=0x6000)
    a.update(args)
    host = ctypes.addressof(jobs)
    for entry in ("gan_input_pipeline_filter", "gan_input_pipeline_u8"):
        rc = getattr(lib, entry)(0x2000, host, a["B"], 0x3000, a["S"], a["filter"], 0x4000, a["tmp_rows"], 0x5000, 0x7000, a["out"], None)
        assert rc != 0 and message in lib.gan_last_error(), (entry, rc, lib.gan_last_error())
    if "filter" not in args:
        rc = lib.gan_input_pipeline(0x2000, host, a["B"], 0x3000, a["S"], 0x4000, a["tmp_rows"], 0x5000, 0x7000, a["out"], None)
        assert rc != 0 and message in lib.gan_last_error(), (rc, lib.gan_last_error())


def test_the_good_job_differs_from_each_bad_one_only_in_the_broken_field():
    """The base job of the argument checks satisfies every condition, restated here, so each case above fails for its own reason."""
    lib, j, S, rows = _lib.load(), _good_job(), 16, 12
    assert j.src and j.crop_h > 0 and j.crop_w > 0 and j.crop_y >= 0 and j.crop_x >= 0 and j.src_stride == 3 * (j.crop_x + j.crop_w)
    assert j.win_y >= 0 and j.win_x >= 0 and j.win_y + S == j.res_h and j.win_x + S == j.res_w
    assert j.hksize == lib.gan_resize_ksize_filter(j.crop_w, j.res_w, C.BICUBIC) != lib.gan_resize_ksize_filter(j.crop_w, j.res_w, C.BILINEAR)
    assert j.vksize == lib.gan_resize_ksize_filter(j.crop_h, j.res_h, C.BICUBIC) and j.crop_h == rows
    assert all(-1 <= j.order[s] <= 3 for s in range(4))
