"""The device input pipeline (csrc/input_pipeline.hip) against Pillow itself at every colour and at its edge shapes.

Every comparison is np.array_equal over every output element: the pipeline promises Pillow's bytes, so there is no tolerance and no
exempted pixel.  The cases and what each was built to catch are in tests/input_pipeline_cases.py; that they have those properties, and
which arithmetic mistake each one notices, is checked on the CPU in tests/test_input_pipeline_edges_cpu.py."""
import numpy as np
import pytest
import torch

from gan_variant_research_amd import _lib, dataio
from oracle import input_ref as R
from tests import input_pipeline_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _upload(images):
    return [torch.from_numpy(im).to(DEV) for im in images]


def _assert_equal(got: np.ndarray, want: np.ndarray, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(1))
        raise AssertionError(f"{what}: {int((got != want).sum())} of {got.size} elements differ, in images {bad[:16].tolist()} ({len(bad)} in all)")


def _expected(images, jobs, filter=C.BICUBIC):
    return np.stack([C.pil_apply(im, jb, filter) for im, jb in zip(images, jobs)])


# ------------------------------------------------------------------------------------------------ 1. the colour cube
@pytest.fixture(scope="module")
def cube_run():
    """run(op, value) -> uint8 [256][3][256][256]: the 256 images of the cube through `run_u8`, 64 per launch sequence."""
    images = list(torch.from_numpy(C.cube()).to(DEV))
    pipe = dataio.InputPipeline(C.CUBE_S, DEV, max_batch=64, max_rows=C.CUBE_S)
    out = torch.empty(256, 3, C.CUBE_S, C.CUBE_S, dtype=torch.uint8, device=DEV)

    def run(op, value):
        jobs = C.cube_jobs(op, value, 64)
        for k in range(0, 256, 64):
            pipe.run_u8(images[k:k + 64], jobs, out=out[k:k + 64])
        return out.cpu().numpy()

    run.pipe, run.images = pipe, images
    return run


@pytest.fixture(scope="module")
def cube_hsv():
    return C.cube_pil_hsv()


@pytest.mark.parametrize("shift", C.HUE_SHIFTS)
def test_cube_hue(cube_run, cube_hsv, shift):
    """hue_rotate on all 2^24 colours: float32 variables, double constants, the device's trunc, floor and round."""
    _assert_equal(cube_run(3, C.hue_factor(shift)), C.nchw(C.cube_pil_hue(cube_hsv, shift)), f"hue shift {shift}")


@pytest.mark.parametrize("name", C.SATURATION_IDS)
def test_cube_saturation(cube_run, name):
    """blend1 with in1 = the pixel's own luma, on every colour; up1 and the searched factors differ under a fused multiply-add."""
    a = C.saturation_factor(name)
    _assert_equal(cube_run(2, a), C.nchw(C.cube_pil_enhance(2, a)), f"saturation {a!r}")


@pytest.mark.parametrize("name", list(C.BRIGHTNESS))
def test_cube_brightness(cube_run, name):
    a = C.BRIGHTNESS[name]
    _assert_equal(cube_run(0, a), C.nchw(C.cube_pil_enhance(0, a)), f"brightness {a!r}")


def test_cube_finish_fp32(cube_run):
    """One fp32 batch of 64 cube images (brightness 1.0 keeps the bytes): input_finish_kernel on all 256 byte values."""
    jobs = C.cube_jobs(0, 1.0, 64)
    out = cube_run.pipe.run(cube_run.images[:64], jobs)
    assert out.dtype == torch.float32
    _assert_equal(out.cpu().numpy(), _expected(C.cube()[:64], jobs), "fp32 finish")


# ------------------------------------------------------------------------------------------------ 2. the contrast mean
def test_contrast_mean_at_the_tie_and_below():
    """input_gray_mean_kernel's (2t + n) / (2n) with the luma sum on a tie (-> d + 1) and one below (-> d), all in one batch."""
    images, jobs, meta = C.mean_batch()
    pipe = dataio.InputPipeline(C.MEAN_S, DEV, max_batch=64, max_rows=C.MEAN_S)
    out = pipe.run(_upload(images), jobs)
    _assert_equal(out.cpu().numpy(), _expected(images, jobs), "contrast at a mean tie")
    assert pipe._mean[:len(jobs)].cpu().tolist() == [m["mean"] for m in meta]


# ------------------------------------------------------------------------------------------------ 3. geometry
@pytest.mark.parametrize("S", list(C.GEOMETRY))
@pytest.mark.parametrize("filter", [C.BICUBIC, C.BILINEAR], ids=["bicubic", "bilinear"])
def test_geometry(filter, S):
    """Every source size x content x flip into S x S: one-pixel sources and outputs, odd S under flip, clip8 on overshoot, and
    2000 rows -> 17 (473 bicubic taps; the buffer between the passes grows), and sources more than 100 times taller than wide, whose
    vertical pass Pillow makes first."""
    images, jobs, meta = C.geometry_batch(S)
    pipe = dataio.InputPipeline(S, DEV, max_batch=C.GEOMETRY_MAX_BATCH, filter=filter)
    rows = pipe.max_rows
    refused = [i for i, jb in enumerate(jobs) if not C.supported(jb, filter)]
    assert [meta[i][:2] for i in refused] == ([(300, 2)] * (2 * len(C.CONTENTS)) if (filter, S) == (C.BICUBIC, 1) else [])
    if refused:         # more taps than the tap generator holds: an error, and the whole batch is not launched
        with pytest.raises(_lib.GanError, match="downscale factor too large"):
            pipe.run(_upload(images), jobs)
        images, jobs = ([v for i, v in enumerate(seq) if i not in refused] for seq in (images, jobs))
    dev = _upload(images)
    want = _expected(images, jobs, filter)
    _assert_equal(pipe.run(dev, jobs).cpu().numpy(), want, f"geometry S={S} fp32")
    _assert_equal(pipe.run_u8(dev, jobs).cpu().numpy(), C.to_bytes(want), f"geometry S={S} uint8")
    assert (pipe.max_rows > rows) == (S == 17)


# ------------------------------------------------------------------------------------------------ 4. crop, stride and window
@pytest.mark.parametrize("filter", [C.BICUBIC, C.BILINEAR], ids=["bicubic", "bilinear"])
def test_crop_stride_and_window(filter):
    """Crops in the corners and of one pixel, windows in the corners of a non-square resize; every source is a strided view of a
    larger tensor whose surroundings hold other bytes, and the reference sees only the view's pixels."""
    images, jobs, names = C.crop_batch()
    if filter == C.BILINEAR:        # the inference filter never meets jitter: the same geometry without it
        jobs = [dict(jb, order=C.NO_JITTER) for jb in jobs]
    views = []
    for im in images:
        big, (y0, x0) = C.embed(im)
        v = torch.from_numpy(big).to(DEV)[y0:y0 + im.shape[0], x0:x0 + im.shape[1]]
        assert not v.is_contiguous() and v.stride(0) == big.shape[1] * 3
        views.append(v)
    pipe = dataio.InputPipeline(C.CROP_S, DEV, max_batch=16, max_rows=320, filter=filter)
    _assert_equal(pipe.run(views, jobs).cpu().numpy(), _expected(images, jobs, filter), f"crop/window {names}")


# ------------------------------------------------------------------------------------------------ 5. the mixed batch
@pytest.mark.parametrize("kind", ["fp32", "uint8"])
def test_mixed_batch_into_a_slice(kind):
    """All 24 jitter orders and jobs without jitter in one batch, flips alternating, written into the middle of a larger buffer."""
    images, jobs = C.mixed_batch()
    B, S = C.MIXED_B, C.MIXED_S
    pipe = dataio.InputPipeline(S, DEV, max_batch=B, max_rows=64)
    want = _expected(images, jobs)
    if kind == "fp32":
        buf = torch.full((B + 2, 3, S, S), float("nan"), dtype=torch.float32, device=DEV)
        out = pipe.run(_upload(images), jobs, out=buf[1:B + 1])
        guards_ok = bool(torch.isnan(buf[0]).all() and torch.isnan(buf[B + 1]).all())
    else:
        buf = torch.full((B + 2, 3, S, S), 0xA5, dtype=torch.uint8, device=DEV)
        out = pipe.run_u8(_upload(images), jobs, out=buf[1:B + 1])
        guards_ok = bool((buf[0] == 0xA5).all() and (buf[B + 1] == 0xA5).all())
        want = C.to_bytes(want)
    assert out.data_ptr() == buf[1].data_ptr()
    _assert_equal(out.cpu().numpy(), want, f"mixed batch {kind}")
    assert guards_ok, "the pipeline wrote outside its output"


# ------------------------------------------------------------------------------------------------ 6. reuse
def test_three_batches_queued_on_one_pipeline():
    """No synchronise between the batches: the second replaces the buffer between the passes, the third the table block, while the
    earlier launches may still be queued; each batch must still come out as Pillow's."""
    batches = C.reuse_batches()
    dev = [_upload(images) for images, _ in batches]
    pipe = dataio.InputPipeline(C.REUSE_S, DEV, max_batch=C.REUSE_MAX_BATCH, max_rows=C.REUSE_MAX_ROWS)
    outs, rows, blocks = [], [], []
    torch.cuda.synchronize()
    for d, (_, jobs) in zip(dev, batches):
        outs.append(pipe.run(d, jobs))
        rows.append(pipe.max_rows)
        blocks.append(pipe._block_bytes)
    torch.cuda.synchronize()
    assert rows[0] == C.REUSE_MAX_ROWS < rows[1] == rows[2] and blocks[0] == blocks[1] == C.FIRST_BLOCK_BYTES < blocks[2]
    for k, (out, (images, jobs)) in enumerate(zip(outs, batches)):
        _assert_equal(out.cpu().numpy(), _expected(images, jobs), f"queued batch {k}")


# ------------------------------------------------------------------------------------------------ 7. the plain entry
class _PlainEntry:
    """The library with `gan_input_pipeline_filter` routed to the older `gan_input_pipeline` (no filter argument: BICUBIC), so that
    InputPipeline packs the jobs and tables and the plain entry launches them."""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def gan_input_pipeline_filter(self, jobs_dev, jobs_host, B, tables, S, filter, tmp, rows, img, mean, out, stream):
        assert filter == C.BICUBIC
        self.calls += 1
        return self._lib.gan_input_pipeline(jobs_dev, jobs_host, B, tables, S, tmp, rows, img, mean, out, stream)


def test_plain_entry_equals_the_filter_entry():
    images, jobs = C.mixed_batch()
    dev = _upload(images)
    via_filter = dataio.InputPipeline(C.MIXED_S, DEV, max_batch=C.MIXED_B, max_rows=64).run(dev, jobs)
    pipe = dataio.InputPipeline(C.MIXED_S, DEV, max_batch=C.MIXED_B, max_rows=64)
    pipe.lib = _PlainEntry(pipe.lib)
    plain = pipe.run(dev, jobs)
    assert pipe.lib.calls == 1
    assert np.array_equal(plain.cpu().numpy().view(np.uint8), via_filter.cpu().numpy().view(np.uint8))
    _assert_equal(plain.cpu().numpy(), _expected(images, jobs), "gan_input_pipeline")
