"""Device-side input pipeline: the reference's per-image PIL transforms as one batched HIP launch sequence.

The reference decodes a JPEG on a DataLoader worker and then runs, still on the CPU and per image,

    GAN_Variant1/dataio/transforms.py:30-39   RandomCropResize(S, (0.85, 1.0)) -> RandomHorizontalFlip -> ColorJitter(.05,.05,.05,.02)
                                              -> ToTensor -> Normalize(0.5, 0.5)            (train)
    GAN_Variant1/dataio/transforms.py:42-49   Resize([S, S], BICUBIC) -> ToTensor -> Normalize           (eval)
    Basic_GAN/src/data.py:8-26                Resize(load, BICUBIC) -> RandomCrop(S) -> flip | Resize(S) -> CenterCrop(S), then the same tail

Here the decoder hands over uint8 HWC images (device tensors), the random parameters are drawn on the host in the reference's order
(`*_job` functions below: numpy's global generator for the crop, torch's for flip and jitter, exactly as the reference mixes them) and
`InputPipeline.run` produces the (B,3,S,S) fp32 batch in [-1,1] on the GPU -- bit-identical to what PIL + torchvision would have
produced for the same draws (tests/test_input_pipeline.py checks against Pillow itself; torchvision is absent from this image, its
glue is restated from its published source).  There is no CPU fallback: without the HIP library `run` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import GanError, GanInputJob

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
BILINEAR, BICUBIC = _lib.RESIZE_BILINEAR, _lib.RESIZE_BICUBIC      # Pillow's ids; the training transforms use BICUBIC, inference BILINEAR


# ------------------------------------------------------------------------------------------------ jobs (host side, per image)
def _job(h, w, crop, resize, window, flip=False, order=(-1, -1, -1, -1), factor=(1.0, 1.0, 1.0, 0.0)) -> Dict:
    return {"size": (int(h), int(w)), "crop": tuple(int(v) for v in crop), "resize": tuple(int(v) for v in resize),
            "window": tuple(int(v) for v in window), "flip": bool(flip), "order": tuple(int(v) for v in order),
            "factor": tuple(float(v) for v in factor)}


def color_jitter_params(brightness=0.05, contrast=0.05, saturation=0.05, hue=0.02) -> Tuple[Tuple[int, ...], Tuple[float, ...]]:
    """torchvision ColorJitter.get_params: a permutation of the four ops, then one uniform draw each for brightness, contrast,
    saturation (in [max(0, 1-x), 1+x]) and hue (in [-hue, hue]), all from torch's global generator."""
    order = tuple(int(i) for i in torch.randperm(4))
    draw = lambda lo, hi: float(torch.empty(1).uniform_(lo, hi))
    b = draw(max(0.0, 1 - brightness), 1 + brightness)
    c = draw(max(0.0, 1 - contrast), 1 + contrast)
    s = draw(max(0.0, 1 - saturation), 1 + saturation)
    h = draw(-hue, hue)
    return order, (b, c, s, h)


def train_job(h: int, w: int, image_size: int = 256, scale=(0.85, 1.0)) -> Dict:
    """get_train_transforms (transforms.py:30-39).  Draw order: np.random.uniform, np.random.randint x2 (RandomCropResize, :19-23),
    torch.rand(1) (flip), torch.randperm(4) + four uniforms (ColorJitter)."""
    sc = np.random.uniform(*scale)
    cs = int(min(w, h) * sc)
    i = np.random.randint(0, h - cs + 1)
    j = np.random.randint(0, w - cs + 1)
    flip = bool(torch.rand(1) < 0.5)
    order, factor = color_jitter_params()
    return _job(h, w, (i, j, cs, cs), (image_size, image_size), (0, 0, image_size, image_size), flip, order, factor)


def eval_job(h: int, w: int, image_size: int = 256) -> Dict:
    """get_eval_transforms (transforms.py:42-49): the whole image resized to S x S."""
    return _job(h, w, (0, 0, h, w), (image_size, image_size), (0, 0, image_size, image_size))


def infer_job(h: int, w: int, image_size: int = 256) -> Dict:
    """generate_folder.py:175-180: the whole image resized to S x S, no flip, no jitter -- eval_job's geometry; the reference resizes
    with BILINEAR there, which is the pipeline's `filter`, not the job's."""
    return eval_job(h, w, image_size)


def _resize_smaller_edge(h: int, w: int, size: int) -> Tuple[int, int]:
    """torchvision Resize(int): the smaller edge becomes `size`, the other int(size * long / short)."""
    if w <= h:
        return int(size * h / w), size
    return size, int(size * w / h)


def basic_job(h: int, w: int, load_size: int = 286, crop_size: int = 256, train: bool = True) -> Dict:
    """Basic_GAN/src/data.py:8-26.  Train: Resize(load_size) -> RandomCrop(crop_size) (torch.randint x2, skipped when nothing to crop)
    -> RandomHorizontalFlip (torch.rand(1)).  Eval: Resize(crop_size) -> CenterCrop(crop_size)."""
    if train:
        rh, rw = _resize_smaller_edge(h, w, load_size)
        if rh == crop_size and rw == crop_size:
            i = j = 0
        else:
            i = int(torch.randint(0, rh - crop_size + 1, size=(1,)))
            j = int(torch.randint(0, rw - crop_size + 1, size=(1,)))
        flip = bool(torch.rand(1) < 0.5)
        return _job(h, w, (0, 0, h, w), (rh, rw), (i, j, crop_size, crop_size), flip)
    rh, rw = _resize_smaller_edge(h, w, crop_size)
    i, j = int(round((rh - crop_size) / 2.0)), int(round((rw - crop_size) / 2.0))
    return _job(h, w, (0, 0, h, w), (rh, rw), (i, j, crop_size, crop_size))


# ------------------------------------------------------------------------------------------------ the device pipeline
def normalize_device(device) -> torch.device:
    """`torch.device("cuda")` names the current device but compares unequal to the `cuda:0` a tensor on it reports: give an index-less
    GPU device the current device's index, once, so that devices can be compared."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class InputPipeline:
    """Batched transform on one GPU.  `run(images, jobs)`: images = uint8 (H, W, 3) device tensors (one per job, any sizes), jobs from
    the `*_job` functions (all with an S x S window) -> (B, 3, S, S) fp32 in [-1, 1].  `filter` is Pillow's resampling filter of every
    resize the pipeline makes (BICUBIC or BILINEAR).  Tap tables are cached per (source, target, filter); jobs and tables travel in one
    pinned block and one asynchronous copy per batch.  `max_rows` sizes the buffer between the two resize passes; a batch with a
    taller image grows it."""

    def __init__(self, image_size: int, device, max_batch: int = 64, max_rows: int = 1024, filter: int = BICUBIC):
        self.S, self.device, self.filter = int(image_size), torch.device(device), int(filter)
        if self.device.type != "cuda":
            raise GanError("the input pipeline runs on the GPU (there is no CPU fallback)")
        self.device = normalize_device(self.device)       # images report an indexed device: `run` compares against this one
        if self.filter not in (BILINEAR, BICUBIC):
            raise GanError(f"input pipeline: unknown filter {filter} (BILINEAR = {BILINEAR}, BICUBIC = {BICUBIC})")
        self.lib = _lib.load()
        self.max_batch, self.max_rows = max_batch, max_rows
        S = self.S
        self._tmp = torch.zeros(max_batch * max_rows * S * 4, dtype=torch.uint8, device=self.device)
        self._img = torch.zeros(max_batch * S * S * 4, dtype=torch.uint8, device=self.device)
        self._mean = torch.zeros(max_batch, dtype=torch.int32, device=self.device)
        self._taps: Dict[Tuple[int, int, int], Tuple[np.ndarray, np.ndarray, int]] = {}
        self._block_bytes = 0
        self._host = self._dev = None

    def taps(self, in_size: int, out_size: int):
        """(bounds [out][2], taps [out][ksize], ksize) of Pillow's resize in_size -> out_size with the pipeline's filter, from the library."""
        key = (in_size, out_size, self.filter)
        t = self._taps.get(key)
        if t is None:
            k = self.lib.gan_resize_ksize_filter(in_size, out_size, self.filter)
            if k < 0:
                raise GanError(self.lib.gan_last_error().decode())
            bounds, kk = np.zeros((out_size, 2), np.int32), np.zeros((out_size, k), np.int32)
            _lib.check(self.lib.gan_resize_coeffs_filter(in_size, out_size, self.filter, bounds.ctypes.data, kk.ctypes.data, k), "gan_resize_coeffs_filter")
            t = self._taps[key] = (bounds, kk, k)
        return t

    def run(self, images: Sequence[torch.Tensor], jobs: Sequence[Dict], out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._run(images, jobs, out, torch.float32, "gan_input_pipeline_filter")

    def run_u8(self, images: Sequence[torch.Tensor], jobs: Sequence[Dict], out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The same transform, left as bytes: (B, 3, S, S) uint8, what PIL's image holds after the jobs' crop, resize, flip and jitter
        (the evaluation loader's `to_tensor(img) * 255` as uint8, EVAL/eval/datasets.py:52-66)."""
        return self._run(images, jobs, out, torch.uint8, "gan_input_pipeline_u8")

    def _run(self, images, jobs, out, dtype, entry) -> torch.Tensor:
        B, S = len(jobs), self.S
        if B == 0 or B != len(images) or B > self.max_batch:
            raise GanError(f"input pipeline: {len(images)} images, {B} jobs, max_batch {self.max_batch}")
        # ---- tables block: [jobs (B x 112 bytes) | int32 taps of every distinct (in, out) pair]
        offs, parts, n = {}, [], 0
        structs = (GanInputJob * B)()
        for b, (im, jb) in enumerate(zip(images, jobs)):
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.device != self.device or im.stride(2) != 1 or im.stride(1) != 3:
                raise GanError(f"input pipeline: image {b} must be a uint8 (H, W, 3) tensor on {self.device} with packed pixels")
            if tuple(im.shape[:2]) != jb["size"]:
                raise GanError(f"input pipeline: image {b} is {tuple(im.shape[:2])}, its job was drawn for {jb['size']}")
            if jb["window"][2:] != (S, S):
                raise GanError(f"input pipeline: job {b} has a {jb['window'][2:]} window, the pipeline produces {S}x{S}")
            cy, cx, ch, cw = jb["crop"]
            if ch > self.max_rows:      # photo folders are not uniform: grow (queued launches keep the old buffer, freed in stream order)
                self.max_rows = -(-ch // 256) * 256
                self._tmp = torch.zeros(self.max_batch * self.max_rows * S * 4, dtype=torch.uint8, device=self.device)
            js = structs[b]
            js.src, js.src_stride = im.data_ptr(), im.stride(0)
            js.crop_y, js.crop_x, js.crop_h, js.crop_w = cy, cx, ch, cw
            js.res_h, js.res_w = jb["resize"]
            js.win_y, js.win_x = jb["window"][:2]
            js.flip = int(jb["flip"])
            for s in range(4):
                js.order[s] = jb["order"][s]
                js.factor[s] = jb["factor"][s]
            js.hue_shift = int(jb["factor"][HUE] * 255) % 256       # torchvision adjust_hue: uint8(hue_factor * 255), wrapping
            for axis, (i_sz, o_sz) in (("h", (cw, js.res_w)), ("v", (ch, js.res_h))):
                key = (i_sz, o_sz)
                if key not in offs:
                    bounds, kk, k = self.taps(i_sz, o_sz)
                    offs[key] = (n, n + bounds.size, k)
                    parts += [bounds.reshape(-1), kk.reshape(-1)]
                    n += bounds.size + kk.size
                bo, ko, k = offs[key]
                if axis == "h":
                    js.hb_off, js.hk_off, js.hksize = bo, ko, k
                else:
                    js.vb_off, js.vk_off, js.vksize = bo, ko, k
        jbytes = C.sizeof(GanInputJob) * B
        total = jbytes + 4 * n
        if total > self._block_bytes:
            self._block_bytes = max(total * 2, 1 << 16)
            self._host = [torch.zeros(self._block_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self._dev = torch.zeros(self._block_bytes, dtype=torch.uint8, device=self.device)
            self._events, self._turn = [None, None], 0
        t = self._turn
        self._turn ^= 1
        if self._events[t] is not None:
            self._events[t].synchronize()
        host = self._host[t]
        hv = host.numpy()
        hv[:jbytes] = np.frombuffer(structs, dtype=np.uint8)
        hv[jbytes:total].view(np.int32)[:] = np.concatenate(parts)
        ts = torch.cuda.current_stream(self.device)          # the copy and the kernels are ordered on torch's current stream
        self._dev[:total].copy_(host[:total], non_blocking=True)
        if self._events[t] is None:
            self._events[t] = torch.cuda.Event()
        self._events[t].record()
        if out is None:
            out = torch.empty(B, 3, S, S, dtype=dtype, device=self.device)
        assert out.shape == (B, 3, S, S) and out.dtype == dtype and out.is_contiguous() and out.device == self.device
        rc = getattr(self.lib, entry)(self._dev.data_ptr(), hv.ctypes.data, B, self._dev.data_ptr() + jbytes, S, self.filter,
                                      self._tmp.data_ptr(), self.max_rows, self._img.data_ptr(), self._mean.data_ptr(), out.data_ptr(),
                                      ts.cuda_stream)
        _lib.check(rc, entry)
        return out


# ------------------------------------------------------------------------------------------------ reference-named constructors
class _Transform:
    """Callable in the shape of the reference's composed transform, but batched: `tf(images)` draws one job per image and returns the
    device batch; `tf(images, jobs)` runs jobs drawn by the caller.  `tf.last_jobs` keeps the draws (tests replay them through Pillow)."""

    def __init__(self, make_job, image_size, device, **kw):
        self.make_job, self.image_size = make_job, image_size
        self.pipe = InputPipeline(image_size, device, **kw)
        self.last_jobs: List[Dict] = []

    def __call__(self, images: Sequence[torch.Tensor], jobs: Optional[Sequence[Dict]] = None) -> torch.Tensor:
        """jobs: already drawn (a data-parallel rank draws the global batch's and passes those of its images); None: drawn here."""
        self.last_jobs = [self.make_job(int(im.shape[0]), int(im.shape[1])) for im in images] if jobs is None else list(jobs)
        return self.pipe.run(images, self.last_jobs)


def get_train_transforms(image_size: int = 256, use_gray_world: bool = False, device="cuda", **kw) -> _Transform:
    """transforms.py:30-39 (use_gray_world is accepted and unused there too)."""
    return _Transform(lambda h, w: train_job(h, w, image_size, (0.85, 1.0)), image_size, device, **kw)


def get_eval_transforms(image_size: int = 256, device="cuda", **kw) -> _Transform:
    """transforms.py:42-49."""
    return _Transform(lambda h, w: eval_job(h, w, image_size), image_size, device, **kw)


def basic_image_tf(load_size: int, crop_size: int, train: bool, device="cuda", **kw) -> _Transform:
    """Basic_GAN/src/data.py:8-26 `_image_tf`."""
    return _Transform(lambda h, w: basic_job(h, w, load_size, crop_size, train), crop_size, device, **kw)


# ------------------------------------------------------------------------------------------------ a folder decoded once
DEFAULT_CACHE_GB = 8            # mi355x.dataset_cache_gb: the Kaggle folders of both reference configs decode to 1.44 GB
ARENA_ALIGN = 256               # every image starts at a multiple of this, as separate tensors from the caching allocator did
STAGE_BYTES = 64 << 20          # pinned staging buffer of one upload chunk (two of them, used in turn)
DECODE_CHUNK = 256              # files per JpegDecoder.decode call: the entropy decode is one lane per restart segment, so its
                                # throughput comes from the number of files in flight


def _decode(path) -> np.ndarray:
    """The reference's decode (`Image.open(p).convert("RGB")`, dataset_unpaired.py / data.py:40) as a writable uint8 (H, W, 3) array."""
    from PIL import Image
    try:
        with Image.open(path) as im:
            return np.array(im.convert("RGB"))
    except Exception as e:          # never skipped: the run stops and names the file
        raise OSError(f"cannot decode image {path}: {e}") from e


def _header_size(path) -> Tuple[int, int]:
    from PIL import Image
    try:
        with Image.open(path) as im:
            w, h = im.size
    except Exception as e:
        raise OSError(f"cannot open image {path}: {e}") from e
    return int(h), int(w)


# ------------------------------------------------------------------------------------------------ baseline JPEGs decoded on the device
_JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


# What the two JPEG parsers share.  Each helper returns None for what the device does not take, and the parser returns None with it.
def _jpeg_segment(data: bytes, pos: int):
    """(marker, L, body) of the marker segment at `pos`; EOI, which has no length, is (0xD9, 0, b"")."""
    n = len(data)
    if pos + 2 > n or data[pos] != 0xFF:
        return None
    if data[pos + 1] == 0xD9:
        return 0xD9, 0, b""
    if pos + 4 > n:
        return None
    L = (data[pos + 2] << 8) | data[pos + 3]
    return None if L < 2 or pos + 2 + L > n else (data[pos + 1], L, data[pos + 4:pos + 2 + L])


def _dqt_tables(body) -> Optional[Dict]:
    """{slot: uint16 [64] in natural order} of a DQT body: 8-bit tables in slots 0 .. 3."""
    qt = {}
    while body:
        if body[0] >> 4 != 0 or (body[0] & 15) > 3 or len(body) < 65:
            return None
        q = np.zeros(64, np.uint16)
        q[list(_JPEG_ZIGZAG)] = np.frombuffer(body[1:65], np.uint8)
        qt[body[0] & 15] = q
        body = body[65:]
    return qt


def _huffman_counts_legal(body) -> Optional[int]:
    """Symbols of the DHT table at the head of `body`, or None when its counts over-subscribe the code space or exceed 256 / the body."""
    counts = body[1:17]
    total, code = sum(counts), 0
    for l in range(16):
        code += counts[l]
        if code > (1 << (l + 1)):
            return None
        code <<= 1
    return None if total > 256 or len(body) < 17 + total else total


def _dht_tables(body, max_id: int) -> Optional[List]:
    """[(class, id, counts and symbols)] of a DHT body, in its order; ids above `max_id` (baseline: 1, progressive: 3) are refused."""
    tables = []
    while body:
        if len(body) < 17 or body[0] >> 4 > 1 or (body[0] & 15) > max_id:
            return None
        total = _huffman_counts_legal(body)
        if total is None:
            return None
        tables.append((body[0] >> 4, body[0] & 15, body[1:17 + total]))
        body = body[17 + total:]
    return tables


def _sof_frame(body):
    """(H, W, [(id, h, v, quantisation slot)]) of a frame header with 8-bit samples."""
    if len(body) < 6 or body[0] != 8 or len(body) != 6 + 3 * body[5]:
        return None
    return (body[1] << 8) | body[2], (body[3] << 8) | body[4], [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(body[5])]


def _luma_sampling(comps) -> Optional[Tuple[int, int]]:
    """(hmax, vmax) of the component classes the device takes: one component sampled 1x1, or components 1, 2, 3 with chroma 1x1 and luma
    1x1, 2x1 or 2x2."""
    if len(comps) == 1:
        return (1, 1) if comps[0][1:3] == (1, 1) else None
    if len(comps) != 3 or tuple(c[0] for c in comps) != (1, 2, 3) or comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1) or comps[0][1:3] not in ((1, 1), (2, 1), (2, 2)):
        return None
    return comps[0][1:3]


def _other_segment(m: int, body, ri: int) -> Optional[int]:
    """The restart interval behind a segment that is neither tables, frame nor scan: DRI sets it, APPn and COM pass; None: a DRI of another
    length, an Adobe APP14, any other marker."""
    if m == 0xDD:
        return (body[0] << 8) | body[1] if len(body) == 2 else None
    if m == 0xEE and body[:5] == b"Adobe":
        return None
    return ri if 0xE0 <= m <= 0xEF or m == 0xFE else None


def _markers(arr: np.ndarray, start: int):
    """(positions, codes) of the markers in arr[start:], stuffed 0xFF 0x00 bytes left out, in one vectorised search."""
    ff = np.flatnonzero(arr[start:len(arr) - 1] == 0xFF) + start
    nxt = arr[ff + 1]
    return ff[nxt != 0], nxt[nxt != 0]


def _scan_end(mpos, mk, sb: int):
    """(positions of the RSTn markers of the scan that begins at sb, position of the first other marker behind it)."""
    i0 = int(np.searchsorted(mpos, sb))
    other = np.flatnonzero((mk[i0:] & 0xF8) != 0xD0)
    if other.size == 0:
        return None
    e = i0 + int(other[0])
    return mpos[i0:e], int(mpos[e])


def _segments(sb: int, rst, end: int):
    """(seg_begin, seg_end) of a scan's restart segments: the entropy-coded bytes between its RSTn markers."""
    return np.concatenate([[sb], rst + 2]).astype(np.int64), np.concatenate([rst, [end]]).astype(np.int64)


def parse_jpeg(data: bytes) -> Optional[Dict]:
    """The plan of a file the device decoder takes, or None ("not mine": Pillow decodes it).  Accepted: SOF0, 8-bit samples, 8-bit
    quantisation tables, one interleaved scan of all components with Ss = 0, Se = 63, Ah = Al = 0; one component sampled 1x1, or
    components 1, 2, 3 with chroma 1x1 and luma 1x1, 2x1 or 2x2; no Adobe APP14; DHT counts that sum to at most 256 and do not
    over-subscribe the code space; an EOI after the scan, with nothing but RSTn markers and stuffed 0xFF bytes before it, and as many
    RSTn as the restart interval asks.  Anything else -- progressive, arithmetic, 12-bit, CMYK, 4:1:1 / 4:4:0, several scans, DNL, fill
    bytes, an unknown marker, a truncated file, another format -- is None."""
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return None
    pos, qt, dht, sof, ri = 2, {}, {}, None, 0
    while True:
        seg = _jpeg_segment(data, pos)
        if seg is None:
            return None
        m, L, body = seg
        if m == 0xDB:
            tables = _dqt_tables(body)
            if tables is None:
                return None
            qt.update(tables)
        elif m == 0xC4:
            tables = _dht_tables(body, 1)
            if tables is None:
                return None
            dht.update({2 * tc + th: raw for tc, th, raw in tables})
        elif m == 0xC0:
            sof = _sof_frame(body) if sof is None else None      # a second frame header is refused
            if sof is None:
                return None
        elif m == 0xDA:
            break
        else:
            ri = _other_segment(m, body, ri)
            if ri is None:
                return None
        pos += 2 + L
    if sof is None:
        return None
    H, W, comps = sof
    sampling = _luma_sampling(comps)
    if H < 1 or W < 1 or sampling is None or len(body) != 4 + 2 * len(comps) or body[0] != len(comps):
        return None
    if tuple(body[-3:]) != (0, 63, 0):
        return None
    hmax, vmax = sampling
    dc_tab, ac_tab, q_tab = [0, 0, 0], [2, 2, 2], [0, 0, 0]
    for c, (cid, _, _, tq) in enumerate(comps):
        sel, tabs = body[1 + 2 * c], body[2 + 2 * c]
        td, ta = tabs >> 4, tabs & 15
        if sel != cid or td > 1 or ta > 1 or td not in dht or 2 + ta not in dht or tq not in qt:
            return None
        dc_tab[c], ac_tab[c], q_tab[c] = td, 2 + ta, tq
    sb = pos + 2 + L
    found = _scan_end(*_markers(np.frombuffer(data, np.uint8), sb), sb)      # stuffed bytes, RSTn and the end of the scan
    if found is None or data[found[1] + 1] != 0xD9:
        return None
    rst, end = found
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    per = ri if ri else mcux * mcuy
    nseg = -(-mcux * mcuy // per)
    if rst.size != nseg - 1:
        return None
    begins, ends = _segments(sb, rst, end)
    return {"format": "jpeg", "H": H, "W": W, "ncomp": len(comps), "hmax": hmax, "vmax": vmax, "mcux": mcux, "mcuy": mcuy, "qt": qt, "dht": dht,
            "dc_tab": dc_tab, "ac_tab": ac_tab, "q_tab": q_tab, "scan": (sb, end), "seg_begin": begins, "seg_end": ends, "per": per, "data": data}


PROG_MAX_SCANS = PROG_MAX_TABLES = 64           # GAN_JPEGPROG_MAX_SCANS, GAN_JPEGPROG_MAX_TABLES


def parse_jpeg_progressive(data: bytes) -> Optional[Dict]:
    """The plan of a progressive file the device decoder takes, or None ("not mine": Pillow decodes it).  Accepted: SOF2, 8-bit samples,
    8-bit quantisation tables (all before the first scan), the component classes of `parse_jpeg`, no Adobe APP14, DHT ids 0 .. 3 with
    `parse_jpeg`'s legality checks; between scans only DHT, DRI, APPn and COM, which take effect for the following scans -- a DHT that
    is defined again is a new table *version*, and a scan names versions.  The scan script must be one libjpeg decodes without a
    warning and without work for its block smoothing: a DC scan (Ss = Se = 0) holds all components interleaved or one component; an AC
    scan (1 <= Ss <= Se <= 63) holds one component and comes after that component's first DC scan; Al <= 13; the first scan that
    touches a (component, coefficient) has Ah = 0, every later one Ah = the previous Al and Al = Ah - 1; at EOI every coefficient of
    every component has reached Al = 0.  Every scan has exactly the RSTn its restart interval and its own MCU / block count ask for,
    EOI follows the last scan, and there are at most PROG_MAX_SCANS scans and PROG_MAX_TABLES table versions.
    Per scan the plan carries comp (-1: all interleaved), Ss, Se, Ah, Al, tab (table version per component, -1: none), per (restart
    interval in the scan's units), units, seg_begin / seg_end, dep (the latest earlier scan that touches one of its (component,
    coefficient) pairs, -1: none) and level (1 + the largest level among all earlier scans that touch one of its pairs)."""
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return None
    arr = np.frombuffer(data, np.uint8)
    pos, qt, slots, versions, sof, ri, scans = 2, {}, {}, [], None, 0, []
    mpos = mk = None
    state = touch = None                       # per (component, coefficient): the Al reached (-1: untouched), the last scan that touched it
    while True:
        seg = _jpeg_segment(data, pos)
        if seg is None:
            return None
        m, L, body = seg
        if m == 0xD9:
            break
        if m == 0xDB:
            tables = None if scans else _dqt_tables(body)      # only before the first scan
            if tables is None:
                return None
            qt.update(tables)
        elif m == 0xC4:
            tables = _dht_tables(body, 3)
            if tables is None or len(versions) + len(tables) > PROG_MAX_TABLES:
                return None
            for tc, th, raw in tables:                         # a slot defined again is a new version; a scan names versions
                slots[(tc, th)] = len(versions)
                versions.append(raw)
        elif m == 0xC2:
            sof = _sof_frame(body) if sof is None else None      # a second frame header is refused
            if sof is None:
                return None
            H, W, comps = sof
            sampling = _luma_sampling(comps)
            if H < 1 or W < 1 or sampling is None:
                return None
            hmax, vmax = sampling
            mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
            state, touch = np.full((len(comps), 64), -1, np.int64), np.full((len(comps), 64), -1, np.int64)
        elif m == 0xDA:
            if sof is None or len(scans) == PROG_MAX_SCANS or not body or len(body) != 4 + 2 * body[0]:
                return None
            ns, (Ss, Se, AhAl) = body[0], body[-3:]
            Ah, Al = AhAl >> 4, AhAl & 15
            ids = [body[1 + 2 * j] for j in range(ns)]
            if ns == 1 and ids[0] in [c[0] for c in comps]:
                comp = [c[0] for c in comps].index(ids[0])
                members = [comp]
            elif ns == len(comps) and ids == [c[0] for c in comps]:
                comp, members = -1, list(range(ns))
            else:
                return None
            if not ((Ss == 0 and Se == 0) or (1 <= Ss <= Se <= 63 and comp >= 0)) or Al > 13:
                return None
            before = state[members, Ss:Se + 1]
            if Ah == 0:
                if (before != -1).any():
                    return None
            elif Al != Ah - 1 or (before != Ah).any():
                return None
            if Ss > 0 and state[comp, 0] < 0:
                return None
            tab = [-1, -1, -1]
            for j, c in enumerate(members):
                sel = body[2 + 2 * j]
                key = (0, sel >> 4) if Ss == 0 else (1, sel & 15)
                if Ss == 0 and Ah:                     # DC refinement reads raw bits
                    continue
                if key[1] > 3 or key not in slots:
                    return None
                tab[c] = slots[key]
            earlier = touch[members, Ss:Se + 1]
            dep = int(earlier.max())
            level = 1 + max(scans[int(t)]["level"] for t in np.unique(earlier) if t >= 0) if dep >= 0 else 0
            state[members, Ss:Se + 1], touch[members, Ss:Se + 1] = Al, len(scans)
            sb = pos + 2 + L
            if mpos is None:                           # one vectorised search for every scan: stuffed bytes, RSTn and the markers behind the scans
                mpos, mk = _markers(arr, sb)
            found = _scan_end(mpos, mk, sb)
            if found is None:
                return None
            rst, end = found
            if comp < 0:
                units = mcux * mcuy
            else:
                h, v = comps[comp][1:3]
                units = -(-(-(-W * h // hmax)) // 8) * -(-(-(-H * v // vmax)) // 8)
            per = ri if ri else units
            if rst.size != -(-units // per) - 1:
                return None
            begins, ends = _segments(sb, rst, end)
            scans.append({"comp": comp, "Ss": Ss, "Se": Se, "Ah": Ah, "Al": Al, "tab": tab, "dep": dep, "level": level, "per": per, "units": units,
                          "seg_begin": begins, "seg_end": ends})
            pos = end
            continue
        else:
            ri = _other_segment(m, body, ri)
            if ri is None:
                return None
        pos += 2 + L
    if not scans or (state != 0).any():
        return None
    q_tab = [0, 0, 0]
    for c, (_, _, _, tq) in enumerate(comps):
        if tq not in qt:
            return None
        q_tab[c] = tq
    return {"format": "jpegprog", "H": H, "W": W, "ncomp": len(comps), "hmax": hmax, "vmax": vmax, "mcux": mcux, "mcuy": mcuy, "qt": qt, "q_tab": q_tab,
            "versions": versions, "scans": scans, "nlevel": 1 + max(s["level"] for s in scans), "data": data}


def _is_progressive(data: bytes) -> bool:
    """Whether a JPEG's frame header is SOF2 (a walk over its marker segments up to the frame or the first scan)."""
    pos, n = 2, len(data)
    if data[:2] != b"\xff\xd8":
        return False
    while pos + 4 <= n and data[pos] == 0xFF:
        m = data[pos + 1]
        if m == 0xC2:
            return True
        if m in (0xDA, 0xD9) or 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return False
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return False


class _DecoderBase:
    """What the device decoders share: the buffers, and a `decode` that sends every source to the decoder whose parser takes it and
    everything else, and every file a kernel flagged, through `_decode` (Pillow)."""

    def __init__(self, device, ops=None):
        from . import autograd as AG
        self.device = normalize_device(device)
        self.ops = AG._OPS_FACTORY(self.device) if ops is None else ops
        if getattr(self.ops, "is_hip", False) and self.device.type != "cuda":
            raise GanError("the MI355X path needs tensors on a GPU (there is no CPU fallback)")
        self.stats = {"device": 0, "unsupported": 0, "flagged": 0}
        self.last_errors: Dict[int, int] = {}          # source index -> error word, of the last call
        self.last_block = None
        self._host = self._dev = self._ws = self._err = None

    def _grow(self, name: str, nbytes: int, dtype=torch.uint8, host=False):
        t = getattr(self, name)
        if t is None or t.numel() < nbytes:
            n = max(int(nbytes * 1.5), 1 << 16)
            t = torch.zeros(n, dtype=dtype, pin_memory=True) if host and self.device.type == "cuda" else torch.zeros(n, dtype=dtype, device="cpu" if host else self.device)
            setattr(self, name, t)
        return t

    def load(self, source):
        """(bytes, plan or None) of a path or of bytes: the part of `decode` that a thread pool can do ahead."""
        data = bytes(source) if isinstance(source, (bytes, bytearray, memoryview)) else open(os.fspath(source), "rb").read()
        return data, self.parse(data)

    def _routes(self) -> Dict:
        """{plan format: (the decoder that launches such plans, then every other decoder whose `stats` count them too)}, in launch order.
        A decoder that launches its own plans takes every plan it is given."""
        return {None: (self,)}

    @staticmethod
    def _is_mine(data: bytes) -> bool:
        """Whether a source this decoder's parser refused is of its format (a member decoder counts those as `unsupported`)."""
        raise NotImplementedError

    def _groups(self, plans):
        """[(decoder, indices of the sources it takes)]."""
        return [(ds[0], [i for i, p in enumerate(plans) if p is not None and (fmt is None or p["format"] == fmt)]) for fmt, ds in self._routes().items()]

    def _count(self, groups, loaded, rest):
        counted = {ds[0]: ds for ds in self._routes().values()}
        for d, idx in groups:
            bad = sum(1 for i in idx if i in d.last_errors)
            for c in counted[d]:
                c.stats["device"] += len(idx) - bad
                c.stats["flagged"] += bad
        self.stats["unsupported"] += len(rest)                   # every source that went to Pillow unparsed; a member counts its own format's
        for d in {c for ds in counted.values() for c in ds} - {self}:
            d.stats["unsupported"] += sum(1 for i in rest if d._is_mine(loaded[i][0]))

    def _upload(self, total: int):
        """The staging buffer's first `total` bytes on the device (the buffer itself on a CPU device)."""
        if self.device.type != "cuda":
            return self._host
        dev = self._grow("_dev", total)
        dev[:total].copy_(self._host[:total], non_blocking=True)
        return dev

    def _launched(self, launches):
        try:
            launches()
        except GanError:
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()      # the upload has left the staging buffer before it is reused
            raise

    @torch.inference_mode()
    def decode(self, sources: Sequence, out: Optional[torch.Tensor] = None, offsets: Optional[Sequence[int]] = None, each=None) -> List[torch.Tensor]:
        """sources: paths or bytes, any number.  out / offsets: a flat uint8 tensor on the decoder's device and the byte offset of every
        image in it (the store's arena); None: one new buffer, every image at a multiple of ARENA_ALIGN.  each: a `map` for the host work
        per file (reading and parsing; Pillow's decode of what is not the device's), e.g. a thread pool's.  Returns (H, W, 3) views."""
        import io
        each = map if each is None else each
        sources = list(sources)
        is_bytes = lambda s: isinstance(s, (bytes, bytearray, memoryview))
        host_decode = lambda i: _decode(io.BytesIO(bytes(sources[i])) if is_bytes(sources[i]) else sources[i])
        loaded = list(each(self.load, sources))
        plans = [p for _, p in loaded]
        every = self._groups(plans)
        groups = [(d, idx) for d, idx in every if idx]
        rest = [i for i, p in enumerate(plans) if p is None]
        arrs = dict(zip(rest, each(host_decode, rest)))
        shapes = [(plans[i]["H"], plans[i]["W"]) if plans[i] is not None else arrs[i].shape[:2] for i in range(len(sources))]
        if out is None:
            offsets, end = [], 0
            for h, w in shapes:
                offsets.append(end)
                end += -(-(h * w * 3) // ARENA_ALIGN) * ARENA_ALIGN
            out = torch.empty(max(end, 1), dtype=torch.uint8, device=self.device)
        elif offsets is None or len(offsets) != len(sources) or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != self.device:
            raise GanError(f"{type(self).__name__}.decode: `out` must be a flat contiguous uint8 tensor on {self.device} with one offset per source")
        self.last_errors = {}
        for d, _ in every:
            if d is not None:
                d.last_errors = {}
        if groups:                                               # every launch of the call, then one download of all error words
            err, at = self._grow("_err", sum(len(idx) for _, idx in groups), torch.int32), 0
            for d, idx in groups:
                d._launch([plans[i] for i in idx], [offsets[i] for i in idx], out, err[at:at + len(idx)])
                at += len(idx)
            words = err[:at].cpu().tolist()                      # it also orders the staging buffers' reuse
            for d, idx in groups:
                d.last_errors = {i: int(w) for i, w in zip(idx, words[:len(idx)]) if w}
                self.last_errors.update(d.last_errors)
                words = words[len(idx):]
        flagged = sorted(self.last_errors)
        for i, a in zip(flagged, each(host_decode, flagged)):    # Pillow's pixels, or its OSError
            if a.shape[:2] != shapes[i]:
                raise OSError(f"image {sources[i]!r} decoded to {a.shape[:2]}, its header said {shapes[i]}")
            arrs[i] = a
        for i, a in arrs.items():
            out[offsets[i]:offsets[i] + a.size].copy_(torch.from_numpy(a).reshape(-1))
        self._count(groups, loaded, rest)
        return [out[o:o + h * w * 3].view(h, w, 3) for o, (h, w) in zip(offsets, shapes)]


def _pack_jpeg_images(dec: _DecoderBase, plans: Sequence[Dict], out_offsets: Sequence[int], spans: Sequence[Tuple[int, int]], o_qt: int, o_data: int):
    """What the upload blocks of both JPEG decoders hold alike, into `dec`'s staging buffer: per image the geometry, quantisation slots and
    out_off of its GanJpegdecImage, its quantisation tables from o_qt on, and bytes spans[i] = (first, end) of its file from o_data on, every
    image's at a multiple of 16.  -> (block bytes, the staging buffer, the descriptors, per image: block offset - file offset of its bytes)."""
    imgs = (_lib.GanJpegdecImage * len(plans))()
    total = o_data + sum(-(-(se - sb) // 16) * 16 for sb, se in spans)
    host = dec._grow("_host", total, host=True).numpy()
    host[o_qt:o_data] = 0
    at, shifts = o_data, []
    for i, (p, im, (sb, se)) in enumerate(zip(plans, imgs, spans)):
        im.ncomp, im.H, im.W, im.hmax, im.vmax, im.mcux, im.mcuy = p["ncomp"], p["H"], p["W"], p["hmax"], p["vmax"], p["mcux"], p["mcuy"]
        for c in range(3):
            im.q_tab[c] = p["q_tab"][c]
        im.out_off = int(out_offsets[i])
        for t, q in p["qt"].items():
            host[o_qt + (4 * i + t) * 128:o_qt + (4 * i + t + 1) * 128].view(np.uint16)[:] = q
        host[at:at + se - sb] = np.frombuffer(p["data"], np.uint8, se - sb, sb)
        shifts.append(at - sb)
        at += -(-(se - sb) // 16) * 16
    return total, host, imgs, shifts


class JpegDecoder(_DecoderBase):
    """Baseline JPEG files -> packed uint8 (H, W, 3) tensors on `device`, pixel-identical to `_decode` (Pillow) for every source.  The
    files `parse` accepts are decoded by csrc/jpegdec.hip: their descriptors, tables and scan bytes go up in one copy from one pinned
    staging buffer, four launches decode any number of files together, and the host reads one error word per file.  Every other
    source, and every file the kernels flagged, goes through `_decode` -- which returns Pillow's pixels or raises its OSError, as
    without the decoder.  Owns and grows its buffers, like InputPipeline.  `stats` counts which way the sources went.
    progressive: the progressive files `parse_jpeg_progressive` accepts are decoded on the device too (csrc/jpegprog.hip), in the same
    call and into the same `out`, with one launch sequence of their own; they count under `stats` like the baseline ones, and
    `progressive_stats` says how many of each count were progressive (`unsupported`: SOF2 files the parser refused)."""

    def __init__(self, device, ops=None, progressive: bool = False):
        super().__init__(device, ops)
        self.progressive = bool(progressive)
        self._prog = _ProgressiveJpeg(self.device, self.ops) if self.progressive else None
        self.progressive_stats = self._prog.stats if self._prog is not None else {"device": 0, "unsupported": 0, "flagged": 0}

    @staticmethod
    def parse(data: bytes) -> Optional[Dict]:
        return parse_jpeg(data)

    def load(self, source):
        data, plan = super().load(source)
        if plan is None and self.progressive:
            plan = parse_jpeg_progressive(data)
        return data, plan

    def _routes(self):
        """The progressive group's counts go into this decoder's `stats` too; the refused SOF2 files into `progressive_stats`."""
        return super()._routes() if self._prog is None else {"jpeg": (self,), "jpegprog": (self._prog, self)}

    @staticmethod
    def _is_mine(data: bytes) -> bool:
        return data[:2] == b"\xff\xd8"

    def _pack(self, plans: Sequence[Dict], out_offsets: Sequence[int]):
        """The upload block of `plans` in the staging buffer -> (block bytes, images, segments, workspace bytes)."""
        n = len(plans)
        nseg = sum(len(p["seg_begin"]) for p in plans)
        o_seg, o_dht, o_qt, o_scan = self.ops.jpegdec_block_offsets(n, nseg)
        total, host, imgs, shifts = _pack_jpeg_images(self, plans, out_offsets, [p["scan"] for p in plans], o_qt, o_scan)
        host[o_dht:o_qt] = 0
        segs = np.zeros((nseg, 5), np.int32)
        s0 = 0
        for i, (p, im, shift) in enumerate(zip(plans, imgs, shifts)):
            k = len(p["seg_begin"])
            im.seg_first, im.seg_count = s0, k
            for c in range(3):
                im.dc_tab[c], im.ac_tab[c] = p["dc_tab"][c], p["ac_tab"][c]
            segs[s0:s0 + k, 0] = i
            segs[s0:s0 + k, 1] = np.arange(k) * p["per"]
            segs[s0:s0 + k, 2] = np.minimum(p["per"], p["mcux"] * p["mcuy"] - segs[s0:s0 + k, 1])
            segs[s0:s0 + k, 3], segs[s0:s0 + k, 4] = p["seg_begin"] + shift, p["seg_end"] + shift
            for t, raw in p["dht"].items():
                host[o_dht + (4 * i + t) * 272:o_dht + (4 * i + t) * 272 + len(raw)] = np.frombuffer(raw, np.uint8)
            s0 += k
        ws_bytes = self.ops.jpegdec_bounds(imgs)
        host[:o_seg] = np.frombuffer(imgs, np.uint8)
        host[o_seg:o_dht].view(np.int32)[:] = segs.reshape(-1)
        return total, n, nseg, ws_bytes

    def _launch(self, plans: Sequence[Dict], offsets: Sequence[int], out: torch.Tensor, err: torch.Tensor) -> None:
        """Packs, uploads and launches the decode of `plans` into `out`; err (int32, one per plan, on the device) receives the error words."""
        total, n, nseg, ws_bytes = self._pack(plans, offsets)
        self.last_block = (total, n, nseg)                   # the staging buffer and the workspace still hold this call (tests locate a difference there)
        ws = self._grow("_ws", ws_bytes)
        dev, o = self._upload(total), self.ops

        def launches():
            o.jpegdec_tables(dev, self._host, total, n, nseg, ws)
            o.jpegdec_entropy(dev, self._host, total, n, nseg, ws)
            o.jpegdec_idct(dev, self._host, total, n, nseg, ws)
            o.jpegdec_pixels(dev, self._host, total, n, nseg, ws, out, err)
        self._launched(launches)


class _ProgressiveJpeg(_DecoderBase):
    """The progressive group of a JpegDecoder: its own staging buffer and workspace (both groups are in flight in one call), the packing
    of `parse_jpeg_progressive`'s plans into the block of csrc/jpegprog.hip, and its four launches.  `stats` is the owner's
    `progressive_stats`."""

    @staticmethod
    def _is_mine(data: bytes) -> bool:
        return _is_progressive(data)

    def _pack(self, plans: Sequence[Dict], out_offsets: Sequence[int]):
        """The upload block of `plans` in the staging buffer -> (block bytes, images, scans, segments, table versions, workspace bytes)."""
        n = len(plans)
        nscan = sum(len(p["scans"]) for p in plans)
        nseg = sum(len(sc["seg_begin"]) for p in plans for sc in p["scans"])
        nver = sum(len(p["versions"]) for p in plans)
        o_pimg, o_scan, o_seg, o_dht, o_qt, o_data = self.ops.jpegprog_block_offsets(n, nscan, nseg, nver)
        spans = [(int(p["scans"][0]["seg_begin"][0]), int(p["scans"][-1]["seg_end"][-1])) for p in plans]      # first scan byte .. last scan's end
        total, host, imgs, shifts = _pack_jpeg_images(self, plans, out_offsets, spans, o_qt, o_data)
        pimg, scans, segs = np.zeros((n, 8), np.int32), np.zeros((nscan, 16), np.int32), np.zeros((nseg, 8), np.int32)
        host[:o_pimg] = 0
        host[o_dht:o_qt] = 0
        c0 = s0 = v0 = 0
        for i, (p, im, shift) in enumerate(zip(plans, imgs, shifts)):
            for c in range(3):
                im.dc_tab[c], im.ac_tab[c] = 0, 2
            k = sum(len(sc["seg_begin"]) for sc in p["scans"])
            pimg[i] = (c0, len(p["scans"]), s0, k, v0, len(p["versions"]), p["nlevel"], 0)
            for j, sc in enumerate(p["scans"]):
                scans[c0 + j, :11] = (i, sc["comp"], sc["Ss"], sc["Se"], sc["Ah"], sc["Al"], sc["tab"][0], sc["tab"][1], sc["tab"][2], sc["dep"], sc["level"])
            for j in sorted(range(len(p["scans"])), key=lambda j: p["scans"][j]["level"]):              # stable: file order inside a level
                sc = p["scans"][j]
                m = len(sc["seg_begin"])
                rows = segs[s0:s0 + m]
                rows[:, 0], rows[:, 1], rows[:, 2] = i, c0 + j, np.arange(m)
                rows[:, 3] = np.arange(m) * sc["per"]
                rows[:, 4] = np.minimum(sc["per"], sc["units"] - rows[:, 3])
                rows[:, 5], rows[:, 6] = sc["seg_begin"] + shift, sc["seg_end"] + shift
                s0 += m
            for t, raw in enumerate(p["versions"]):
                host[o_dht + (v0 + t) * 272:o_dht + (v0 + t) * 272 + len(raw)] = np.frombuffer(raw, np.uint8)
            c0, v0 = c0 + len(p["scans"]), v0 + len(p["versions"])
        ws_bytes = self.ops.jpegprog_bounds(imgs, nver)
        host[:n * C.sizeof(_lib.GanJpegdecImage)] = np.frombuffer(imgs, np.uint8)
        host[o_pimg:o_scan].view(np.int32)[:] = pimg.reshape(-1)
        host[o_scan:o_seg].view(np.int32)[:] = scans.reshape(-1)
        host[o_seg:o_dht].view(np.int32)[:] = segs.reshape(-1)
        return total, n, nscan, nseg, nver, ws_bytes

    def _launch(self, plans: Sequence[Dict], offsets: Sequence[int], out: torch.Tensor, err: torch.Tensor) -> None:
        total, n, nscan, nseg, nver, ws_bytes = self._pack(plans, offsets)
        self.last_block = (total, n, nscan, nseg, nver)
        ws = self._grow("_ws", ws_bytes)
        dev, o = self._upload(total), self.ops
        counts = (n, nscan, nseg, nver)

        def launches():
            o.jpegprog_tables(dev, self._host, total, counts, ws)
            o.jpegprog_entropy(dev, self._host, total, counts, ws)
            o.jpegprog_idct(dev, self._host, total, counts, ws)
            o.jpegprog_pixels(dev, self._host, total, counts, ws, out, err)
        self._launched(launches)


# ------------------------------------------------------------------------------------------------ PNGs decoded on the device
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# Ancillary chunks that Pillow itself parses.  It raises for one that is shorter than it needs, and for text and profiles it has limits of
# its own, so the parser passes over only what cannot change Pillow's outcome: these four at exactly their length, a tRNS of the right
# length for its colour type, a little plain text; every chunk type Pillow has no handler for is read and dropped by it whatever it holds.
_PNG_FIXED_LENGTH = {b"gAMA": 4, b"cHRM": 32, b"sRGB": 1, b"pHYs": 9}
_PNG_NOT_MINE = (b"acTL", b"fcTL", b"fdAT", b"iCCP", b"zTXt", b"iTXt", b"eXIf")
_PNG_MAX_TEXT = 1 << 16         # bytes of tEXt chunks in one file (Pillow's own limit on text is 64 MiB)
PNG_MAX_PIXELS = 89478485       # Pillow's Image.MAX_IMAGE_PIXELS: above it Pillow warns or raises, so such a file stays Pillow's


def parse_png(data: bytes) -> Optional[Dict]:
    """The plan of a file the device decoder takes, or None ("not mine": Pillow decodes it).  Accepted: no interlace, compression and
    filter method 0; colour type 0, 2, 4 or 6 at 8 bits, or colour type 3 at 1, 2, 4 or 8 bits with a PLTE of at least 1 << depth
    entries (no index can leave it); every chunk's type four letters and its CRC right; IHDR first, PLTE before the IDATs, the IDATs in one
    run, IEND last and nothing behind it; no unknown critical chunk; a zlib header with CM = 8, CINFO <= 7, FDICT = 0 and a valid FCHECK; rows of
    at most _lib.PNGDEC_MAX_ROWBYTES bytes; raw and output bytes below 2^31.  The IDAT payloads are concatenated (empty and 1-byte ones
    included) to the one zlib stream the device reads.  Anything else -- 16-bit samples, grey below 8 bits, Adam7, APNG, a truncated
    file, another format -- is None.  Of the ancillary chunks Pillow parses, gAMA, cHRM, sRGB and pHYs pass at exactly their length, a
    tRNS before the IDATs at the length of its colour type (RGB: 6; palette: 1 .. PLTE entries; none in grey or with alpha) and up to 64 KiB of
    tEXt; acTL, fcTL, fdAT, iCCP, zTXt, iTXt and eXIf are None (Pillow raises for malformed ones and has limits of its own for the compressed
    ones).  Chunk types Pillow has no handler for are passed over, as Pillow drops them unread.  None of these changes convert("RGB")."""
    import zlib
    n = len(data)
    if n < 8 or data[:8] != _PNG_SIGNATURE:
        return None
    view = memoryview(data)
    pos, ihdr, plte, idat, state, trns, text = 8, None, None, [], 0, False, 0      # state: 0 before the IDATs, 1 among them, 2 behind them
    while True:
        if pos + 12 > n:
            return None
        L, typ = int.from_bytes(data[pos:pos + 4], "big"), bytes(data[pos + 4:pos + 8])
        if not typ.isalpha() or pos + 12 + L > n or zlib.crc32(view[pos + 4:pos + 8 + L]) != int.from_bytes(data[pos + 8 + L:pos + 12 + L], "big"):
            return None
        if ihdr is None:
            if typ != b"IHDR" or L != 13:
                return None
            ihdr = (int.from_bytes(data[pos + 8:pos + 12], "big"), int.from_bytes(data[pos + 12:pos + 16], "big")) + tuple(data[pos + 16:pos + 21])
        elif typ == b"IDAT":
            if state == 2:
                return None
            state = 1
            idat.append(view[pos + 8:pos + 8 + L])
        else:
            state = 2 if state else 0
            if typ == b"IEND":
                if L != 0 or pos + 12 != n:
                    return None
                break
            if typ == b"PLTE":
                if plte is not None or state != 0 or L == 0 or L % 3 or L > 768:
                    return None
                plte = bytes(view[pos + 8:pos + 8 + L])
            elif not typ[0] & 0x20 or typ in _PNG_NOT_MINE:      # IHDR again or a critical chunk this parser does not know; APNG, compressed text, profiles
                return None
            elif typ in _PNG_FIXED_LENGTH:
                if L != _PNG_FIXED_LENGTH[typ]:
                    return None
            elif typ == b"tRNS":                                 # before the IDATs, once; six bytes in an RGB file, at most one per PLTE entry in a palette file
                if trns or state != 0 or not (L == 6 if ihdr[3] == 2 else ihdr[3] == 3 and plte is not None and 1 <= L <= len(plte) // 3):
                    return None
                trns = True
            elif typ == b"tEXt":
                text += L
                if text > _PNG_MAX_TEXT:
                    return None
        pos += 12 + L
    W, H, depth, color, compression, filtering, interlace = ihdr
    if not idat or W < 1 or H < 1 or compression or filtering or interlace or color not in _PNG_CHANNELS:
        return None
    if depth != 8 and not (color == 3 and depth in (1, 2, 4)):
        return None
    if (color == 3 and (plte is None or len(plte) // 3 < 1 << depth)) or (color in (0, 4) and plte is not None):
        return None
    channels = _PNG_CHANNELS[color]
    rowbytes = (W * channels * depth + 7) // 8
    if rowbytes > _lib.PNGDEC_MAX_ROWBYTES or H * (1 + rowbytes) >= 1 << 31 or H * W * 3 >= 1 << 31 or H * W > PNG_MAX_PIXELS:
        return None
    stream = b"".join(idat)
    if not 7 <= len(stream) < 1 << 31:
        return None
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or flg & 0x20 or (cmf << 8 | flg) % 31:
        return None
    return {"format": "png", "H": H, "W": W, "color": color, "depth": depth, "bpp": max(1, channels * depth // 8), "rowbytes": rowbytes,
            "palette": plte if color == 3 else b"", "wbits": (cmf >> 4) + 8, "stream": stream}


class PngDecoder(_DecoderBase):
    """PNG files -> packed uint8 (H, W, 3) tensors on `device`, pixel-identical to `_decode` (Pillow) for every source; the interface
    and the guarantees of `JpegDecoder`.  The files `parse` accepts are decoded by csrc/pngdec.hip: their descriptors, palettes and zlib
    streams go up in one copy from one pinned staging buffer, two launches (inflate; unfilter and convert) decode any number of files
    together, one workgroup per file, and the host reads one error word per file.  Every other source, and every file the kernels
    flagged (a stream zlib would reject, a filter byte above 4, a wrong Adler-32), goes through `_decode`."""

    @staticmethod
    def parse(data: bytes) -> Optional[Dict]:
        return parse_png(data)

    @staticmethod
    def _is_mine(data: bytes) -> bool:
        return data[:8] == _PNG_SIGNATURE

    def _pack(self, plans: Sequence[Dict], out_offsets: Sequence[int]):
        """The upload block of `plans` in the staging buffer -> (block bytes, files, workspace bytes)."""
        n = len(plans)
        imgs = (_lib.GanPngdecImage * n)()
        o_pal, o_stream = self.ops.pngdec_block_offsets(n)
        total = o_stream + sum(-(-len(p["stream"]) // 16) * 16 for p in plans)
        host = self._grow("_host", total, host=True).numpy()
        host[o_pal:o_stream] = 0
        at = o_stream
        for i, (p, im) in enumerate(zip(plans, imgs)):
            im.H, im.W, im.color, im.depth, im.bpp, im.rowbytes, im.wbits = p["H"], p["W"], p["color"], p["depth"], p["bpp"], p["rowbytes"], p["wbits"]
            im.pal_count, im.stream_off, im.stream_len, im.out_off = len(p["palette"]) // 3, at, len(p["stream"]), int(out_offsets[i])
            end = at + -(-len(p["stream"]) // 16) * 16
            host[at:at + len(p["stream"])] = np.frombuffer(p["stream"], np.uint8)
            host[at + len(p["stream"]):end] = 0
            host[o_pal + 768 * i:o_pal + 768 * i + len(p["palette"])] = np.frombuffer(p["palette"], np.uint8)
            at = end
        ws_bytes = self.ops.pngdec_bounds(imgs)
        host[:o_pal] = np.frombuffer(imgs, np.uint8)
        return total, n, ws_bytes

    def _launch(self, plans: Sequence[Dict], offsets: Sequence[int], out: torch.Tensor, err: torch.Tensor) -> None:
        total, n, ws_bytes = self._pack(plans, offsets)
        self.last_block = (total, n)
        ws = self._grow("_ws", ws_bytes)
        dev, o = self._upload(total), self.ops

        def launches():
            o.pngdec_inflate(dev, self._host, total, n, ws)
            o.pngdec_pixels(dev, self._host, total, n, ws, out, err)
        self._launched(launches)


class DeviceDecoder(_DecoderBase):
    """Both device decoders behind one `decode`: every source is read once and goes by its content, not its suffix, to `self.jpeg`
    (a JpegDecoder) or `self.png` (a PngDecoder); everything lands in one arena in one call, and the error words of both come back in one
    download.  The sub-decoders keep their own `stats`
    (`unsupported`: files of their format that their parser refused); `self.stats` counts all sources.
    progressive: `self.jpeg` is a JpegDecoder(progressive=True); its progressive group launches in the same call."""

    def __init__(self, device, jpeg: bool = True, png: bool = True, ops=None, progressive: bool = False):
        if not (jpeg or png):
            raise ValueError("DeviceDecoder: at least one of jpeg and png")
        if progressive and not jpeg:
            raise ValueError("DeviceDecoder: progressive needs jpeg")
        super().__init__(device, ops)
        self.jpeg = JpegDecoder(self.device, ops=self.ops, progressive=progressive) if jpeg else None
        self.png = PngDecoder(self.device, ops=self.ops) if png else None
        self.progressive = bool(progressive)

    @property
    def progressive_stats(self):
        return self.jpeg.progressive_stats

    def parse(self, data: bytes) -> Optional[Dict]:
        plan = parse_jpeg(data) if self.jpeg is not None else None
        if plan is None and self.progressive:
            plan = parse_jpeg_progressive(data)
        return parse_png(data) if plan is None and self.png is not None else plan

    def _routes(self):
        routes = {"jpeg": (self.jpeg, self), "jpegprog": (self.jpeg and self.jpeg._prog, self.jpeg, self), "png": (self.png, self)}
        return {fmt: ds for fmt, ds in routes.items() if ds[0] is not None}


class ImageStore:
    """The images of `paths`, decoded once with Pillow on a thread pool, as uint8 (H, W, 3) tensors on `device` -- what
    `InputPipeline.run` reads.  `store[i]` is image i (in the order of `paths`), `store.sizes[i]` its (h, w).

    Resident (the decoded images fit `budget_bytes`; default DEFAULT_CACHE_GB GiB): one uint8 arena holds every image, each at a
    multiple of 256 bytes (`store.offsets`); it is filled chunk by chunk through two pinned staging buffers with non-blocking copies,
    and `store[i]` is a view into it.  Streaming (otherwise): nothing is kept; `store[i]` and `store.fetch(indices)` decode (fetch: on
    the pool) and upload per call.  Both modes hand out the same tensors.  On a CPU device the arena / the fetched images are CPU
    tensors (the drivers' host logic is tested that way; the pipeline itself has no CPU path).
    `folder` only names the place in the error an empty list raises.
    device_decode: the baseline JPEGs among the files are decoded by a `JpegDecoder` on the device -- resident: read and parsed on the
    pool and decoded chunk by chunk (DECODE_CHUNK files) straight into the arena; streaming: `fetch` decodes its batch there.  Every
    other file, and every file the decoder flags, still goes through Pillow; the store holds the same bytes either way.
    device_png: the same for the PNGs among the files, with a `PngDecoder`; with both switches one `DeviceDecoder` takes both formats.
    device_progressive (needs device_decode): the progressive JPEGs the device decoder takes are decoded there too.
    decoder: any object with JpegDecoder's `decode`, used instead of a new one when a switch is on."""

    def __init__(self, paths: Sequence, device, budget_bytes: Optional[int] = None, workers: Optional[int] = None, folder=None,
                 device_decode: bool = False, decoder=None, device_png: bool = False, device_progressive: bool = False):
        self._pool = None
        self._decoder = None
        if device_progressive and not device_decode:
            raise ValueError("device_progressive needs device_decode")
        self.paths = [os.fspath(p) for p in paths]
        if not self.paths:
            raise FileNotFoundError(f"no images found in {os.fspath(folder) if folder is not None else 'the given (empty) list of paths'}")
        self.device = normalize_device(device)
        if device_decode or device_png:
            prog = bool(device_progressive)
            make = (lambda dev: DeviceDecoder(dev, progressive=prog)) if device_decode and device_png else PngDecoder if device_png else (lambda dev: JpegDecoder(dev, progressive=prog))
            self._decoder = decoder if decoder is not None else make(self.device)
        self.workers = max(1, min(16, int(workers) if workers is not None else (os.cpu_count() or 1)))
        self._pool = ThreadPoolExecutor(self.workers)
        self._stage = self._stage_event = None
        try:
            self.sizes: List[Tuple[int, int]] = list(self._pool.map(_header_size, self.paths))
            self.offsets, end = [], 0
            for h, w in self.sizes:
                self.offsets.append(end)
                end += -(-(h * w * 3) // ARENA_ALIGN) * ARENA_ALIGN
            self.nbytes = sum(h * w * 3 for h, w in self.sizes)
            budget = DEFAULT_CACHE_GB << 30 if budget_bytes is None else int(budget_bytes)
            self.resident = end <= budget
            self.arena = None
            if self.resident:
                self._fill(end)
        except BaseException:
            self.close()
            raise
        if self.resident:
            self.close()              # the pool has done its work; streaming keeps it for `fetch`

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __del__(self):
        self.close()

    def __len__(self) -> int:
        return len(self.paths)

    def _checked(self, i: int, arr: np.ndarray) -> np.ndarray:
        if arr.shape != self.sizes[i] + (3,):
            raise OSError(f"image {self.paths[i]} decoded to {arr.shape[:2]}, its header said {self.sizes[i]}")
        return arr

    def _view(self, buf: torch.Tensor, off: int, i: int) -> torch.Tensor:
        h, w = self.sizes[i]
        return buf[off:off + h * w * 3].view(h, w, 3)

    # ---- resident
    def _device_decode(self, idx: Sequence[int], out=None, offsets=None) -> List[torch.Tensor]:
        imgs = self._decoder.decode([self.paths[i] for i in idx], out=out, offsets=offsets, each=self._pool.map)
        for i, im in zip(idx, imgs):
            if tuple(im.shape) != self.sizes[i] + (3,):
                raise OSError(f"image {self.paths[i]} decoded to {tuple(im.shape[:2])}, its header said {self.sizes[i]}")
        return imgs

    def _fill(self, total: int):
        cuda = self.device.type == "cuda"
        self.arena = torch.empty(total, dtype=torch.uint8, device=self.device)
        if self._decoder is not None:
            for first in range(0, len(self), DECODE_CHUNK):
                idx = range(first, min(first + DECODE_CHUNK, len(self)))
                self._device_decode(idx, self.arena, [self.offsets[i] for i in idx])
            if cuda:
                torch.cuda.current_stream(self.device).synchronize()
            return
        if not cuda:
            dst = self.arena.numpy()

            def put(i):
                o, (h, w) = self.offsets[i], self.sizes[i]
                dst[o:o + h * w * 3] = self._checked(i, _decode(self.paths[i])).reshape(-1)
            list(self._pool.map(put, range(len(self))))
            return
        ends = self.offsets[1:] + [total]
        cap = max(STAGE_BYTES, max(e - o for o, e in zip(self.offsets, ends)))
        stages = [torch.empty(min(cap, total), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        events = [None, None]
        first, turn = 0, 0
        while first < len(self):
            last = first                      # images first .. last-1 fit one staging buffer
            while last < len(self) and ends[last] - self.offsets[first] <= stages[0].numel():
                last += 1
            base, stage = self.offsets[first], stages[turn]
            if events[turn] is not None:
                events[turn].synchronize()    # the copy that last read this staging buffer has run
            host = stage.numpy()

            def put(i, host=host, base=base):
                o, (h, w) = self.offsets[i] - base, self.sizes[i]
                host[o:o + h * w * 3] = self._checked(i, _decode(self.paths[i])).reshape(-1)
            list(self._pool.map(put, range(first, last)))
            n = ends[last - 1] - base
            self.arena[base:base + n].copy_(stage[:n], non_blocking=True)
            events[turn] = torch.cuda.Event()
            events[turn].record()
            first, turn = last, turn ^ 1
        torch.cuda.current_stream(self.device).synchronize()      # the staging buffers are released below

    # ---- both modes
    def __getitem__(self, i: int) -> torch.Tensor:
        i = range(len(self))[i]
        if self.resident:
            return self._view(self.arena, self.offsets[i], i)
        if self._decoder is not None:
            return self._device_decode([i])[0]
        return torch.from_numpy(self._checked(i, _decode(self.paths[i]))).to(self.device)

    def fetch(self, indices: Sequence[int]) -> List[torch.Tensor]:
        """`[store[i] for i in indices]`; streaming mode decodes them on the pool and uploads them with one copy."""
        idx = [range(len(self))[i] for i in indices]
        if self.resident:
            return [self._view(self.arena, self.offsets[i], i) for i in idx]
        if self._decoder is not None:
            return self._device_decode(idx)
        arrs = [self._checked(i, a) for i, a in zip(idx, self._pool.map(_decode, [self.paths[i] for i in idx]))]
        if self.device.type != "cuda":
            return [torch.from_numpy(a) for a in arrs]
        offs, end = [], 0
        for a in arrs:
            offs.append(end)
            end += -(-a.size // ARENA_ALIGN) * ARENA_ALIGN
        if self._stage is None or self._stage.numel() < end:
            self._stage, self._stage_event = torch.empty(max(end, 1 << 20), dtype=torch.uint8, pin_memory=True), None
        if self._stage_event is not None:
            self._stage_event.synchronize()
        host = self._stage.numpy()
        for o, a in zip(offs, arrs):
            host[o:o + a.size] = a.reshape(-1)
        dev = torch.empty(end, dtype=torch.uint8, device=self.device)
        dev.copy_(self._stage[:end], non_blocking=True)
        self._stage_event = torch.cuda.Event()
        self._stage_event.record()
        return [self._view(dev, o, i) for o, i in zip(offs, idx)]
