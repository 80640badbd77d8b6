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
            out = torch.empty(B, 3, S, S, dtype=torch.float32, device=self.device)
        assert out.shape == (B, 3, S, S) and out.dtype == torch.float32 and out.is_contiguous() and out.device == self.device
        rc = self.lib.gan_input_pipeline_filter(self._dev.data_ptr(), hv.ctypes.data, B, self._dev.data_ptr() + jbytes, S, self.filter,
                                                self._tmp.data_ptr(), self.max_rows, self._img.data_ptr(), self._mean.data_ptr(), out.data_ptr(),
                                                ts.cuda_stream)
        _lib.check(rc, "gan_input_pipeline_filter")
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


class ImageStore:
    """The images of `paths`, decoded once with Pillow on a thread pool, as uint8 (H, W, 3) tensors on `device` -- what
    `InputPipeline.run` reads.  `store[i]` is image i (in the order of `paths`), `store.sizes[i]` its (h, w).

    Resident (the decoded images fit `budget_bytes`; default DEFAULT_CACHE_GB GiB): one uint8 arena holds every image, each at a
    multiple of 256 bytes (`store.offsets`); it is filled chunk by chunk through two pinned staging buffers with non-blocking copies,
    and `store[i]` is a view into it.  Streaming (otherwise): nothing is kept; `store[i]` and `store.fetch(indices)` decode (fetch: on
    the pool) and upload per call.  Both modes hand out the same tensors.  On a CPU device the arena / the fetched images are CPU
    tensors (the drivers' host logic is tested that way; the pipeline itself has no CPU path).
    `folder` only names the place in the error an empty list raises."""

    def __init__(self, paths: Sequence, device, budget_bytes: Optional[int] = None, workers: Optional[int] = None, folder=None):
        self._pool = None
        self.paths = [os.fspath(p) for p in paths]
        if not self.paths:
            raise FileNotFoundError(f"no images found in {os.fspath(folder) if folder is not None else 'the given (empty) list of paths'}")
        self.device = normalize_device(device)
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
    def _fill(self, total: int):
        cuda = self.device.type == "cuda"
        self.arena = torch.empty(total, dtype=torch.uint8, device=self.device)
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
        return torch.from_numpy(self._checked(i, _decode(self.paths[i]))).to(self.device)

    def fetch(self, indices: Sequence[int]) -> List[torch.Tensor]:
        """`[store[i] for i in indices]`; streaming mode decodes them on the pool and uploads them with one copy."""
        idx = [range(len(self))[i] for i in indices]
        if self.resident:
            return [self._view(self.arena, self.offsets[i], i) for i in idx]
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
