"""Device buffers ("halo-NHWC" views), the op layer over the C ABI, and replayable programs.

Every op constructor returns a zero-argument callable with its ctypes arguments prebuilt, so a training step
is a flat list of kernel launches ("program") replayed on one HIP stream without any Python-side shape logic,
host synchronisation or allocation -- the same list can be captured into a hipGraph.
PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import torch

from . import _lib
from ._lib import ACT_NONE, BF16, F32, FP8, HALO_NONE, HALO_REFLECT, HALO_ZERO, GanAdamTensor, GanConvDesc, GanView, GanWgradDesc

IN_WS_CHUNKS = 96
ADAM_CHUNK = 16384


def check_palette_size(T):
    """palette_prior.low_freq_size: the unbiased standard deviation over T*T cells needs T >= 2 (torch gives NaN for one cell)."""
    if int(T) != T or not 2 <= int(T) <= 1024:
        raise ValueError(f"palette prior: low_freq_size must be an integer in [2, 1024], got {T!r}")


def torch_dtype(code: int):
    return torch.float32 if code == F32 else torch.uint8 if code == FP8 else torch.bfloat16      # FP8: raw e4m3 bytes


class View:
    """A [B][H+2h][W+2h][C] activation buffer with a symmetric spatial halo h."""

    def __init__(self, t: torch.Tensor, B: int, H: int, W: int, C_: int, halo: int, dtype: int):
        self.t, self.B, self.H, self.W, self.C, self.halo, self.dtype = t, B, H, W, C_, halo, dtype
        self.Hp, self.Wp = H + 2 * halo, W + 2 * halo
        assert t.numel() == B * self.Hp * self.Wp * C_ and C_ % (16 if dtype == FP8 else 8) == 0
        self._struct = None

    @property
    def y0(self):
        return self.halo

    @property
    def x0(self):
        return self.halo

    def ptr(self) -> int:
        return self.t.data_ptr()

    def struct(self) -> GanView:
        if self._struct is None:
            self._struct = GanView(self.ptr(), self.B, self.Hp, self.Wp, self.C, self.halo, self.halo, self.H, self.W, self.dtype, 0)
        return self._struct

    def nhwc(self) -> torch.Tensor:
        """Logical interior as a (B,H,W,C) tensor view (tests / debugging)."""
        full = self.t.view(self.B, self.Hp, self.Wp, self.C)
        return full[:, self.halo:self.halo + self.H, self.halo:self.halo + self.W, :]

    def padded(self) -> torch.Tensor:
        return self.t.view(self.B, self.Hp, self.Wp, self.C)

    def batch(self, b0: int, n: int) -> "View":
        """Images b0 .. b0+n-1 as a view of the same storage."""
        assert 0 <= b0 and b0 + n <= self.B
        return View(self.t.view(self.B, -1)[b0:b0 + n].reshape(-1), n, self.H, self.W, self.C, self.halo, self.dtype)


@dataclass
class ConvCall:
    """Python mirror of gan_conv_desc (see include/mi355x_gan.h)."""
    B: int
    Ho: int
    Wo: int
    Cin: int
    ntaps: int
    Nw: int
    Nst: int
    x: View
    in_y0: int
    in_x0: int
    in_sy: int
    in_sx: int
    tapoff: torch.Tensor
    w: Optional[torch.Tensor]
    bias: Optional[torch.Tensor]
    out: View
    out_y0: int
    out_x0: int
    out_sy: int
    out_sx: int
    act: int = ACT_NONE
    mask: Optional[View] = None
    mask_y0: int = 0
    mask_x0: int = 0
    max_tapoff: int = 0
    w_frag: bool = False      # w is the fragment-major copy (range-patch kernel)
    tile_rows: int = 0        # range-patch kernel: pixels per tile, fixed at planning time (HipOps.conv_patch_tile_rows)
    tile_cols: int = 0        # ... and output channels per tile (HipOps.conv_patch_tile_cols, after tile_rows)
    stats: Optional[torch.Tensor] = None   # InstanceNorm partials written by the epilogue (see HipOps.conv_stats_parts)
    win7: Optional[tuple] = None           # (ty0, tx0): run by the 7x7 window kernel, taps row-major from that position (w_layout 2)
    w_scale: Optional[torch.Tensor] = None  # fp8 operands: device float, dequantisation scale of the weight copy
    in_scale: Optional[torch.Tensor] = None  # fp8 operands: device float[B], per-image scale of the input copy (None: 1)
    stats_mode: int = 0                    # 0: forward statistics; 1: backward chain, (sum t [m > 0], sum t m) with m = `mask` at the pixel (gan_conv_desc)
    flop_scale: float = 1.0                # algorithmic / launched FLOPs (paired phases multiply by zero blocks: 0.75); bench.py prices with it
    alg_pixels: Optional[int] = None       # output pixels per image of the REFERENCE op this launch implements, when they differ from Ho*Wo
                                           # (stride-1 input gradients run on the input's -- possibly reflect-padded -- domain); SURVEY §8d

    def alg_flops(self) -> float:
        """Algorithmic FLOPs (2*M*N*K with M the reference op's output pixels), what bench.py and tools/step_ops.py price."""
        px = self.Ho * self.Wo if self.alg_pixels is None else self.alg_pixels
        return 2.0 * self.B * px * self.Nst * self.Cin * self.ntaps * self.flop_scale


@dataclass
class WgradCall:
    """Python mirror of gan_wgrad_desc."""
    B: int
    Ho: int
    Wo: int
    Cx: int
    ntaps: int
    N: int
    nsplit: int
    x: View
    x_y0: int
    x_x0: int
    x_sy: int
    x_sx: int
    tapoff: torch.Tensor
    g: View
    g_y0: int
    g_x0: int
    g_sy: int
    g_sx: int
    part: Optional[torch.Tensor]
    max_tapoff: int = 0
    variant: int = 0          # 1: range-patch kernel (nsplit = B * splits per image); 2: 7x7 window kernel (nsplit = its block count)
    g_scale: Optional[torch.Tensor] = None   # e4m3 operands (x.dtype == FP8, variant 1): device float[B], per-image scale of g (None: 1)
    g_scale_pow2: Optional[bool] = None      # e4m3 operands: True promises that every g_scale[b] is a power of two (quantize_fp8_pow2); a
                                             # split may then cover several whole images (nsplit = B // -wgrad_patch_splits)


Op = Callable[[], None]



class Program:
    """A flat, replayable list of kernel launches."""

    def __init__(self, name: str = ""):
        self.name, self.ops = name, []  # type: str, List[Op]

    def add(self, op):
        if op is None:
            return
        if isinstance(op, (list, tuple)):
            for o in op:
                self.add(o)
        elif isinstance(op, Program):
            self.ops.extend(op.ops)
        else:
            self.ops.append(op)

    def run(self):
        for op in self.ops:
            op()

    def __len__(self):
        return len(self.ops)


class HipOps:
    """Op constructors bound to libmi355x_gan.so and one HIP stream.  `stream` is a raw hipStream_t handle (int)."""

    is_hip = True

    def __init__(self, device: torch.device, stream: Optional[int] = None, torch_stream=None):
        self.lib = _lib.load()
        self.device = device
        self.stream = stream  # None: torch's current stream at op-construction time (the module API builds graph slots that way); see bind()
        self.torch_stream = torch_stream   # the torch.cuda.Stream behind `stream` (needed for event record / wait)
        self._keep = []       # ctypes structs referenced by prebuilt calls
        self._side = None
        self._fork = None

    # ---- a second HIP stream: independent MFMA-bound launches (weight gradients) run there while the HBM-bound chain
    #      (InstanceNorm backward, reflection folds) continues on the main stream; ordering by events recorded in the programs
    def side(self) -> "HipOps":
        if os.environ.get("GAN_SINGLE_STREAM"):     # profiling aid: per-kernel durations without concurrent kernels stretching them
            return self
        if self._side is None:
            ts = torch.cuda.Stream(device=self.device)
            self._side = HipOps(self.device, stream=ts.cuda_stream, torch_stream=ts)
        return self._side

    def fork(self) -> "HipOps":
        """A new op layer on its own (non-blocking) HIP stream of the same device (GAN_SINGLE_STREAM: this one)."""
        if os.environ.get("GAN_SINGLE_STREAM"):
            return self
        if self._fork is None:
            ts = torch.cuda.Stream(device=self.device)
            self._fork = HipOps(self.device, stream=ts.cuda_stream, torch_stream=ts)
        return self._fork

    def bind_queues(self):
        """Creates this op layer's streams (discriminator stream, weight-gradient side stream) and runs one trivial kernel on each.
        HIP binds a stream to one of its few hardware queues at first use; doing that before anything else creates streams (RCCL does
        when the process group is set up) keeps the three compute streams on three different queues."""
        if os.environ.get("GAN_SINGLE_STREAM") or self.device.type != "cuda":
            return
        for h in (self, self.fork(), self.side()):
            with torch.cuda.stream(h._ts()):
                torch.zeros(64, device=self.device).add_(1.0)
        torch.cuda.synchronize(self.device)

    def bind(self):
        """Binds an op layer created without a stream to the stream that is current NOW, for good: launches (raw handle baked into the
        prebuilt calls) and the torch-side events, copies and collectives (_ts) of a trainer then always meet on one stream,
        whatever is current when its programs are built or replayed."""
        if self.stream is None and self.device.type == "cuda":
            self.torch_stream = torch.cuda.current_stream(self.device)
            self.stream = self.torch_stream.cuda_stream
        return self

    def _ts(self):
        return self.torch_stream if self.torch_stream is not None else torch.cuda.current_stream(self.device)

    def new_event(self):
        return torch.cuda.Event()

    def record(self, ev) -> Op:
        """ev marks everything queued so far on this op layer's stream."""
        return lambda: ev.record(self._ts())

    def wait(self, ev) -> Op:
        """Launches queued after this on this op layer's stream start after `ev`."""
        return lambda: self._ts().wait_event(ev)

    def _s(self):
        return C.c_void_p(self.stream if self.stream is not None else torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name: str, *args) -> Op:
        fn = getattr(self.lib, name)
        self._keep.append(args)
        lib = self.lib
        if os.environ.get("GAN_DEBUG_SYNC"):   # debugging aid: name every launch and wait for it, so a fault is attributable
            def dbg():
                print(f"[gan] {name}", file=sys.stderr, flush=True)
                rc = fn(*args)
                if rc != 0:
                    raise _lib.GanError(f"{name}: {lib.gan_last_error().decode()}")
                torch.cuda.synchronize()
            return dbg

        def op():
            rc = fn(*args)
            if rc != 0:
                raise _lib.GanError(f"{name}: {lib.gan_last_error().decode()}")
        op.__name__ = name
        return op

    # Prebuilt calls hold RAW device pointers: every tensor / view an op captures is pinned here so that it can never be
    # returned to the caching allocator while a program that uses it is alive.
    def _p(self, t: Optional[torch.Tensor]):
        if t is None:
            return C.c_void_p(0)
        self._keep.append(t)
        return C.c_void_p(t.data_ptr())

    def _v(self, v: Optional[View]):
        if v is None:
            return C.cast(None, _lib.PV)
        self._keep.append(v)
        return C.byref(v.struct())

    # ---- convolution family
    def _conv_desc(self, c: ConvCall) -> GanConvDesc:
        d = GanConvDesc()
        d.dtype, d.B, d.Ho, d.Wo, d.Cin, d.ntaps, d.Nw, d.Nst = c.x.dtype, c.B, c.Ho, c.Wo, c.Cin, c.ntaps, c.Nw, c.Nst
        d.in_, d.in_Hp, d.in_Wp, d.in_y0, d.in_x0, d.in_sy, d.in_sx = c.x.ptr(), c.x.Hp, c.x.Wp, c.in_y0, c.in_x0, c.in_sy, c.in_sx
        d.tapoff, d.w, d.bias = c.tapoff.data_ptr(), (c.w.data_ptr() if c.w is not None else None), (c.bias.data_ptr() if c.bias is not None else None)
        d.out, d.out_Hp, d.out_Wp, d.out_C = c.out.ptr(), c.out.Hp, c.out.Wp, c.out.C
        d.out_y0, d.out_x0, d.out_sy, d.out_sx, d.act = c.out_y0, c.out_x0, c.out_sy, c.out_sx, c.act
        if c.mask is not None:
            assert c.mask.C == c.out.C and c.mask.dtype == c.out.dtype
            d.mask, d.mask_Hp, d.mask_Wp, d.mask_y0, d.mask_x0 = c.mask.ptr(), c.mask.Hp, c.mask.Wp, c.mask_y0, c.mask_x0
        d.stats = c.stats.data_ptr() if c.stats is not None else None
        d.stats_mode = c.stats_mode
        d.max_tapoff = c.max_tapoff
        d.w_layout = 1 if c.w_frag else 0
        d.tile_rows, d.tile_cols = c.tile_rows, c.tile_cols
        d.w_scale = c.w_scale.data_ptr() if c.w_scale is not None else None
        d.in_scale = c.in_scale.data_ptr() if c.in_scale is not None else None
        if c.win7 is not None:
            assert not c.w_frag
            d.w_layout, d.win_ty0, d.win_tx0 = 2, c.win7[0], c.win7[1]
        assert c.out.dtype == (BF16 if c.x.dtype == FP8 else c.x.dtype)       # fp8 operands produce a bf16 result
        return d

    def conv_patch_ok(self, c: ConvCall) -> bool:
        """True if the range-patch kernel takes this call (then `c.w` must be the fragment-major weight copy)."""
        return bool(self.lib.gan_conv_patch_ok(C.byref(self._conv_desc(c))))

    def conv_patch_tile_rows(self, c: ConvCall) -> int:
        """Pixels per tile the range-patch kernel uses for this call (0: not eligible); planned once, carried in the descriptor."""
        return int(self.lib.gan_conv_patch_tile_rows(C.byref(self._conv_desc(c))))

    def conv_patch_tile_cols(self, c: ConvCall) -> int:
        """Output channels per tile (128 | 256) for the call's tile_rows; planned once, carried in the descriptor."""
        return int(self.lib.gan_conv_patch_tile_cols(C.byref(self._conv_desc(c))))

    def conv_patch_variant(self, c: ConvCall) -> dict:
        """The range-patch instantiation this call runs on ({} if it does not qualify): rows, cols, slices, fp8, static9, static_taps."""
        d = self._conv_desc(c)
        v = int(self.lib.gan_conv_patch_variant(C.byref(d))) if c.w_frag else 0
        return {} if v == 0 else {"rows": v & 0xfff, "cols": (v >> 12) & 0xfff, "slices": (v >> 24) & 0xf, "fp8": bool((v >> 28) & 1), "static9": bool((v >> 29) & 1),
                                      "static_taps": 9 if (v >> 29) & 1 else (0, 4, 2, 16)[(v >> 30) & 3]}

    def conv_igemm_variant(self, c: ConvCall) -> dict:
        """Tiling of the launch gan_conv_igemm makes for this planned call (generic, range-patch or 7x7 window kernel, by its weight
        layout): rows and cols per tile, tiles, and the blocks launched (grid)."""
        info = (C.c_int32 * 4)()
        _lib.check(self.lib.gan_conv_igemm_variant(C.byref(self._conv_desc(c)), info), "gan_conv_igemm_variant")
        return {"rows": info[0], "cols": info[1], "tiles": info[2], "grid": info[3]}

    def wgrad_reduce_lanes(self, nsplit: int, N_real: int, ntaps: int, Cx: int) -> int:
        """Lanes G that gan_wgrad_reduce lets share one output quad for these arguments."""
        return int(self.lib.gan_wgrad_reduce_lanes(nsplit, N_real, ntaps, Cx))

    def conv_win7_ok(self, c: ConvCall, ty0: int, tx0: int) -> bool:
        """True if the 7x7 window kernel takes this call with its 49 row-major taps starting at (ty0, tx0)."""
        d = self._conv_desc(c)
        d.win_ty0, d.win_tx0 = ty0, tx0
        return bool(self.lib.gan_conv_win7_ok(C.byref(d)))

    def conv_stats_parts(self, c: ConvCall) -> int:
        """Pixel tiles per image for which this call can write InstanceNorm partials in its epilogue (0: it cannot)."""
        return int(self.lib.gan_conv_stats_parts(C.byref(self._conv_desc(c))))

    def in_stats_from_parts(self, parts, nparts, B, Cc, HW, eps, stats) -> Op:
        return self._call("gan_in_stats_from_parts", self._p(parts), nparts, B, Cc, HW, C.c_float(eps), self._p(stats), self._s())

    def conv_igemm(self, c: ConvCall) -> Op:
        self._keep.append(c)
        op = self._call("gan_conv_igemm", C.byref(self._conv_desc(c)), self._s())
        op.conv = c   # lets bench.py enumerate a program's convolution launches and price them
        return op

    def _wgrad_desc(self, c: WgradCall) -> GanWgradDesc:
        d = GanWgradDesc()
        d.dtype, d.B, d.Ho, d.Wo, d.Cx, d.ntaps, d.N, d.nsplit = c.x.dtype, c.B, c.Ho, c.Wo, c.Cx, c.ntaps, c.N, c.nsplit
        d.x, d.x_Hp, d.x_Wp, d.x_y0, d.x_x0, d.x_sy, d.x_sx = c.x.ptr(), c.x.Hp, c.x.Wp, c.x_y0, c.x_x0, c.x_sy, c.x_sx
        d.tapoff, d.g = c.tapoff.data_ptr(), c.g.ptr()
        d.g_Hp, d.g_Wp, d.g_C, d.g_y0, d.g_x0, d.g_sy, d.g_sx = c.g.Hp, c.g.Wp, c.g.C, c.g_y0, c.g_x0, c.g_sy, c.g_sx
        d.part = c.part.data_ptr() if c.part is not None else None
        d.max_tapoff, d.variant = c.max_tapoff, c.variant
        d.g_scale = c.g_scale.data_ptr() if c.g_scale is not None else None
        d.g_scale_pow2 = 1 if c.g_scale_pow2 else 0
        assert c.g.dtype == c.x.dtype and (c.g_scale is None or (c.x.dtype == FP8 and c.g_scale.dtype == torch.float32 and c.g_scale.numel() >= c.B))
        return d

    def wgrad_patch_splits(self, c: WgradCall) -> int:
        """Splits per image the range-patch weight-gradient kernel wants for this call (0: not eligible)."""
        return int(self.lib.gan_wgrad_patch_splits(C.byref(self._wgrad_desc(c))))

    def wgrad_win7_splits(self, c: WgradCall) -> int:
        """Slabs the 7x7 window weight-gradient kernel writes for this call (0: not eligible); then variant 2, nsplit = this."""
        return int(self.lib.gan_wgrad_win7_splits(C.byref(self._wgrad_desc(c))))

    def conv_wgrad(self, c: WgradCall) -> Op:
        self._keep.append(c)
        assert c.part.numel() >= c.nsplit * c.N * c.ntaps * c.Cx
        op = self._call("gan_conv_wgrad", C.byref(self._wgrad_desc(c)), self._s())
        op.wgrad = c
        return op

    def wgrad_reduce(self, part, nsplit, N, ntaps, Cx, N_real, C_real, swap, I2, KK, khw, grad, accumulate) -> Op:
        return self._call("gan_wgrad_reduce", self._p(part), nsplit, N, ntaps, Cx, N_real, C_real, int(swap), I2, KK, self._p(khw),
                          self._p(grad), int(accumulate), self._s())

    def pack_weight(self, src, dst, dtype, Nw, ntaps, Cin, N_real, C_real, swap, I2, KK, khw, layout=0, scale=None) -> Op:
        """One operand copy.  dtype FP8 (e4m3, needs `scale`: a device float the batch launch fills with max|W| / 448) exists only in
        the batched form: the returned op then only carries its arguments for pack_weight_batch."""
        if dtype == FP8 or scale is not None:
            # fp8: scale = max|W| / 448, filled by the batch launch; bf16 / fp32: a device float the copy is divided by (spectral norm's
            # sigma).  Both exist only in the batched form.
            assert dtype != FP8 or layout == 1

            def op():
                raise _lib.GanError("scaled operand copies are packed by pack_weight_batch")
        else:
            op = self._call("gan_pack_weight", self._p(src), self._p(dst), dtype, Nw, ntaps, Cin, N_real, C_real, int(swap), I2, KK,
                            self._p(khw), int(layout), self._s())
        op.pack_args = (src, dst, dtype, Nw, ntaps, Cin, N_real, C_real, int(swap), I2, KK, khw, int(layout), scale)
        return op

    def pack_weight_batch(self, packs) -> Op:
        """One launch for many operand copies; `packs` = the pack_args tuples of ops built by pack_weight."""
        arr = (_lib.GanPackDesc * len(packs))()
        first = 0
        any_fp8 = False
        for d, (src, dst, dtype, Nw, ntaps, Cin, N_real, C_real, swap, I2, KK, khw, layout, *rest) in zip(arr, packs):
            assert layout == 0 or (Nw % 16 == 0 and (ntaps * Cin) % 32 == 0)
            scale = rest[0] if rest else None
            self._keep.extend((src, dst, khw, scale))
            d.src, d.dst, d.khw = src.data_ptr(), dst.data_ptr(), khw.data_ptr()
            d.scale = scale.data_ptr() if scale is not None else None
            any_fp8 = any_fp8 or dtype == FP8
            d.dtype, d.Nw, d.ntaps, d.Cin, d.N_real, d.C_real, d.swap, d.I2, d.KK, d.layout = dtype, Nw, ntaps, Cin, N_real, C_real, swap, I2, KK, layout
            d.nblocks = max(1, min(512, (Nw * ntaps * Cin + 1023) // 1024))
            d.first_block, first = first, first + d.nblocks
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        pack = self._call("gan_pack_weight_batch", self._p(table), len(packs), first, self._s())
        if not any_fp8:
            return pack
        scales = self._call("gan_weight_scale_batch", self._p(table), len(packs), self._s())   # per-tensor max|W| / 448 first

        def op():
            scales()
            pack()
        op.__name__ = "gan_pack_weight_batch"
        return op

    def bias_grad(self, g: View, N_real, grad, accumulate, ws) -> Op:
        return self._call("gan_bias_grad", self._v(g), N_real, self._p(grad), int(accumulate), self._p(ws), self._s())

    # ---- norm / activations / layout
    def in_stats(self, x: View, eps, stats, ws) -> Op:
        return self._call("gan_in_stats", self._v(x), C.c_float(eps), self._p(stats), self._p(ws), self._s())

    def in_finalize(self, stats, BC, HW, eps) -> Op:
        """stats: fp32 [BC][2] whole-image (sum, sum of squares), turned into (mean, rstd) in place."""
        assert stats.dtype == torch.float32 and stats.numel() >= BC * 2
        return self._call("gan_in_finalize", self._p(stats), BC, HW, C.c_float(eps), self._s())

    @staticmethod
    def _hbm(op: Op, x: View, ntensors: int) -> Op:
        """Algorithmic HBM bytes of an HBM-bound launch (every operand tensor read or written once), for bench.py."""
        op.hbm_bytes = ntensors * x.B * x.H * x.W * x.C * (4 if x.dtype == F32 else 2)
        return op

    def in_apply(self, x: View, stats, act, residual: Optional[View], y: View, halo_mode) -> Op:
        return self._hbm(self._call("gan_in_apply", self._v(x), self._p(stats), act, self._v(residual), self._v(y), halo_mode, self._s()),
                         x, 2 + (residual is not None))

    def in_partial_count(self, x: View) -> int:
        """Statistics partials per image gan_in_partial writes for x (<= 16: gan_in_apply_parts sums them itself)."""
        n = int(self.lib.gan_in_partial_count(self._v(x)))
        if n < 1:
            raise _lib.GanError(self.lib.gan_last_error().decode())
        return n

    def in_partial(self, x: View, parts) -> Op:
        assert parts.dtype == torch.float32 and parts.numel() >= x.B * self.in_partial_count(x) * x.C * 2
        return self._call("gan_in_partial", self._v(x), self._p(parts), self._s())

    def in_apply_parts(self, x: View, parts, nparts, eps, stats, act, residual: Optional[View], y: View, halo_mode, y8: Optional[View] = None) -> Op:
        """InstanceNorm apply with the statistics summed from `nparts` (<= 16) partial pairs per image inside the pass (no finalize launch).
        y8: an e4m3 view of y's geometry that receives a copy of y in the same pass (fp8 path)."""
        assert 1 <= nparts <= 16 and parts.numel() >= x.B * nparts * x.C * 2 and stats.numel() >= x.B * x.C * 2
        if y8 is not None:
            assert y8.dtype == FP8 and (y8.B, y8.Hp, y8.Wp, y8.C, y8.halo) == (y.B, y.Hp, y.Wp, y.C, y.halo)
            return self._hbm(self._call("gan_in_apply_parts_fp8", self._v(x), self._p(parts), nparts, C.c_float(eps), self._p(stats), act, self._v(residual),
                                        self._v(y), self._v(y8), halo_mode, self._s()), x, 2 + (residual is not None))
        return self._hbm(self._call("gan_in_apply_parts", self._v(x), self._p(parts), nparts, C.c_float(eps), self._p(stats), act, self._v(residual),
                                    self._v(y), halo_mode, self._s()), x, 2 + (residual is not None))

    def in_bwd(self, x: View, stats, act, gy: View, fold, g2: Optional[View], dx: View, ws) -> Op:
        return self._hbm(self._call("gan_in_bwd", self._v(x), self._p(stats), act, self._v(gy), int(fold), self._v(g2), self._v(dx), self._p(ws), self._s()),
                         x, 3 + (g2 is not None))

    def in_bwd_bias(self, x: View, stats, act, gy: View, fold, g2: Optional[View], dx: View, ws, bias_grad, bias_n, accumulate) -> Op:
        return self._hbm(self._call("gan_in_bwd_bias", self._v(x), self._p(stats), act, self._v(gy), int(fold), self._v(g2), self._v(dx), self._p(ws),
                                    self._p(bias_grad), bias_n, int(accumulate), self._s()), x, 3 + (g2 is not None))

    def in_bwd_bias_parts(self, x: View) -> int:
        n = int(self.lib.gan_in_bwd_bias_parts(self._v(x)))
        if n < 0:
            raise _lib.GanError(self.lib.gan_last_error().decode())
        return n

    def in_bwd_bias_deferred(self, x: View, stats, act, gy: View, fold, g2: Optional[View], dx: View, ws, bias_part) -> Op:
        assert bias_part.dtype == torch.float32 and bias_part.numel() >= self.in_bwd_bias_parts(x) * x.C
        return self._hbm(self._call("gan_in_bwd_bias_deferred", self._v(x), self._p(stats), act, self._v(gy), int(fold), self._v(g2), self._v(dx),
                                    self._p(ws), self._p(bias_part), self._s()), x, 3 + (g2 is not None))

    def in_bwd_parts(self, x: View, stats, act, gy: View, fold, dx: View, parts, nparts, parts_mode, bias_part=None) -> Op:
        """The apply half of the InstanceNorm backward alone: the per-(image, channel) sums come as `nparts` partial pairs from the
        input-gradient epilogue that wrote gy (ConvCall.stats_mode 1 | 2 = parts_mode)."""
        assert parts.dtype == torch.float32 and parts.numel() >= x.B * nparts * x.C * 2
        assert bias_part is None or bias_part.numel() >= self.in_bwd_bias_parts(x) * x.C
        return self._hbm(self._call("gan_in_bwd_parts", self._v(x), self._p(stats), act, self._v(gy), int(fold), self._v(dx), self._p(parts), nparts,
                                    parts_mode, self._p(bias_part), self._s()), x, 3)

    def bias_finalize_batch(self, items) -> Op:
        """items: (part, nparts, C, grad, N_real, accumulate) per layer -> one launch."""
        arr = (_lib.GanBiasPartDesc * len(items))()
        first = 0
        for d, (part, nparts, Cc, grad, n_real, acc) in zip(arr, items):
            self._keep.extend((part, grad))
            d.part, d.grad, d.nparts, d.C, d.N_real, d.accumulate = part.data_ptr(), grad.data_ptr(), nparts, Cc, n_real, int(acc)
            d.first_block, first = first, first + (Cc + 31) // 32
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        return self._call("gan_bias_finalize_batch", self._p(table), len(items), first, self._s())

    def in_bwd_amax(self, x: View, stats, act, gy: View, fold, dx: View, ws, bias_part, amax) -> Op:
        """InstanceNorm backward that also leaves max|dx| per image in `amax` (float[B]): the scale of dx's e4m3 copy."""
        assert amax.dtype == torch.float32 and amax.numel() >= x.B
        return self._hbm(self._call("gan_in_bwd_amax", self._v(x), self._p(stats), act, self._v(gy), int(fold), self._v(dx), self._p(ws),
                                    self._p(bias_part), self._p(amax), self._s()), x, 3)

    def quantize_fp8(self, src: View, dst: View, amax=None, scale_out=None) -> Op:
        """e4m3 copy of a whole buffer (halo included): unit scale, or per-image scale amax[b] / 448 written to scale_out[b]."""
        assert dst.dtype == FP8 and (src.B, src.Hp, src.Wp, src.C, src.halo) == (dst.B, dst.Hp, dst.Wp, dst.C, dst.halo)
        return self._call("gan_quantize_fp8", self._v(src), self._v(dst), self._p(amax), self._p(scale_out), self._s())

    def quantize_fp8_pow2(self, src: View, dst: View, amax, scale_out) -> Op:
        """quantize_fp8 with the per-image scale rounded up to a power of two, 2^ceil(log2(amax[b] / 448)): what WgradCall.g_scale_pow2
        promises (the scale's exponent byte is the MFMA's block scale)."""
        assert dst.dtype == FP8 and (src.B, src.Hp, src.Wp, src.C, src.halo) == (dst.B, dst.Hp, dst.Wp, dst.C, dst.halo)
        assert amax is not None and scale_out is not None and amax.numel() >= src.B and scale_out.numel() >= src.B
        return self._call("gan_quantize_fp8_pow2", self._v(src), self._v(dst), self._p(amax), self._p(scale_out), self._s())

    def fold_add(self, a: Optional[View], b: View, fold, out: View) -> Op:
        return self._call("gan_fold_add", self._v(a), self._v(b), int(fold), self._v(out), self._s())

    def pad_fold(self, g: View, mode, out: View) -> Op:
        """Gradient of a padding layer: out = sum of g (which carries the halo) over the padded positions copied from each pixel."""
        return self._call("gan_pad_fold", self._v(g), mode, self._v(out), self._s())

    def act_bwd(self, y: View, act, g: View, fold, g2: Optional[View], dx: View) -> Op:
        return self._call("gan_act_bwd", self._v(y), act, self._v(g), int(fold), self._v(g2), self._v(dx), self._s())

    def nchw_to_view(self, src: torch.Tensor, Cr, dst: View, halo_mode) -> Op:
        assert src.dtype == torch.float32 and src.is_contiguous()
        return self._call("gan_nchw_to_view", self._p(src), Cr, self._v(dst), halo_mode, self._s())

    def view_to_nchw(self, src: View, Cr, dst: torch.Tensor) -> Op:
        assert dst.dtype == torch.float32 and dst.is_contiguous()
        return self._call("gan_view_to_nchw", self._v(src), Cr, self._p(dst), self._s())

    def view_to_u8_hwc(self, src: View, Cr, dst: torch.Tensor) -> Op:
        """Interior of src -> packed (B, H, W, Cr) uint8: clamp(-1, 1) * 0.5 + 0.5, * 255, round half to even (inference.to_uint8)."""
        assert dst.dtype == torch.uint8 and dst.is_contiguous() and tuple(dst.shape) == (src.B, src.H, src.W, Cr)
        return self._call("gan_view_to_u8_hwc", self._v(src), Cr, self._p(dst), self._s())

    # ---- JPEG encoder (csrc/jpeg.hip; inference.JpegEncoder owns the buffers)
    def jpeg_bounds(self, B, H, W):
        """(workspace bytes, scan output bytes) for a batch of B images of H x W; refuses what the kernels refuse."""
        ws, out = C.c_int64(0), C.c_int64(0)
        _lib.check(self.lib.gan_jpeg_bounds(B, H, W, C.byref(ws), C.byref(out)), "gan_jpeg_bounds")
        return int(ws.value), int(out.value)

    def jpeg_blocks(self, rgb: torch.Tensor, quality, ws: torch.Tensor, hist: torch.Tensor) -> Op:
        """Packed uint8 (B, H, W, 3) -> quantised zig-zag coefficients in ws, symbol histograms (B, 4, 256) in hist."""
        B, H, W, _ = rgb.shape
        assert rgb.dtype == torch.uint8 and rgb.is_contiguous() and rgb.shape[3] == 3 and ws.dtype == torch.uint8
        assert hist.dtype == torch.int32 and hist.is_contiguous() and hist.numel() >= B * 1024
        return self._call("gan_jpeg_blocks", self._p(rgb), B, H, W, int(quality), self._p(ws), ws.numel(), self._p(hist), self._s())

    def jpeg_tables(self, hist: torch.Tensor, n, dht: torch.Tensor, codes: torch.Tensor) -> Op:
        """n histograms of 256 counts -> optimal tables: dht (n, 272) uint8 = 16 counts + symbols, codes (n, 256) int32 = length << 16 | code."""
        assert hist.dtype == torch.int32 and dht.dtype == torch.uint8 and codes.dtype == torch.int32
        assert hist.is_contiguous() and dht.is_contiguous() and codes.is_contiguous()
        assert hist.numel() >= n * 256 and dht.numel() >= n * 272 and codes.numel() >= n * 256
        return self._call("gan_jpeg_tables", self._p(hist), int(n), self._p(dht), self._p(codes), self._s())

    def jpeg_scan(self, ws: torch.Tensor, B, H, W, codes: torch.Tensor, out: torch.Tensor, offsets: torch.Tensor) -> Op:
        """The stuffed, padded scans of the B images of ws back to back in out; offsets (B + 1) int64: image b is out[offsets[b]:offsets[b + 1]]."""
        assert ws.dtype == torch.uint8 and out.dtype == torch.uint8 and codes.dtype == torch.int32 and offsets.dtype == torch.int64
        assert codes.numel() >= B * 1024 and offsets.numel() >= B + 1 and out.is_contiguous() and offsets.is_contiguous()
        return self._call("gan_jpeg_scan", self._p(ws), ws.numel(), B, H, W, self._p(codes), self._p(out), out.numel(), self._p(offsets), self._s())

    # ---- whole files and their CRC-32 for stored ZIP entries (csrc/zip.hip; inference.JpegEncoder owns the buffers)
    def crc32_ranges(self, buf: torch.Tensor, offsets: torch.Tensor, crc: torch.Tensor, flag: torch.Tensor) -> Op:
        """zlib's CRC-32 of buf[offsets[i]:offsets[i + 1]] for the n = len(offsets) - 1 ranges, into crc (n) int32; an inconsistent pair
        gives 0 and ORs 1 into flag (1) int32, which the caller zeroes."""
        n = offsets.numel() - 1
        assert buf.dtype == torch.uint8 and offsets.dtype == torch.int64 and crc.dtype == torch.int32 and flag.dtype == torch.int32
        assert buf.is_contiguous() and offsets.is_contiguous() and crc.is_contiguous() and n >= 0 and crc.numel() >= n and flag.numel() >= 1
        return self._call("gan_crc32_ranges", self._p(buf), buf.numel(), self._p(offsets), n, self._p(crc), self._p(flag), self._s())

    def jpeg_files_bounds(self, B, H, W, head_bytes, sos_bytes=14):
        """Bytes that B complete files of H x W can need: jpeg_bounds' scan bytes plus head, four full DHT segments, SOS and EOI each."""
        out = C.c_int64(0)
        _lib.check(self.lib.gan_jpeg_files_bounds(B, H, W, int(head_bytes), int(sos_bytes), C.byref(out)), "gan_jpeg_files_bounds")
        return int(out.value)

    def jpeg_files(self, head: torch.Tensor, sos: torch.Tensor, dht: torch.Tensor, scan: torch.Tensor, scan_offsets: torch.Tensor, B,
                   files: torch.Tensor, file_offsets: torch.Tensor, crc: torch.Tensor, flag: torch.Tensor) -> Op:
        """Complete JPEG files back to back in files: head, the four DHT segments of dht (B, 4, 272), sos, the image's bytes of scan, EOI.
        file_offsets (B + 1) int64, crc (B) int32 = CRC-32 of every file, flag (1) int32: bit 0 inconsistent scan_offsets, bit 1 files too small."""
        assert all(t.dtype == torch.uint8 and t.is_contiguous() for t in (head, sos, dht, scan, files))
        assert scan_offsets.dtype == torch.int64 and file_offsets.dtype == torch.int64 and crc.dtype == torch.int32 and flag.dtype == torch.int32
        assert dht.numel() >= B * 4 * 272 and scan_offsets.numel() >= B + 1 and file_offsets.numel() >= B + 1 and crc.numel() >= B and flag.numel() >= 1
        assert scan_offsets.is_contiguous() and file_offsets.is_contiguous() and crc.is_contiguous()
        return self._call("gan_jpeg_files", self._p(head), head.numel(), self._p(sos), sos.numel(), self._p(dht), self._p(scan), scan.numel(),
                          self._p(scan_offsets), int(B), self._p(files), files.numel(), self._p(file_offsets), self._p(crc), self._p(flag), self._s())

    # ---- JPEG decoder (csrc/jpegdec.hip; dataio.JpegDecoder owns the buffers).  A decode's descriptors are new with every call, so these
    #      entries launch at once instead of returning a prebuilt Op.
    def _now(self, name: str, *args):
        rc = getattr(self.lib, name)(*args)
        if rc != 0:
            raise _lib.GanError(f"{name}: {self.lib.gan_last_error().decode()}")

    def jpegdec_block_offsets(self, n, nseg):
        """Byte offsets (segments, dht, qt, scan bytes) of the upload block of n images and nseg restart segments."""
        off = (C.c_int64 * 4)()
        self._now("gan_jpegdec_block_offsets", int(n), int(nseg), off)
        return tuple(int(v) for v in off)

    def jpegdec_bounds(self, imgs) -> int:
        """imgs: a ctypes array of _lib.GanJpegdecImage; fills their coef_off / plane_off and returns the workspace bytes."""
        ws = C.c_int64(0)
        self._now("gan_jpegdec_bounds", C.cast(imgs, C.c_void_p), len(imgs), C.byref(ws))
        return int(ws.value)

    def _jpegdec_args(self, blk_dev, blk_host, nbytes, n, nseg, ws):
        assert blk_dev.dtype == torch.uint8 and blk_host.dtype == torch.uint8 and ws.dtype == torch.uint8 and blk_host.device.type == "cpu"
        assert blk_dev.is_contiguous() and blk_host.is_contiguous() and ws.is_contiguous() and nbytes <= min(blk_dev.numel(), blk_host.numel())
        return (C.c_void_p(blk_dev.data_ptr()), C.c_void_p(blk_host.data_ptr()), int(nbytes), int(n), int(nseg), C.c_void_p(ws.data_ptr()), ws.numel())

    def jpegdec_tables(self, blk_dev, blk_host, nbytes, n, nseg, ws):
        """DHT tables of the block -> decode tables in ws; zeroes the error words and the coefficients."""
        self._now("gan_jpegdec_tables", *self._jpegdec_args(blk_dev, blk_host, nbytes, n, nseg, ws), self._s())

    def jpegdec_entropy(self, blk_dev, blk_host, nbytes, n, nseg, ws):
        """The scans -> int16 coefficients in ws, one workgroup per image, one lane per restart segment."""
        self._now("gan_jpegdec_entropy", *self._jpegdec_args(blk_dev, blk_host, nbytes, n, nseg, ws), self._s())

    def jpegdec_idct(self, blk_dev, blk_host, nbytes, n, nseg, ws):
        """Coefficients -> uint8 component planes in ws."""
        self._now("gan_jpegdec_idct", *self._jpegdec_args(blk_dev, blk_host, nbytes, n, nseg, ws), self._s())

    def jpegdec_pixels(self, blk_dev, blk_host, nbytes, n, nseg, ws, out, err):
        """Planes -> packed (H, W, 3) at every image's out_off in `out`; err (int32 [n]) receives the error words."""
        assert out.dtype == torch.uint8 and out.is_contiguous() and err.dtype == torch.int32 and err.is_contiguous() and err.numel() >= n
        self._now("gan_jpegdec_pixels", *self._jpegdec_args(blk_dev, blk_host, nbytes, n, nseg, ws), C.c_void_p(out.data_ptr()), out.numel(),
                  C.c_void_p(err.data_ptr()), self._s())

    # ---- progressive JPEG decoder (csrc/jpegprog.hip).  counts = (images, scans, segments, table versions) of the block.
    def jpegprog_block_offsets(self, n, nscan, nseg, nver):
        """Byte offsets (progressive image descriptors, scans, segments, dht, qt, scan bytes) of the upload block."""
        off = (C.c_int64 * 6)()
        self._now("gan_jpegprog_block_offsets", int(n), int(nscan), int(nseg), int(nver), off)
        return tuple(int(v) for v in off)

    def jpegprog_bounds(self, imgs, nver) -> int:
        """imgs: a ctypes array of _lib.GanJpegdecImage; fills their coef_off / plane_off and returns the workspace bytes."""
        ws = C.c_int64(0)
        self._now("gan_jpegprog_bounds", C.cast(imgs, C.c_void_p), len(imgs), int(nver), C.byref(ws))
        return int(ws.value)

    def _jpegprog_args(self, blk_dev, blk_host, nbytes, counts, ws):
        a = self._jpegdec_args(blk_dev, blk_host, nbytes, counts[0], counts[2], ws)
        return a[:3] + tuple(int(v) for v in counts) + a[5:]

    def jpegprog_tables(self, blk_dev, blk_host, nbytes, counts, ws):
        """DHT versions of the block -> decode tables in ws; zeroes the error words and the coefficients."""
        self._now("gan_jpegprog_tables", *self._jpegprog_args(blk_dev, blk_host, nbytes, counts, ws), self._s())

    def jpegprog_entropy(self, blk_dev, blk_host, nbytes, counts, ws):
        """The scans -> int16 coefficients in ws: one workgroup per image, one lane per (scan, restart segment), level after level."""
        self._now("gan_jpegprog_entropy", *self._jpegprog_args(blk_dev, blk_host, nbytes, counts, ws), self._s())

    def jpegprog_idct(self, blk_dev, blk_host, nbytes, counts, ws):
        self._now("gan_jpegprog_idct", *self._jpegprog_args(blk_dev, blk_host, nbytes, counts, ws), self._s())

    def jpegprog_pixels(self, blk_dev, blk_host, nbytes, counts, ws, out, err):
        assert out.dtype == torch.uint8 and out.is_contiguous() and err.dtype == torch.int32 and err.is_contiguous() and err.numel() >= counts[0]
        self._now("gan_jpegprog_pixels", *self._jpegprog_args(blk_dev, blk_host, nbytes, counts, ws), C.c_void_p(out.data_ptr()), out.numel(),
                  C.c_void_p(err.data_ptr()), self._s())

    # ---- PNG decoder (csrc/pngdec.hip; dataio.PngDecoder owns the buffers); launched at once, like the JPEG decoder's entries
    def pngdec_block_offsets(self, n):
        """Byte offsets (palettes, first stream) of the upload block of n files."""
        off = (C.c_int64 * 2)()
        self._now("gan_pngdec_block_offsets", int(n), off)
        return tuple(int(v) for v in off)

    def pngdec_bounds(self, imgs) -> int:
        """imgs: a ctypes array of _lib.GanPngdecImage; fills their raw_off and returns the workspace bytes."""
        ws = C.c_int64(0)
        self._now("gan_pngdec_bounds", C.cast(imgs, C.c_void_p), len(imgs), C.byref(ws))
        return int(ws.value)

    def _pngdec_args(self, blk_dev, blk_host, nbytes, n, ws):
        assert blk_dev.dtype == torch.uint8 and blk_host.dtype == torch.uint8 and ws.dtype == torch.uint8 and blk_host.device.type == "cpu"
        assert blk_dev.is_contiguous() and blk_host.is_contiguous() and ws.is_contiguous() and nbytes <= min(blk_dev.numel(), blk_host.numel())
        return (C.c_void_p(blk_dev.data_ptr()), C.c_void_p(blk_host.data_ptr()), int(nbytes), int(n), C.c_void_p(ws.data_ptr()), ws.numel())

    def pngdec_inflate(self, blk_dev, blk_host, nbytes, n, ws):
        """The zlib streams -> the filtered scanlines in ws, one workgroup per file; overwrites the error words."""
        self._now("gan_pngdec_inflate", *self._pngdec_args(blk_dev, blk_host, nbytes, n, ws), self._s())

    def pngdec_pixels(self, blk_dev, blk_host, nbytes, n, ws, out, err):
        """Scanlines -> packed (H, W, 3) at every file's out_off in `out`; err (int32 [n]) receives the error words."""
        assert out.dtype == torch.uint8 and out.is_contiguous() and err.dtype == torch.int32 and err.is_contiguous() and err.numel() >= n
        self._now("gan_pngdec_pixels", *self._pngdec_args(blk_dev, blk_host, nbytes, n, ws), C.c_void_p(out.data_ptr()), out.numel(),
                  C.c_void_p(err.data_ptr()), self._s())

    # ---- evaluation (csrc/mifid.hip; evaluate.py is the caller).  Feature matrices are 2-D float32 / float64 tensors whose rows may be
    #      strided (stride(1) == 1); results are float64 tensors on the same device.  Launched at once, like the decoders' entries.
    @staticmethod
    def _feat(x: torch.Tensor):
        assert x.dim() == 2 and x.dtype in (torch.float32, torch.float64) and (x.shape[1] == 1 or x.stride(1) == 1), "feature matrix: 2-D fp32/fp64, unit column stride"
        ld = x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1])
        return C.c_void_p(x.data_ptr()), (_lib.FEAT_F64 if x.dtype == torch.float64 else _lib.FEAT_F32), int(ld)

    @staticmethod
    def _f64(t: Optional[torch.Tensor], n: int):
        if t is None:
            return C.c_void_p(0)
        assert t.dtype == torch.float64 and t.is_contiguous() and t.numel() == n
        return C.c_void_p(t.data_ptr())

    def feat_moments(self, x: torch.Tensor, out: Optional[dict] = None) -> dict:
        """x (n, D) -> mean [D], colcss [D] (centred sums of squares per column, second pass), norm [n], rowsum [n], css [1], flag (int32 [1],
        non-zero when x holds a NaN or an Inf).  out: the same keys as contiguous buffers of at least those sizes; their heads are written
        and returned, nothing behind them."""
        p, dt, ld = self._feat(x)
        n, D = x.shape
        sizes = {"mean": D, "colcss": D, "norm": n, "rowsum": n, "css": 1, "flag": 1}
        if out is None:
            out = {k: torch.empty(v, dtype=torch.int32 if k == "flag" else torch.float64, device=x.device) for k, v in sizes.items()}
        for k, v in sizes.items():
            t = out[k]
            assert t.dtype == (torch.int32 if k == "flag" else torch.float64) and t.is_contiguous() and t.numel() >= v and t.device == x.device, k
        self._now("gan_feat_moments", p, dt, n, D, ld, *(C.c_void_p(out[k].data_ptr()) for k in ("mean", "colcss", "norm", "rowsum", "css", "flag")), self._s())
        return {k: out[k].reshape(-1)[:v] for k, v in sizes.items()}

    def _gram_args(self, a, b, trans, ca, cb, ra, rb):
        (pa, da, lda), (pb, db, ldb) = self._feat(a), self._feat(b)
        M, N, K = (a.shape[1], b.shape[1], a.shape[0]) if trans else (a.shape[0], b.shape[0], a.shape[1])
        assert (b.shape[0] if trans else b.shape[1]) == K, "gram: contraction lengths differ"
        cen = (M, N) if trans else (K, K)
        return (pa, da, lda, pb, db, ldb), (M, N, K), (self._f64(ca, cen[0]), self._f64(cb, cen[1]), self._f64(ra, M), self._f64(rb, N))

    def gram_f64(self, a, b, trans=0, ca=None, cb=None, ra=None, rb=None, alpha=1.0, out=None) -> torch.Tensor:
        """trans = 0: out[i][j] = alpha ra[i] rb[j] sum_k (a[i][k] - ca[k]) (b[j][k] - cb[k]); trans = 1: out[p][q] = alpha sum_i (a[i][p] - ca[p])
        (b[i][q] - cb[q]).  out: float64 (M, N), rows may be strided."""
        ops, (M, N, K), cs = self._gram_args(a, b, int(trans), ca, cb, ra, rb)
        if out is None:
            out = torch.empty(M, N, dtype=torch.float64, device=a.device)
        assert out.dtype == torch.float64 and tuple(out.shape) == (M, N) and (N == 1 or out.stride(1) == 1)
        ldc = out.stride(0) if M > 1 else max(out.stride(0), N)
        self._now("gan_gram_f64", *ops[:6], int(trans), M, N, K, *cs, C.c_double(alpha), C.c_void_p(out.data_ptr()), int(ldc), self._s())
        return out

    def cos_rowmin_bounds(self, M, N) -> int:
        ws = C.c_int64(0)
        self._now("gan_cos_rowmin_bounds", int(M), int(N), C.byref(ws))
        return int(ws.value)

    def cos_rowmin(self, a, b, ca=None, cb=None, ra=None, rb=None, alpha=1.0, absolute=False, ws=None, dmin=None, imin=None):
        """Per row i of a: (min_j d_ij, lowest such j), d = 1 - s or 1 - |s|, s the trans = 0 product of gram_f64; rows / columns of scale 0
        are left out (+inf, -1 for a row with nothing to compare against).  ws: uint8 workspace of cos_rowmin_bounds bytes."""
        ops, (M, N, K), cs = self._gram_args(a, b, 0, ca, cb, ra, rb)
        if ws is None:
            ws = torch.empty(self.cos_rowmin_bounds(M, N), dtype=torch.uint8, device=a.device)
        if dmin is None:
            dmin = torch.empty(M, dtype=torch.float64, device=a.device)
        if imin is None:
            imin = torch.empty(M, dtype=torch.int32, device=a.device)
        assert ws.dtype == torch.uint8 and ws.is_contiguous() and dmin.dtype == torch.float64 and imin.dtype == torch.int32
        assert dmin.numel() >= M and imin.numel() >= M and dmin.is_contiguous() and imin.is_contiguous()
        self._now("gan_cos_rowmin", *ops, M, N, K, *cs, C.c_double(alpha), int(bool(absolute)), C.c_void_p(ws.data_ptr()), ws.numel(),
                  C.c_void_p(dmin.data_ptr()), C.c_void_p(imin.data_ptr()), self._s())
        return dmin, imin

    # ---- selection (csrc/mifid.hip; select_7k.py is the caller).  Column transform: x' = (x - c[k]) * s[k], c and s float64 [K] or None.
    def sqdist_rowmin_bounds(self, M, N) -> int:
        ws = C.c_int64(0)
        self._now("gan_sqdist_rowmin_bounds", int(M), int(N), C.byref(ws))
        return int(ws.value)

    def sqdist_rowmin(self, a, b, ca=None, sa=None, cb=None, sb=None, ws=None, dmin=None, imin=None):
        """Per row i of a: (min_j d_ij, lowest such j), d_ij = max(0, |a'_i|^2 + |b'_j|^2 - 2 a'_i . b'_j) over the transformed rows.
        ws: uint8 workspace of sqdist_rowmin_bounds bytes."""
        (pa, da, lda), (pb, db, ldb) = self._feat(a), self._feat(b)
        M, N, K = a.shape[0], b.shape[0], a.shape[1]
        assert b.shape[1] == K, "sqdist_rowmin: row lengths differ"
        if ws is None:
            ws = torch.empty(self.sqdist_rowmin_bounds(M, N), dtype=torch.uint8, device=a.device)
        if dmin is None:
            dmin = torch.empty(M, dtype=torch.float64, device=a.device)
        if imin is None:
            imin = torch.empty(M, dtype=torch.int32, device=a.device)
        assert ws.dtype == torch.uint8 and ws.is_contiguous() and dmin.dtype == torch.float64 and imin.dtype == torch.int32
        assert dmin.numel() >= M and imin.numel() >= M and dmin.is_contiguous() and imin.is_contiguous()
        self._now("gan_sqdist_rowmin", pa, da, lda, pb, db, ldb, M, N, K, self._f64(ca, K), self._f64(sa, K), self._f64(cb, K), self._f64(sb, K),
                  C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(dmin.data_ptr()), C.c_void_p(imin.data_ptr()), self._s())
        return dmin, imin

    def kmeans_update(self, x, labels, k, c=None, s=None, sums=None, counts=None, err=None):
        """sums (k, D) float64 (rows may be strided): per cluster the sum of the transformed rows in ascending row order; counts int32 [k];
        err int32 [1], non-zero when a label lies outside [0, k) (those rows are skipped)."""
        p, dt, ld = self._feat(x)
        n, D = x.shape
        k = int(k)
        assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == n and labels.device == x.device
        if sums is None:
            sums = torch.empty(k, D, dtype=torch.float64, device=x.device)
        if counts is None:
            counts = torch.empty(k, dtype=torch.int32, device=x.device)
        if err is None:
            err = torch.empty(1, dtype=torch.int32, device=x.device)
        assert sums.dtype == torch.float64 and tuple(sums.shape) == (k, D) and (D == 1 or sums.stride(1) == 1)
        assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= k and err.dtype == torch.int32 and err.numel() >= 1
        lds = sums.stride(0) if k > 1 else max(sums.stride(0), D)
        self._now("gan_kmeans_update", p, dt, n, D, ld, self._f64(c, D), self._f64(s, D), C.c_void_p(labels.data_ptr()), k,
                  C.c_void_p(sums.data_ptr()), int(lds), C.c_void_p(counts.data_ptr()), C.c_void_p(err.data_ptr()), self._s())
        return sums, counts, err

    def view_copy(self, src: View, dst: View, halo_mode) -> Op:
        return self._call("gan_view_copy", self._v(src), self._v(dst), halo_mode, self._s())

    def spectral_norm_ws_floats(self, h, w) -> int:
        return int(_lib.load().gan_spectral_norm_ws_floats(h, w))

    def spectral_norm_fwd(self, W, u, v, power_iter: bool, eps, sigma, Wsn, ws) -> Op:
        h, w = W.shape[0], W.numel() // W.shape[0]
        for t in (W, u, v, sigma, Wsn, ws):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert u.numel() == h and v.numel() == w and Wsn.numel() == W.numel() and ws.numel() >= self.spectral_norm_ws_floats(h, w)
        return self._call("gan_spectral_norm_fwd", self._p(W), h, w, self._p(u), self._p(v), int(power_iter), float(eps), self._p(sigma),
                          self._p(Wsn), self._p(ws), self._s())

    def spectral_norm_bwd(self, G, Wsn, u, v, sigma, dW, ws) -> Op:
        h, w = G.shape[0], G.numel() // G.shape[0]
        for t in (G, Wsn, u, v, sigma, dW, ws):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert u.numel() == h and v.numel() == w and dW.numel() == G.numel() and ws.numel() >= self.spectral_norm_ws_floats(h, w)
        return self._call("gan_spectral_norm_bwd", self._p(G), self._p(Wsn), self._p(u), self._p(v), self._p(sigma), h, w, self._p(dW),
                          self._p(ws), self._s())

    def spectral_norm_batch_ws_floats(self, h, w) -> int:
        return int(_lib.load().gan_spectral_norm_batch_ws_floats(h, w))

    _SN_FIELDS = ("W", "u", "v", "sigma", "u_snap", "v_snap", "G", "dW", "ws")

    def _sn_table(self, entries: Sequence[dict]):
        """entries: dicts of fp32 contiguous tensors W (weight_orig, any shape with h = shape[0]), u [h], v [w], sigma [1], u_snap [h],
        v_snap [w], ws (>= spectral_norm_batch_ws_floats) and, for the backward, G and dW (W's size).  -> (device table, total blocks)."""
        arr = (_lib.GanSnDesc * len(entries))()
        first = 0
        for d, e in zip(arr, entries):
            W = e["W"]
            h, w = W.shape[0], W.numel() // W.shape[0]
            for k in self._SN_FIELDS:
                t = e.get(k)
                assert t is not None or k in ("G", "dW"), k
                if t is not None:
                    assert t.dtype == torch.float32 and t.is_contiguous() and t.device == W.device, k
                    setattr(d, k, t.data_ptr())
            assert e["u"].numel() == h == e["u_snap"].numel() and e["v"].numel() == w == e["v_snap"].numel() and e["sigma"].numel() >= 1
            assert e["ws"].numel() >= self.spectral_norm_batch_ws_floats(h, w)
            assert all(e.get(k) is None or e[k].numel() == W.numel() for k in ("G", "dW"))
            d.h, d.w = h, w
            d.nblocks = int(_lib.load().gan_spectral_norm_batch_blocks(h, w))
            d.first_block, first = first, first + d.nblocks
        self._keep.append(list(entries))
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device), first

    def spectral_norm_batch_fwd(self, entries: Sequence[dict], power_iter: bool, eps: float) -> Op:
        """One gan_spectral_norm_batch_fwd over every entry (see _sn_table): power iteration (u, v in place), sigma, snapshots."""
        table, total = self._sn_table(entries)
        return self._call("gan_spectral_norm_batch_fwd", self._p(table), len(entries), total, int(power_iter), C.c_float(eps), self._s())

    def spectral_norm_batch_bwd(self, entries: Sequence[dict], accumulate: bool) -> Op:
        """dW (+)= (G - (<G, W> / sigma) u_snap v_snap^T) / sigma for every entry, one gan_spectral_norm_batch_bwd."""
        assert all(e.get("G") is not None and e.get("dW") is not None for e in entries)
        table, total = self._sn_table(entries)
        return self._call("gan_spectral_norm_batch_bwd", self._p(table), len(entries), total, int(accumulate), self._s())

    def avgpool_fwd(self, x: View, y: View) -> Op:
        return self._call("gan_avgpool_fwd", self._v(x), self._v(y), self._s())

    def avgpool_bwd(self, gy: View, gx: View, accumulate: bool) -> Op:
        return self._call("gan_avgpool_bwd", self._v(gy), self._v(gx), int(accumulate), self._s())

    # ---- augmentation and losses
    def diffaug_fwd(self, x: View, Cr, prm, y: View, ws) -> Op:
        return self._call("gan_diffaug_fwd", self._v(x), Cr, self._p(prm), self._v(y), self._p(ws), self._s())

    def diffaug_bwd(self, gy: View, Cr, prm, gx: View, ws) -> Op:
        return self._call("gan_diffaug_bwd", self._v(gy), Cr, self._p(prm), self._v(gx), self._p(ws), self._s())

    def patch_loss(self, logits: View, mode, target, scale, loss, grad: Optional[View]) -> Op:
        return self._call("gan_patch_loss", self._v(logits), mode, C.c_float(target), C.c_float(scale), self._p(loss), self._v(grad), self._s())

    def l1_loss(self, x: View, Cr, target_nchw, scale, dev_scale, loss, grad: Optional[View], ws) -> Op:
        return self._call("gan_l1_loss", self._v(x), Cr, self._p(target_nchw), C.c_float(scale), self._p(dev_scale), self._p(loss),
                          self._v(grad), self._p(ws), self._s())

    def r1_reduce(self, g: View, Cr, scale, loss, u: Optional[View], ws) -> Op:
        return self._call("gan_r1_reduce", self._v(g), Cr, C.c_float(scale), self._p(loss), self._v(u), self._p(ws), self._s())

    # ---- palette prior (csrc/palette.hip): cells [B][T*T][3], stats / gstats [B][3][2], batch / prior [3][2] fp32, steps int32 [1]
    def palette_stats(self, x: View, T, cells, stats) -> Op:
        check_palette_size(T)
        assert cells.numel() >= x.B * T * T * 3 and stats.numel() >= x.B * 6
        return self._call("gan_palette_stats", self._v(x), int(T), self._p(cells), self._p(stats), self._s())

    def palette_batch_mean(self, stats, B, batch) -> Op:
        assert stats.numel() >= B * 6 and batch.numel() >= 6
        return self._call("gan_palette_batch_mean", self._p(stats), int(B), self._p(batch), self._s())

    def palette_prior_update(self, batch, batch_scale, prior, steps, use_ema, decay) -> Op:
        assert steps.dtype == torch.int32 and prior.numel() >= 6 and batch.numel() >= 6
        return self._call("gan_palette_prior_update", self._p(batch), C.c_float(batch_scale), self._p(prior), self._p(steps), int(bool(use_ema)),
                          C.c_float(decay), self._s())

    def palette_loss(self, stats, prior, B, scale, loss, gstats) -> Op:
        assert stats.numel() >= B * 6 and (gstats is None or gstats.numel() >= B * 6)
        return self._call("gan_palette_loss", self._p(stats), self._p(prior), int(B), C.c_float(scale), self._p(loss), self._p(gstats), self._s())

    def palette_bwd(self, x: View, T, cells, stats, gstats, scale, gx: View, accumulate) -> Op:
        check_palette_size(T)
        return self._call("gan_palette_bwd", self._v(x), int(T), self._p(cells), self._p(stats), self._p(gstats), C.c_float(scale), self._v(gx),
                          int(bool(accumulate)), self._s())

    # ---- feature matching (csrc/featmatch.hip): *loss += loss_scale * mean |f - r| over C real channels; g (accumulate: +=) its gradient
    #      wrt f times grad_scale / loss_scale, through act' (f is a LeakyReLU output when g is the gradient in front of that LeakyReLU)
    def featmatch_ws_floats(self, f: View) -> int:
        return int(self.lib.gan_featmatch_ws_floats(self._v(f)))

    def featmatch(self, f: View, r: View, Cr, loss_scale, loss, grad_scale, act, g: Optional[View], accumulate, ws) -> Op:
        assert ws.dtype == torch.float32 and ws.numel() >= self.featmatch_ws_floats(f) and loss.dtype == torch.float32
        return self._call("gan_featmatch", self._v(f), self._v(r), int(Cr), C.c_float(loss_scale), self._p(loss), C.c_float(grad_scale), int(act),
                          self._v(g), int(bool(accumulate)), self._p(ws), self._s())

    def patchnce_ws_floats(self, B, P, Cc) -> int:
        return int(self.lib.gan_patchnce_ws_floats(B, P, Cc))

    def patchnce_fwd(self, src: View, tgt: View, ids, P, Cc, temperature, weight, loss, ws) -> Op:
        return self._call("gan_patchnce_fwd", self._v(src), self._v(tgt), self._p(ids), P, Cc, C.c_float(temperature), C.c_float(weight),
                          self._p(loss), self._p(ws), self._s())

    def patchnce_bwd(self, tgt: View, ids, P, Cc, temperature, weight, gtgt: View, ws) -> Op:
        return self._call("gan_patchnce_bwd", self._v(tgt), self._p(ids), P, Cc, C.c_float(temperature), C.c_float(weight), self._v(gtgt),
                          self._p(ws), self._s())

    # ---- PatchNCE with negatives from the whole minibatch (include/mi355x_gan.h): keys = fp32 tensor of `segs` segments of B*P rows of Cc
    #      floats, `seg_stride` floats apart; single rank: keys = ws (its own Sn), 1, 0, 0
    def patchnce_all_ws_floats(self, B, P, Cc) -> int:
        return int(self.lib.gan_patchnce_all_ws_floats(B, P, Cc))

    def patchnce_all_gather(self, src: View, tgt: View, ids, P, Cc, ws) -> Op:
        return self._call("gan_patchnce_all_gather", self._v(src), self._v(tgt), self._p(ids), P, Cc, self._p(ws), self._s())

    def patchnce_all_fwd(self, tgt: View, P, Cc, temperature, weight, keys, segs, seg_stride, self_seg, loss, ws) -> Op:
        assert keys.dtype == torch.float32 and keys.numel() >= (segs - 1) * seg_stride + tgt.B * P * Cc
        return self._call("gan_patchnce_all_fwd", self._v(tgt), P, Cc, C.c_float(temperature), C.c_float(weight), self._p(keys), int(segs),
                          C.c_int64(seg_stride), int(self_seg), self._p(loss), self._p(ws), self._s())

    def patchnce_all_bwd(self, tgt: View, ids, P, Cc, temperature, weight, keys, segs, seg_stride, self_seg, gtgt: View, ws) -> Op:
        assert keys.dtype == torch.float32 and keys.numel() >= (segs - 1) * seg_stride + tgt.B * P * Cc
        return self._call("gan_patchnce_all_bwd", self._v(tgt), self._p(ids), P, Cc, C.c_float(temperature), C.c_float(weight), self._p(keys),
                          int(segs), C.c_int64(seg_stride), int(self_seg), self._v(gtgt), self._p(ws), self._s())

    # ---- optimiser
    def adam_step(self, table, ntensors, chunk_tensor, chunk_off, nchunks, lr, b1, b2, eps, max_norm, grad_scale, ema_decay, norm_out, ws,
                  lr_dev=None, inv_scale=None, skip_nonfinite=False) -> Op:
        """lr_dev: device float that holds the learning rate (a scheduler rewrites it; `lr` is then ignored); inv_scale / skip_nonfinite:
        GradScaler semantics (gradients x *inv_scale; a non-finite norm skips the step); norm_out: [3] (norm, clip coefficient, found_inf)."""
        assert norm_out.numel() >= 3
        return self._call("gan_adam_step", self._p(table), ntensors, self._p(chunk_tensor), self._p(chunk_off), nchunks, C.c_float(lr),
                          C.c_float(b1), C.c_float(b2), C.c_float(eps), C.c_float(max_norm), C.c_float(grad_scale), C.c_float(ema_decay),
                          self._p(lr_dev), self._p(inv_scale), int(skip_nonfinite), self._p(norm_out), self._p(ws), self._s())

    def adam_step_wd(self, table, ntensors, chunk_tensor, chunk_off, nchunks, lr, b1, b2, eps, max_norm, grad_scale, ema_decay, norm_out, ws,
                     weight_decay, decoupled=False, lr_dev=None, inv_scale=None, skip_nonfinite=False) -> Op:
        """adam_step with torch's weight decay: torch.optim.Adam(weight_decay) (L2, added to the clipped gradient) or, decoupled,
        torch.optim.AdamW (p *= 1 - lr * weight_decay before the update).  The decay is not part of the norm."""
        assert norm_out.numel() >= 3
        return self._call("gan_adam_step_wd", self._p(table), ntensors, self._p(chunk_tensor), self._p(chunk_off), nchunks, C.c_float(lr),
                          C.c_float(b1), C.c_float(b2), C.c_float(eps), C.c_float(max_norm), C.c_float(grad_scale), C.c_float(ema_decay),
                          self._p(lr_dev), self._p(inv_scale), int(skip_nonfinite), C.c_float(weight_decay), int(decoupled), self._p(norm_out),
                          self._p(ws), self._s())

    def scaler_update(self, scale, inv_scale, tracker, found_inf, growth=2.0, backoff=0.5, interval=2000) -> Op:
        assert tracker.dtype == torch.int32
        return self._call("gan_scaler_update", self._p(scale), self._p(inv_scale), self._p(tracker), self._p(found_inf), C.c_float(growth),
                          C.c_float(backoff), int(interval), self._s())

    def make_adam_table(self, entries: Sequence[dict]) -> torch.Tensor:
        """entries: dicts with tensors p, g (or None), m, v, ema (or None), step (int32 tensor of 1).  -> device uint8 table."""
        arr = (GanAdamTensor * len(entries))()
        self._keep.append(entries)
        for i, e in enumerate(entries):
            arr[i].p, arr[i].m, arr[i].v = e["p"].data_ptr(), e["m"].data_ptr(), e["v"].data_ptr()
            arr[i].g = e["g"].data_ptr() if e.get("g") is not None else None
            arr[i].ema = e["ema"].data_ptr() if e.get("ema") is not None else None
            arr[i].numel, arr[i].step = e["p"].numel(), e["step"].data_ptr()
        raw = bytes(arr)
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)

    def fill(self, t: torch.Tensor, value: float) -> Op:
        assert t.dtype == torch.float32
        return self._call("gan_fill_f32", self._p(t), C.c_int64(t.numel()), C.c_float(value), self._s())

    def axpy(self, y: torch.Tensor, x: torch.Tensor, a: float) -> Op:
        return self._call("gan_axpy_f32", self._p(y), self._p(x), C.c_float(a), C.c_int64(y.numel()), self._s())

    def zero_(self, t: torch.Tensor) -> Op:
        """Byte-zero of any buffer (hipMemsetAsync through torch, graph-capturable)."""
        self._keep.append(t)

        def op():
            t.zero_()
        return op


class Ctx:
    """Allocation context: device, operand dtype, op layer and shared scratch workspaces."""

    def __init__(self, ops, device, dtype: int):
        self.ops, self.device, self.dtype = ops, torch.device(device), dtype
        self.tdtype = torch_dtype(dtype)
        self._scratch, self._retired = {}, []

    def view(self, B, H, W, C_, halo=0, dtype: Optional[int] = None) -> View:
        dt = self.dtype if dtype is None else dtype
        t = torch.zeros(B * (H + 2 * halo) * (W + 2 * halo) * C_, dtype=torch_dtype(dt), device=self.device)
        return View(t, B, H, W, C_, halo, dt)

    def f32(self, n, fill=0.0) -> torch.Tensor:
        return torch.full((int(n),), fill, dtype=torch.float32, device=self.device)

    def i32(self, values) -> torch.Tensor:
        return torch.tensor(list(values), dtype=torch.int32, device=self.device)

    def scratch(self, name: str, nfloats: int) -> torch.Tensor:
        """Grow-only shared fp32 workspace (safe to share: all launches are ordered on one stream)."""
        cur = self._scratch.get(name)
        if cur is None or cur.numel() < nfloats:
            if cur is not None:
                self._retired.append(cur)  # ops built earlier hold its raw pointer
            cur = torch.zeros(int(nfloats), dtype=torch.float32, device=self.device)
            self._scratch[name] = cur
        return cur


def check_weight_decay(weight_decay):
    """torch.optim.Adam's refusal, at construction as torch has it and where the launch is chosen (a NaN fails the comparison too)."""
    if not weight_decay >= 0.0:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")


class AdamPlan:
    """What a fused clip + Adam (+ EMA) launch over a fixed set of tensors needs besides them: the ADAM_CHUNK slices, norm_out, the
    workspace, the table, the learning rate (host value beside the device float the kernels read: a scheduler rewrites that and rebuilds
    nothing) and the prebuilt launches.  cut.FusedAdam, training.HipAdam and training.fused_adam_launch are its front ends.
    `entries` as make_adam_table takes them; the table is made with the first launch."""

    def __init__(self, ctx: Ctx, entries: Sequence[dict], lr: float):
        self.ctx, self.entries, self.n, self.lr = ctx, entries, len(entries), float(lr)
        ct, co = [], []
        for i, e in enumerate(entries):
            for off in range(0, e["p"].numel(), ADAM_CHUNK):
                ct.append(i); co.append(off)
        self.nchunks = len(ct)
        self.chunk_tensor, self.chunk_off = ctx.i32(ct), torch.tensor(co, dtype=torch.int64, device=ctx.device)
        self.norm_out, self.ws, self.lr_dev = ctx.f32(4), ctx.f32(self.nchunks + 16), ctx.f32(1, self.lr)
        self._table, self._ops = None, {}

    def table(self, entries: Optional[Sequence[dict]] = None) -> torch.Tensor:
        """The plan's table (made once), or a new one for other entries over the same tensors (FusedAdam's skip sets share the chunks,
        norm_out and the workspace); the caller keeps such a table alive and passes it to step_op."""
        if entries is not None:
            return self.ctx.ops.make_adam_table(entries)
        if self._table is None:
            self._table = self.ctx.ops.make_adam_table(self.entries)
        return self._table

    def set_lr(self, lr: float):
        if float(lr) != self.lr:      # a scheduler moved the rate: one device float follows, the prebuilt launches stay
            self.lr = float(lr)
            self.lr_dev.fill_(self.lr)

    def step_op(self, b1, b2, eps, max_norm, grad_scale, ema_decay, weight_decay=0.0, decoupled=False, inv_scale=None, skip_nonfinite=False,
                table=None, cached=True) -> Op:
        """The launch for these arguments, gan_adam_step without decay and gan_adam_step_wd with it, built once per argument tuple
        (cached=False: a new one, for a trainer that builds its update programs again).  The positional lr is the plan's when the launch
        is built; the kernels read lr_dev."""
        table = self.table() if table is None else table
        key = (id(table), b1, b2, eps, max_norm, grad_scale, ema_decay, float(weight_decay), bool(decoupled) and weight_decay != 0.0,
               inv_scale.data_ptr() if inv_scale is not None else 0, bool(skip_nonfinite))
        op = self._ops.get(key) if cached else None
        if op is None:
            check_weight_decay(weight_decay)
            args = (table, self.n, self.chunk_tensor, self.chunk_off, self.nchunks, self.lr, b1, b2, eps, max_norm, grad_scale, ema_decay,
                    self.norm_out, self.ws)
            kw = dict(lr_dev=self.lr_dev)
            if inv_scale is not None or skip_nonfinite:      # GradScaler's arguments only where a caller gives them
                kw.update(inv_scale=inv_scale, skip_nonfinite=skip_nonfinite)
            if weight_decay == 0.0:
                op = self.ctx.ops.adam_step(*args, **kw)
            else:
                op = self.ctx.ops.adam_step_wd(*args, float(weight_decay), bool(decoupled), **kw)
            self._ops[key] = op
        return op


def stream_key(device) -> int:
    """Last part of every plan key.  The op layer bakes the stream that is current on the TENSORS' device into a plan's launches
    (HipOps._s) while the staging copies run on whatever stream is current there at each call: keyed on that stream's handle, a caller on
    another stream (`with torch.cuda.stream(s)`) gets a plan of its own, not an unordered pair -- also on a GPU that is not current."""
    device = torch.device(device)
    return torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0


def cached_plan(cache: dict, key: tuple, device, make):
    key = key + (stream_key(device),)
    if key not in cache:
        cache[key] = make()
    return cache[key]


def cpad(c: int) -> int:
    """Channel padding rule of halo-NHWC: next power of two >= 8."""
    p = 8
    while p < c:
        p *= 2
    return p
