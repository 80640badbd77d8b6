"""TEST INFRASTRUCTURE: cases, runner and assertions for the weight-gradient family -- gan_conv_wgrad (csrc/conv_wgrad.hip's generic
kernel, csrc/wgrad_patch.hip's range-patch kernel, csrc/conv_win7.hip's two window kernels), gan_wgrad_reduce and gan_bias_grad --
written against an op layer: tests/test_wgrad_family_cpu.py runs them on the emulator, tests/test_wgrad_family_gpu.py on HipOps, with the
same shapes and the same assertions.  The float64 statements are in tests/wgrad_ref64.py; the bounds are tests/cases.derived_bound and,
for the reduction alone, the worst-case sum bound nsplit * 2^-24 * sum_s |part[s]|.  No tolerance here is fitted to a measured error.

A `Case` is a layer geometry, a batch, a dtype, the halos of the tap operand and of the row operand, and the launch it is meant for
(variant, nsplit, addressing path, lanes of the reduction).  `run` plans ConvLayer.wgrad(x, dy, accumulate, bias_too=True) on a wrapping
op layer that points the planned call's `part` at a guarded buffer (grad_w and grad_b are guarded from the start), launches twice and
asserts, before any figure is compared:
  * the recorded call names the kernel the case is meant for; on the library also the reduction's lane count -- a miss fails;
  * every element of part[:nsplit * N * ntaps * Cx] was written (it starts as NaN), and no guard zone of part, grad_w or grad_b;
  * x, dy and the tap table are bit-unchanged; the second launch gave the same bits.
The row operand (dy; the layer input of a transposed layer) carries a NaN halo: it must not be read."""
import math
from collections import namedtuple

import torch

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd._lib import GanError
from gan_variant_research_amd.convplan import ConvLayer
from gan_variant_research_amd.runtime import Ctx, View, cpad
from tests import wgrad_ref64 as R
from tests.cases import derived_bound, to_view
from tests.conv_cases import GUARD, NAME, TDT, _gen, bits, guarded_f32, sync
from tests.emulator import HALO_REFLECT, HALO_ZERO, EmuOps

ST_FILL, GW_FILL, GB_FILL = -9.0, 7.5, -3.25      # sentinels: guard zones of part; grad_w and grad_b before a launch that does not accumulate
NAN = float("nan")

Geom = namedtuple("Geom", "cin cout k s p tr H W")
Case = namedtuple("Case", "g B dtype xh gh variant nsplit fast lanes")


def out_hw(g):
    return (2 * g.H, 2 * g.W) if g.tr else ((g.H + 2 * g.p - g.k) // g.s + 1, (g.W + 2 * g.p - g.k) // g.s + 1)


def reflects(S):
    """the tap operand's halo mode: reflect for the stride-1 k3 / k7 layers whose map is larger than the halo, else zero"""
    g = S.g
    return (not g.tr) and g.s == 1 and g.k in (3, 7) and min(g.H, g.W) > S.xh


def kernel_of(S):
    if S.variant == 2:
        return "window-to3" if S.g.cin == 64 else "window-from3"
    return "range-patch" if S.variant == 1 else f"generic-{NAME[S.dtype]}"


def case_id(S):
    g = S.g
    return f"{g.cin}-{g.cout}k{g.k}s{g.s}{'T' if g.tr else ''}-{g.H}x{g.W}-B{S.B}-{NAME[S.dtype]}-x{S.xh}g{S.gh}"


# ------------------------------------------------------------------------------------------------ the cases
# generic kernel: (cin, cout, k, s, p, transposed, H, W), B, fast addressing path, nsplit (bf16, fp32), lanes of the reduction
F_, T_ = False, True
GENERIC_TABLE = [
    ((8, 8, 3, 1, 1, F_, 1, 1), 1, 0, (1, 1), 1),           # M = 1: one partial stage, the decomp clamp, skinny tile, Ktot = 72 < 128 (the xtap clamp)
    ((8, 8, 3, 1, 1, F_, 1, 1), 3, 0, (1, 1), 1),           # M = 3
    ((16, 32, 3, 1, 1, F_, 8, 8), 1, 1, (1, 1), 1),         # M = 64, fast path, N = 32 inside one tile: the gn clamp
    ((16, 32, 3, 1, 1, F_, 7, 9), 1, 0, (1, 1), 1),         # M = 63, general path
    ((16, 32, 3, 1, 1, F_, 5, 13), 1, 0, (1, 1), 1),        # M = 65
    ((16, 32, 3, 1, 1, F_, 8, 24), 1, 0, (1, 1), 1),        # HoWo % 64 == 0 but Wo = 24: general path
    ((16, 32, 3, 1, 1, F_, 2, 64), 2, 1, (1, 1), 1),        # fast path with Wo % 64 == 0
    ((16, 32, 3, 1, 1, F_, 1, 128), 2, 1, (1, 1), 1),
    ((16, 32, 3, 1, 1, F_, 4, 16), 3, 1, (1, 1), 1),        # fast path with 64 % Wo == 0
    ((16, 32, 3, 1, 1, F_, 37, 1), 2, 0, (1, 1), 1),        # Wo = 1
    ((16, 32, 3, 1, 1, F_, 1, 37), 2, 0, (1, 1), 1),        # Ho = 1
    ((16, 32, 3, 1, 1, F_, 19, 19), 3, 0, (2, 2), 1),       # M = 1083: 2 splits of 576, the second starting inside image 1, tail of 59 rows
    ((8, 8, 3, 1, 1, F_, 19, 19), 3, 0, (2, 2), 1),         # the same, skinny
    ((8, 8, 3, 1, 1, F_, 33, 33), 2, 0, (4, 4), 1),         # 4 splits, tail of 2 rows
    ((8, 8, 3, 1, 1, F_, 32, 32), 2, 1, (4, 4), 1),         # 4 splits of 512 on the fast path, each starting mid-image
    ((64, 128, 3, 1, 1, F_, 16, 16), 66, 1, (33, 27), 4),   # > 64 small images, no even grouping: 33 x 512 (bf16), 27 x 640 (fp32: mid-image starts)
    ((32, 1, 4, 1, 1, F_, 9, 6), 3, 0, (1, 1), 1),          # 16 taps, N = 8
    ((256, 1, 4, 1, 1, F_, 5, 9), 2, 0, (1, 1), 1),
    ((512, 1, 4, 1, 1, F_, 8, 5), 2, 0, (1, 1), 1),
    ((256, 512, 4, 1, 1, F_, 9, 7), 2, 0, (1, 1), 1),       # N = 512: 4 / 8 n-tiles
    ((3, 16, 7, 1, 3, F_, 5, 23), 3, 0, (1, 1), 1),         # 49 taps, Cx = 8, N = 16 skinny
    ((16, 3, 7, 1, 3, F_, 12, 7), 2, 0, (1, 1), 1),         # 49 taps, Cx = 16
    ((16, 32, 3, 2, 1, F_, 6, 14), 3, 0, (1, 1), 1),        # stride 2
    ((16, 32, 3, 2, 1, F_, 7, 13), 3, 0, (1, 1), 1),        # stride 2 on an odd map
    ((64, 128, 4, 2, 1, F_, 6, 10), 3, 0, (1, 1), 1),       # k4 s2
    ((3, 16, 4, 2, 1, F_, 12, 10), 3, 0, (1, 1), 1),        # k4 s2, Cx = 8
    ((128, 64, 3, 2, 1, T_, 3, 9), 3, 0, (1, 1), 1),        # transposed: the roles swap, stride 2 on dy
    ((32, 16, 3, 2, 1, T_, 6, 5), 2, 0, (1, 1), 1),
    ((64, 128, 3, 1, 1, F_, 7, 16), 1, 0, (1, 1), 1),       # HoWo = 112: one row short of the range-patch kernel
    ((64, 128, 3, 1, 1, F_, 16, 8), 1, 1, (1, 1), 1),       # Wo = 8: range-patch refuses
    ((32, 128, 3, 1, 1, F_, 8, 16), 1, 1, (1, 1), 1),       # range-patch refuses on channels
    ((64, 64, 3, 1, 1, F_, 8, 16), 1, 1, (1, 1), 1),
    ((64, 256, 3, 1, 1, F_, 40, 40), 1, 0, (3, 3), 1),      # Wo = 40, 3 splits
]
BIG = {      # the long reductions (left out of the emulator's per-slab run)
    (64, 128, 3, 1, 1, F_, 16, 16), (256, 256, 3, 1, 1, F_, 16, 16), (64, 3, 7, 1, 3, F_, 33, 36), (3, 64, 7, 1, 3, F_, 33, 36)}
# range-patch kernel (bf16): geometry, B, nsplit, fast (not used by that kernel: what the formula gives)
PATCH_TABLE = [
    ((64, 128, 3, 1, 1, F_, 8, 16), 1, 1, 1),               # the smallest map it takes
    ((64, 128, 3, 1, 1, F_, 2, 64), 1, 1, 1),
    ((64, 128, 3, 1, 1, F_, 1, 128), 1, 1, 1),              # one row of the 128-wide row-ring variant
    ((64, 128, 3, 1, 1, F_, 3, 128), 1, 1, 1),
    ((64, 128, 3, 1, 1, F_, 4, 32), 3, 3, 1),
    ((128, 256, 3, 1, 1, F_, 10, 16), 2, 2, 0),             # HoWo = 160: a tail range
    ((256, 256, 3, 1, 1, F_, 8, 16), 3, 3, 1),
    ((256, 256, 3, 1, 1, F_, 16, 16), 64, 32, 1),           # two whole images per split
]
# 7x7 window kernels (bf16), 64 -> 3 and 3 -> 64: H, W, B, nsplit, fast, lanes (to3, from3)
WINDOW_TABLE = [(16, 16, 1, 1, 1, (1, 1)), (1, 9, 3, 3, 0, (1, 1)), (9, 20, 3, 6, 0, (1, 1)), (17, 33, 3, 18, 0, (4, 4)),
                (33, 36, 29, 256, 0, (32, 16))]             # 261 tiles on 256 persistent blocks: blocks 0 .. 4 walk a second tile, in another image


def _halos(g, xh_min):
    """(tap-operand halo, row-operand halo): the smallest, then one more ring on the tap operand (origin 1) and k - 1 on the row operand"""
    return [(xh_min, 0), (xh_min + 1, g[2] - 1)]


def _cases():
    gen, patch, win = [], [], []
    for g, B, fast, ns, lanes in GENERIC_TABLE:
        for dt, n in zip((BF16, F32), ns):
            for xh, gh in _halos(g, 1 if g[5] else g[4]):
                gen.append(Case(Geom(*g), B, dt, xh, gh, 0, n, fast, lanes))
    gen.append(Case(Geom(16, 32, 3, 1, 1, F_, 7, 9), 1, BF16, 3, 0, 0, 1, 0, 1))                 # a k3 layer reading an x view of halo 3
    gen += [Case(Geom(256, 256, 3, 1, 1, F_, 16, 16), 64, F32, xh, gh, 0, 3, 1, 1) for xh, gh in ((1, 0), (2, 2))]      # fp32 only: 3 splits of 5504 rows, the second starts at row 128 of image 21
    for g, B, ns, fast in PATCH_TABLE:
        patch += [Case(Geom(*g), B, BF16, xh, gh, 1, ns, fast, 1) for xh, gh in _halos(g, 1)]
    for H, W, B, ns, fast, lanes in WINDOW_TABLE:
        for (cin, cout), ln in zip(((64, 3), (3, 64)), lanes):
            g = (cin, cout, 7, 1, 3, F_, H, W)
            win += [Case(Geom(*g), B, BF16, xh, gh, 2, ns, fast, ln) for xh, gh in _halos(g, 3)]
    return gen, patch, win


GENERIC, PATCH, WINDOW = _cases()
CASES = GENERIC + PATCH + WINDOW
KERNELS = ["generic-bf16", "generic-fp32", "range-patch", "window-to3", "window-from3"]


def find(g, B, dtype, i=0):
    """the i-th halo variant of a listed case"""
    return [S for S in CASES if tuple(S.g) == tuple(g) and S.B == B and S.dtype == dtype][i]


# accumulate = True on seeded prior values: one case per kernel and dtype, multi-split and single
ACCUMULATE = [find((16, 32, 3, 1, 1, F_, 19, 19), 3, BF16), find((8, 8, 3, 1, 1, F_, 33, 33), 2, F32), find((3, 16, 7, 1, 3, F_, 5, 23), 3, BF16, 1),
              find((128, 64, 3, 2, 1, T_, 3, 9), 3, F32), find((32, 1, 4, 1, 1, F_, 9, 6), 3, BF16), find((64, 128, 3, 1, 1, F_, 4, 32), 3, BF16),
              find((128, 256, 3, 1, 1, F_, 10, 16), 2, BF16, 1), find((64, 3, 7, 1, 3, F_, 17, 33), 3, BF16), find((3, 64, 7, 1, 3, F_, 9, 20), 3, BF16, 1)]
BIAS_ACCUMULATE_DIFFERS = find((16, 32, 3, 2, 1, F_, 7, 13), 3, BF16)       # accumulate = True, bias_accumulate = False
# one NaN in a real channel of an interior pixel of image 1 of 3
NAN_CASES = [find((16, 32, 3, 1, 1, F_, 19, 19), 3, BF16), find((8, 8, 3, 1, 1, F_, 19, 19), 3, F32, 1), find((16, 32, 3, 2, 1, F_, 7, 13), 3, BF16),
             find((64, 128, 3, 1, 1, F_, 4, 32), 3, BF16), find((64, 3, 7, 1, 3, F_, 9, 20), 3, BF16), find((3, 64, 7, 1, 3, F_, 9, 20), 3, BF16, 1)]


# ------------------------------------------------------------------------------------------------ op layers
class Guarding:
    """an op layer that points the weight-gradient call it is asked to build at a guarded partial buffer and remembers it"""

    def __init__(self, ops, ctx, launch=True):
        self._ops, self._ctx, self._launch = ops, ctx, launch
        self.call = self.part = self.part_big = self.reduce_args = None

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def conv_wgrad(self, c):
        assert self.call is None
        n = c.nsplit * c.N * c.ntaps * c.Cx
        self.part, self.part_big = guarded_f32(self._ctx, n, ST_FILL)
        c.part, self.call = self.part, c
        return self._ops.conv_wgrad(c) if self._launch else None

    def wgrad_reduce(self, part, *a):
        self.reduce_args = a
        return self._ops.wgrad_reduce(self.part, *a) if self._launch else None

    def bias_grad(self, *a):
        return self._ops.bias_grad(*a) if self._launch else None


class SlabEmuOps(EmuOps):
    """The emulator with the generic kernel's split decomposition: slab s holds the pixels [s * Ms, min(M, (s + 1) * Ms)) as gan_conv_wgrad
    cuts them (the plain emulator puts everything into slab 0).  Lets the per-slab assertion run, and be shown to bite, without a GPU."""
    slabbed = True

    def conv_wgrad(self, c):
        if c.variant != 0:
            return super().conv_wgrad(c)

        def op():
            out = R.desc64(R.desc_of(c), c.x.padded().double(), c.g.padded().double(), slab_ranges(c))
            c.part.view(-1)[:out.numel()] = out.float().reshape(-1)
        return op


def slab_ranges(c):
    M = c.B * c.Ho * c.Wo
    Ms = R.slab_rows(M, c.nsplit)
    return [(s * Ms, min(M, (s + 1) * Ms)) for s in range(c.nsplit)]


def is_fast(c):
    return int((c.Ho * c.Wo) % 64 == 0 and (c.Wo % 64 == 0 or 64 % c.Wo == 0))


def assert_reached(S, ops, call, reduce_args, lanes_of=None):
    """variant, nsplit and addressing path are those the case names; with the library's host function at hand also the lanes of the reduction"""
    what = case_id(S)
    got = (call.variant, call.nsplit, is_fast(call))
    assert got == (S.variant, S.nsplit, S.fast), f"{what}: planned (variant, nsplit, fast) = {got}, the case names {(S.variant, S.nsplit, S.fast)}"
    lanes_of = lanes_of or (ops.wgrad_reduce_lanes if ops.is_hip else None)
    if lanes_of is not None:
        nsplit, N, ntaps, Cx, N_real = reduce_args[:5]
        assert (nsplit, N, ntaps, Cx) == (call.nsplit, call.N, call.ntaps, call.Cx)
        G = lanes_of(nsplit, N_real, ntaps, Cx)
        assert G == S.lanes, f"{what}: the reduction takes {G} lanes, the case names {S.lanes}"


# ------------------------------------------------------------------------------------------------ data
def operands(S, poison=None):
    """the layer input and the output gradient, NCHW, N(0,1) rounded to the dtype, image by image.  poison: 'x' | 'dy': one NaN in real
    channel 1 of an interior pixel of image 1."""
    g = S.g
    Ho, Wo = out_hw(g)
    x = torch.stack([torch.randn(g.cin, g.H, g.W, generator=_gen(g.H, g.W, g.cin, b, 21)) for b in range(S.B)]).to(TDT[S.dtype]).float()
    dy = torch.stack([torch.randn(g.cout, Ho, Wo, generator=_gen(Ho, Wo, g.cout, b, 23)) for b in range(S.B)]).to(TDT[S.dtype]).float()
    if poison:
        t = x if poison == "x" else dy
        t[1, 1, t.shape[2] // 2, t.shape[3] // 2] = NAN
    return x, dy


def nan_halo(v):
    """fills the halo of a view with NaN and leaves its interior as it is"""
    if v.halo:
        keep = v.nhwc().clone()
        v.t.fill_(NAN)
        v.nhwc().copy_(keep)


def priors(S, dev):
    g = S.g
    n = g.cin * g.cout * g.k * g.k
    gen = _gen(n, g.cout, 29)
    return torch.randn(n, generator=gen).to(dev), torch.randn(g.cout, generator=gen).to(dev)


# ------------------------------------------------------------------------------------------------ one planned request, launched
def run(make, S, accumulate=False, bias_accumulate=None, poison=None):
    """plans S on make(S.dtype)'s op layer, launches it twice and returns what it left (tensors on the context's device)"""
    ctx = make(S.dtype)
    ops = Guarding(ctx.ops, ctx)
    ctx.ops = ops
    g, dev, what = S.g, ctx.device, case_id(S)
    wshape = (g.cin, g.cout, g.k, g.k) if g.tr else (g.cout, g.cin, g.k, g.k)
    n_w = g.cin * g.cout * g.k * g.k
    gw, gw_big = guarded_f32(ctx, n_w, GW_FILL)
    gb, gb_big = guarded_f32(ctx, g.cout, GB_FILL)
    layer = ConvLayer(ctx, torch.zeros(wshape, device=dev), torch.zeros(g.cout, device=dev), gw.view(wshape), gb, g.k, g.s, g.p, g.tr)
    x, dy = operands(S, poison)
    if g.tr:        # rows run over the layer input; the taps over dy
        xv, dyv = to_view(ctx, x, S.gh, HALO_ZERO), to_view(ctx, dy, S.xh, HALO_ZERO)
        nan_halo(xv)
    else:
        xv, dyv = to_view(ctx, x, S.xh, HALO_REFLECT if reflects(S) else HALO_ZERO), to_view(ctx, dy, S.gh, HALO_ZERO)
        nan_halo(dyv)
    launches = layer.wgrad(xv, dyv, accumulate, bias_too=True, bias_accumulate=bias_accumulate)
    call = ops.call
    assert call is not None and len(launches) == 3, f"{what}: {len(launches)} launches"
    assert_reached(S, ops, call, ops.reduce_args)
    bias_acc = accumulate if bias_accumulate is None else bias_accumulate
    Pw, Pb = priors(S, dev)
    n_part = call.nsplit * call.N * call.ntaps * call.Cx
    sync(ctx)
    before = [bits(t) for t in (xv.t, dyv.t, call.tapoff)]
    snaps = []
    for _ in range(2):
        ops.part_big.fill_(ST_FILL)
        ops.part.fill_(NAN)
        gw_big.fill_(GW_FILL)
        gb_big.fill_(GB_FILL)
        if accumulate:
            gw.copy_(Pw)
        if bias_acc:
            gb.copy_(Pb)
        for o in launches:
            o()
        sync(ctx)
        snaps.append([bits(t) for t in (ops.part_big, gw_big, gb_big)])
    after = [bits(t) for t in (xv.t, dyv.t, call.tapoff)]
    assert all(torch.equal(a, b) for a, b in zip(before, after)), f"{what}: x, dy or the tap table changed"
    for name, a, b in zip(("part", "grad_w", "grad_b"), *snaps):
        assert torch.equal(a, b), f"{what}: a repeated launch gave other bits in {name}"
    for name, big, fill in (("part", ops.part_big, ST_FILL), ("grad_w", gw_big, GW_FILL), ("grad_b", gb_big, GB_FILL)):
        assert bool((big[:GUARD] == fill).all() and (big[-GUARD:] == fill).all()), f"{what}: a guard zone of {name} was written"
    assert ops.part.numel() == n_part
    if not poison:
        assert not bool(torch.isnan(ops.part).any()), f"{what}: {int(torch.isnan(ops.part).sum())} elements of part[:nsplit * N * ntaps * Cx] were not written"
        if not accumulate:
            assert bool((gw != GW_FILL).all()), f"{what}: an element [n < N_real][c < C_real][k] of grad_w was not written"
        if not bias_acc:
            assert bool((gb != GB_FILL).all()), f"{what}: an element of grad_b[:cout] was not written"
    return {"case": S, "call": call, "desc": R.desc_of(call), "slabbed": getattr(ctx.ops._ops, "slabbed", ctx.ops.is_hip) and call.variant == 0,
            "ranges": slab_ranges(call), "part": ops.part.clone().view(call.nsplit, call.N, call.ntaps, call.Cx), "gw": gw.clone().view(wshape),
            "gb": gb.clone(), "xpad": call.x.padded().double(), "gpad": call.g.padded().double(), "dypad": dyv.padded().double(),
            "x64": x.double().to(dev), "dy64": dy.double().to(dev), "Pw": Pw.view(wshape), "Pb": Pb, "wshape": wshape, "dev": dev.type}


_results = {}


def result(make, S, **kw):
    ctx = make(S.dtype)
    k = (ctx.device.type, type(ctx.ops).__name__, S, tuple(sorted(kw.items())))
    if k not in _results:
        _results[k] = run(make, S, **kw)
    return _results[k]


# ------------------------------------------------------------------------------------------------ references, right and wrong
class Ref:
    missing_pixel = shift_first_row = swap_taps = wrong_stride = zero_pad = swap_index = ignore_accumulate = bias_with_halo = False


def _wrong(name, **kw):
    return type(name, (Ref,), kw)


WRONG = [_wrong("LastPixelOfTheLastImageLeftOut", missing_pixel=True), _wrong("FirstRowOfASplitInTheNeighbouringSlab", shift_first_row=True),
         _wrong("TapRowsAndColumnsSwapped", swap_taps=True), _wrong("StrideOnTheWrongOperandOfTheTransposedLayer", wrong_stride=True),
         _wrong("ZeroPaddingForReflect", zero_pad=True), _wrong("SwapIndexFormulaForThePlainOne", swap_index=True),
         _wrong("AccumulateIgnored", ignore_accumulate=True), _wrong("HaloOfDySummedIntoTheBiasGradient", bias_with_halo=True)]


def _layer64(S, x64, dy64, wshape, ref):
    """tests/cases.conv_ref64('wgrad') over image chunks (the sum over the batch is exact in the statement: chunks only bound the unfold)"""
    g = S.g
    per = max(1, (1 << 23) // max(1, (g.cout if g.tr else g.cin) * g.k * g.k * x64.shape[2] * x64.shape[3] * (4 if g.tr else 1)))
    tot = None
    for b0 in range(0, S.B, per):
        r, A, K = R.layer64(g.k, g.s, g.p, g.tr, reflects(S), x64[b0:b0 + per], dy64[b0:b0 + per], wshape, swap_taps=ref.swap_taps, zero_pad=ref.zero_pad,
                            wrong_stride=ref.wrong_stride)
        tot = (r, A, K) if tot is None else (tot[0] + r, tot[1] + A, tot[2] + K)
    return tot


def ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / (bound + 1e-300)).max())


_worst, _count, _rejecting = {}, {}, []


def report(dev, kernel, what, r, note=""):
    if _rejecting:
        print(f"[wgrad-family] (against the wrong reference {_rejecting[0]}) {kernel} {what}: {r:.3g}")
        return
    _worst[(dev, kernel)] = max(_worst.get((dev, kernel), 0.0), r)
    print(f"[wgrad-family] {kernel:13s} {what}: error / bound = {r:.3g}{note}   (worst of the variant so far {_worst[(dev, kernel)]:.3g})")


def check(make, S, ref=None):
    """the result of S against the float64 statements: the reduced gradient, the sum of the slabs, each slab of the generic kernel (where
    the op layer cuts slabs) and the bias gradient.  Returns the worst error / bound."""
    ref = ref or Ref()
    res = result(make, S)
    what, g, d = case_id(S), S.g, res["desc"]
    x64, dy64, xpad, gpad, dypad = res["x64"], res["dy64"], res["xpad"], res["gpad"], res["dypad"]
    if ref.missing_pixel:       # the last pixel of the last image of the row operand
        x64, dy64, gpad, dypad = x64.clone(), dy64.clone(), gpad.clone(), dypad.clone()
        (x64 if g.tr else dy64)[-1, :, -1, -1] = 0.0
        gpad[-1, d.g_y0 + (d.Ho - 1) * d.g_sy, d.g_x0 + (d.Wo - 1) * d.g_sx] = 0.0
        if not g.tr:
            dypad[-1, S.gh + d.Ho - 1, S.gh + d.Wo - 1] = 0.0
    M = d.B * d.Ho * d.Wo
    rw, Aw, K = _layer64(S, x64, dy64, res["wshape"], ref)
    assert K == M, (K, M)
    figs = {"grad_w": ratio(res["gw"], rw, derived_bound(rw, Aw, K, 0.0))}
    kw = dict(swap_taps=ref.swap_taps)
    if ref.wrong_stride and g.tr:        # the same wrong statement at the descriptor: every second pixel of dy under a unit-stride window
        xp2 = xpad[:, S.xh:-S.xh, S.xh:-S.xh][:, ::2, ::2]
        xp2 = torch.nn.functional.pad(xp2, (0, 0, 1, 1, 1, 1))
        d2 = d._replace(x_Wp=xp2.shape[2], x_sy=1, x_sx=1, x_y0=0, x_x0=0, tapoff=tuple((kh * xp2.shape[2] + kw_) * d.Cx for kh in range(3) for kw_ in range(3)))
        sp, sa = R.desc64(d2, xp2, gpad)[0], R.desc64(d2, xp2, gpad, absolute=True)[0]
    else:
        if ref.zero_pad and reflects(S):
            xpad = torch.zeros_like(xpad)
            xpad[:, S.xh:S.xh + g.H, S.xh:S.xh + g.W] = res["xpad"][:, S.xh:S.xh + g.H, S.xh:S.xh + g.W]
        sp, sa = R.desc64(d, xpad, gpad, **kw)[0], R.desc64(d, xpad, gpad, absolute=True, **kw)[0]
    figs["sum of slabs"] = ratio(res["part"].double().sum(0), sp, derived_bound(sp, sa, M, 0.0))
    if res["slabbed"]:
        rs = R.desc64(d, xpad, gpad, res["ranges"], shift_first_row=ref.shift_first_row, **kw)
        ra = R.desc64(d, xpad, gpad, res["ranges"], absolute=True, shift_first_row=ref.shift_first_row, **kw)
        figs["slabs"] = max(ratio(res["part"][s], rs[s], derived_bound(rs[s], ra[s], m1 - m0, 0.0)) for s, (m0, m1) in enumerate(res["ranges"]))
    Ho, Wo = out_hw(g)
    rb, Ab, Kb = R.bias64(dypad, S.xh if g.tr else S.gh, Ho, Wo, g.cout, with_halo=ref.bias_with_halo)
    figs["grad_b"] = ratio(res["gb"], rb, derived_bound(rb, Ab, Kb, 0.0))
    worst = max(v if v == v else math.inf for v in figs.values())
    report(res["dev"], kernel_of(S), what, worst, "  (" + ", ".join(f"{k} {v:.3g}" for k, v in figs.items()) + f"; K = {M}, {S.nsplit} slabs)")
    if not _rejecting:
        _count[(res["dev"], kernel_of(S))] = _count.get((res["dev"], kernel_of(S)), set()) | {S}
    if S not in KEEP:           # only the cases that further tests come back to stay cached
        _results.pop(next((k for k in _results if k[0] == res["dev"] and k[2] == S and not k[3]), None), None)
    for k, v in figs.items():
        assert v <= 1.0, f"{what}: {k}: max error / bound = {v:.3g}"
    return worst


def check_accumulate(make, S, ref=None, bias_differs=False):
    """accumulate = True onto seeded prior values P is fl32(P + s), bit for bit, with s what the same launch gives with accumulate = False;
    bias_differs: accumulate = True with bias_accumulate = False leaves grad_b = s"""
    ref = ref or Ref()
    base = result(make, S)
    acc = result(make, S, accumulate=True, bias_accumulate=False) if bias_differs else result(make, S, accumulate=True)
    assert torch.equal(bits(acc["part"]), bits(base["part"])), f"{case_id(S)}: the slabs depend on accumulate"
    want_w = base["gw"] if ref.ignore_accumulate else acc["Pw"] + base["gw"]
    want_b = base["gb"] if (ref.ignore_accumulate or bias_differs) else acc["Pb"] + base["gb"]
    assert torch.equal(bits(acc["gw"]), bits(want_w)), f"{case_id(S)}: grad_w after accumulate is not fl32(P + s): {int((bits(acc['gw']) != bits(want_w)).sum())} elements differ"
    assert torch.equal(bits(acc["gb"]), bits(want_b)), f"{case_id(S)}: grad_b after accumulate is not {'s' if bias_differs else 'fl32(P + s)'}"


_excused = {}


def check_nan(make, S, where):
    """One NaN in `where` ('dy' | 'x'): every element of grad_w (and, for 'dy', of grad_b) whose float64 reference is NaN is NaN, every
    other element is bit-identical to the clean run.  The excused set -- elements outside the reference's footprint that differ from the
    clean run -- is counted, and it is empty for every kernel of the family."""
    clean, bad = result(make, S), result(make, S, poison=where)
    what = f"{case_id(S)}-nan-{where}"
    rw, _, _ = _layer64(S, bad["x64"], bad["dy64"], bad["wshape"], Ref())
    nan_w = torch.isnan(rw)
    assert bool(nan_w.any()) and not bool(nan_w.all()), f"{what}: the poison reaches nothing, or everything"
    assert bool(torch.isnan(bad["gw"][nan_w]).all()), f"{what}: {int((~torch.isnan(bad['gw'][nan_w])).sum())} elements of grad_w whose reference is NaN are not NaN"
    differs = (bits(bad["gw"]) != bits(clean["gw"])).to(nan_w.device) & ~nan_w
    _excused[(bad["dev"], what)] = int(differs.sum())
    assert not bool(differs.any()), f"{what}: {int(differs.sum())} elements of grad_w outside the NaN's footprint differ from the clean run"
    nan_b = torch.isnan(bad["dy64"].sum((0, 2, 3)))
    assert bool(nan_b.any()) == (where == "dy")
    assert bool(torch.isnan(bad["gb"][nan_b]).all()), f"{what}: grad_b of the poisoned channel is not NaN"
    assert torch.equal(bits(bad["gb"])[~nan_b.cpu()], bits(clean["gb"])[~nan_b.cpu()]), f"{what}: grad_b outside the poisoned channel differs from the clean run"
    print(f"[wgrad-family] {what}: footprint {int(nan_w.sum())} of {nan_w.numel()} elements of grad_w, excused 0")


def check_plan(hip_ops, S):
    """the library's own plan for S, asked on the host (the queries are pure: no GPU): variant, nsplit, path and lanes are those the case names"""
    ctx = Ctx(None, "cpu", S.dtype)
    ops = Guarding(hip_ops, ctx, launch=False)
    ctx.ops = ops
    g = S.g
    Ho, Wo = out_hw(g)
    wshape = (g.cin, g.cout, g.k, g.k) if g.tr else (g.cout, g.cin, g.k, g.k)
    layer = ConvLayer(ctx, torch.zeros(wshape), torch.zeros(g.cout), torch.zeros(wshape), torch.zeros(g.cout), g.k, g.s, g.p, g.tr)
    layer.wgrad(ctx.view(S.B, g.H, g.W, cpad(g.cin), S.gh if g.tr else S.xh), ctx.view(S.B, Ho, Wo, cpad(g.cout), S.xh if g.tr else S.gh), False)
    assert_reached(S, ops, ops.call, ops.reduce_args, lanes_of=getattr(hip_ops, "wgrad_reduce_lanes", None))
    return ops.call


# ------------------------------------------------------------------------------------------------ the reduction on its own
RCase = namedtuple("RCase", "nsplit N ntaps Cx N_real C_real swap I2 KK khw lanes")
K9 = tuple(range(9))
REDUCE = [
    RCase(1, 16, 12, 16, 12, 12, False, 12, 9, K9 + (-1, -1, -1), 1),                    # one slab: a copy; ntaps padded beyond KK
    RCase(3, 8, 9, 8, 3, 5, True, 3, 9, K9, 1),                                           # swap, N_real < N, C_real = 5: the break inside the second quad
    RCase(8, 8, 12, 8, 8, 3, False, 8, 9, K9 + (-1, -1, -1), 2),                          # C_real = 3, I2 != C_real
    RCase(15, 16, 9, 8, 12, 8, False, 8, 9, (0, -1, 2, 3, -1, 5, 6, 7, 8), 2),            # khw with -1 entries, C_real = Cx
    RCase(16, 16, 9, 16, 16, 12, True, 20, 9, tuple(8 - k for k in K9), 4),               # swap with I2 != N_real, C_real = 12 of 16, flipped taps
    RCase(40, 64, 16, 8, 64, 5, False, 5, 16, tuple(range(16)), 8),
    RCase(100, 32, 9, 16, 20, 16, False, 16, 9, K9, 16),
    RCase(256, 8, 52, 64, 3, 64, False, 64, 49, tuple(range(49)) + (-1, -1, -1), 32),
]
REDUCE_PAST_THE_GRID = [RCase(1, 1024, 16, 512, 1024, 512, False, 512, 16, tuple(range(16)), 1),       # exactly 8192 blocks of quads
                        RCase(1, 1040, 16, 512, 1040, 512, False, 512, 16, tuple(range(16)), 1)]      # past them: the stride loop runs


def rcase_id(r):
    return f"s{r.nsplit}-N{r.N_real}of{r.N}-t{r.ntaps}-C{r.C_real}of{r.Cx}-{'swap' if r.swap else 'plain'}-I{r.I2}"


def body_reduce(make, r, accumulate, ref=None, lanes_of=None):
    """ops.wgrad_reduce on slabs of distinct seeded values against the float64 sum scattered by the index formula: within the worst-case
    bound of any summation order, a bit-exact copy for one slab, fl32(P + s) bit for bit with accumulate, untouched elements and guard
    zones bit-unchanged, the lane count the case names."""
    ref = ref or Ref()
    ctx = make(F32)
    ops, dev, what = ctx.ops, ctx.device, rcase_id(r) + ("-acc" if accumulate else "")
    lanes_of = lanes_of or (ops.wgrad_reduce_lanes if ops.is_hip else None)
    if lanes_of is not None:
        G = lanes_of(r.nsplit, r.N_real, r.ntaps, r.Cx)
        assert G == r.lanes, f"{what}: the reduction takes {G} lanes, the case names {r.lanes}"
    n = r.nsplit * r.N * r.ntaps * r.Cx
    gen = _gen(r.nsplit, r.N, r.ntaps, r.Cx, 31)
    part, part_big = guarded_f32(ctx, n, ST_FILL)
    part.copy_((torch.randn(n, generator=gen) * (1.0 + torch.arange(n) % 7)).to(dev))
    n_grad = (r.C_real if r.swap else r.N_real) * r.I2 * r.KK
    grad, grad_big = guarded_f32(ctx, n_grad, GW_FILL)
    P = torch.randn(n_grad, generator=gen).to(dev)
    khw = ctx.i32(r.khw)
    before = bits(part_big)
    out = []
    for acc in ((False, True) if accumulate else (False,)):
        op = ops.wgrad_reduce(part, r.nsplit, r.N, r.ntaps, r.Cx, r.N_real, r.C_real, r.swap, r.I2, r.KK, khw, grad, acc)
        for _ in range(2):
            grad_big.fill_(GW_FILL)
            if acc:
                grad.copy_(P)
            op()
            sync(ctx)
        out.append(grad.clone())
        assert bool((grad_big[:GUARD] == GW_FILL).all() and (grad_big[-GUARD:] == GW_FILL).all()), f"{what}: a guard zone of grad was written"
    assert torch.equal(before, bits(part_big)), f"{what}: the slabs changed"
    want, bound, touched = R.reduce64(part, r.nsplit, r.N, r.ntaps, r.Cx, r.N_real, r.C_real, r.swap != ref.swap_index, r.I2, r.KK, r.khw, n_grad)
    s = out[0]
    assert bool((s[~touched] == GW_FILL).all()), f"{what}: {int((s[~touched] != GW_FILL).sum())} elements of grad outside the index formula's image were written"
    rr = ratio(s[touched], want[touched], bound[touched])
    if r.nsplit == 1:
        assert torch.equal(bits(s[touched]), bits(want[touched].float())), f"{what}: one slab is not copied bit for bit"
    if accumulate:
        a = out[1]
        assert torch.equal(bits(a[~touched]), bits(P[~touched])), f"{what}: accumulate changed elements outside the index formula's image"
        want_a = s if ref.ignore_accumulate else P + s
        assert torch.equal(bits(a[touched]), bits(want_a[touched])), f"{what}: accumulate is not fl32(P + s) bit for bit"
    report(dev.type, f"reduce-G{r.lanes}", what, rr)
    assert rr <= 1.0, f"{what}: max error / bound = {rr:.3g}"
    return rr


# ------------------------------------------------------------------------------------------------ the bias gradient on its own
BCase = namedtuple("BCase", "dtype C B H W N_real")
BIAS = [BCase(BF16, 8, 1, 1, 1, 1), BCase(BF16, 8, 3, 5, 7, 3), BCase(BF16, 64, 1, 3, 11, 64), BCase(BF16, 512, 1, 65, 65, 512),
        BCase(F32, 8, 1, 1, 1, 1), BCase(F32, 8, 3, 5, 7, 3), BCase(F32, 512, 2, 9, 7, 512), BCase(F32, 1024, 1, 3, 3, 1024)]


def bcase_id(b):
    return f"{NAME[b.dtype]}-C{b.C}-B{b.B}-{b.H}x{b.W}-N{b.N_real}"


def body_bias(make, b, halo, ref=None):
    """ops.bias_grad over a view with a NaN halo against the float64 column sums of its logical pixels, accumulate both ways"""
    ref = ref or Ref()
    ctx = make(b.dtype)
    ops, dev, what = ctx.ops, ctx.device, f"{bcase_id(b)}-halo{halo}"
    v = ctx.view(b.B, b.H, b.W, b.C, halo)
    gen = _gen(b.C, b.B, b.H, b.W, 37)
    v.nhwc().copy_(torch.randn(b.B, b.H, b.W, b.C, generator=gen).to(TDT[b.dtype]).to(dev))
    nan_halo(v)
    grad, grad_big = guarded_f32(ctx, b.N_real, GB_FILL)
    P = torch.randn(b.N_real, generator=gen).to(dev)
    ws, ws_big = guarded_f32(ctx, 256 * max(b.C, 256), ST_FILL)
    before = bits(v.t)
    out = []
    for acc in (False, True):
        op = ops.bias_grad(v, b.N_real, grad, acc, ws)
        for _ in range(2):
            grad_big.fill_(GB_FILL)
            if acc:
                grad.copy_(P)
            op()
            sync(ctx)
        out.append(grad.clone())
        assert bool((grad_big[:GUARD] == GB_FILL).all() and (grad_big[-GUARD:] == GB_FILL).all()), f"{what}: a guard zone of grad was written"
        assert bool((ws_big[:GUARD] == ST_FILL).all() and (ws_big[-GUARD:] == ST_FILL).all()), f"{what}: a guard zone of the workspace was written"
    assert torch.equal(before, bits(v.t)), f"{what}: dy changed"
    rb, Ab, K = R.bias64(v.padded().double(), halo, b.H, b.W, b.N_real, with_halo=ref.bias_with_halo)
    rr = ratio(out[0], rb, derived_bound(rb, Ab, K, 0.0))
    rr = rr if rr == rr else math.inf
    want_a = out[0] if ref.ignore_accumulate else P + out[0]
    assert torch.equal(bits(out[1]), bits(want_a)), f"{what}: accumulate is not fl32(P + s) bit for bit"
    report(dev.type, f"bias-{NAME[b.dtype]}", what, rr)
    assert rr <= 1.0, f"{what}: max error / bound = {rr:.3g}"
    return rr


# ------------------------------------------------------------------------------------------------ wrong references
REJECT_ON = {
    "LastPixelOfTheLastImageLeftOut": [("case", find((16, 32, 3, 1, 1, F_, 19, 19), 3, BF16)), ("case", find((64, 128, 3, 1, 1, F_, 16, 16), 66, BF16)),
                                       ("case", find((64, 128, 3, 1, 1, F_, 4, 32), 3, BF16)), ("case", find((64, 3, 7, 1, 3, F_, 33, 36), 29, BF16)),
                                       ("case", find((3, 64, 7, 1, 3, F_, 33, 36), 29, BF16)), ("case", find((128, 64, 3, 2, 1, T_, 3, 9), 3, F32))],
    "FirstRowOfASplitInTheNeighbouringSlab": [("slab", find((16, 32, 3, 1, 1, F_, 19, 19), 3, BF16)), ("slab", find((8, 8, 3, 1, 1, F_, 32, 32), 2, F32)),
                                              ("slab", find((64, 128, 3, 1, 1, F_, 16, 16), 66, F32))],
    "TapRowsAndColumnsSwapped": [("case", find((16, 32, 3, 1, 1, F_, 7, 9), 1, BF16)), ("case", find((64, 128, 3, 1, 1, F_, 8, 16), 1, BF16)),
                                 ("case", find((3, 64, 7, 1, 3, F_, 9, 20), 3, BF16)), ("case", find((16, 32, 3, 2, 1, F_, 7, 13), 3, F32))],
    "StrideOnTheWrongOperandOfTheTransposedLayer": [("case", find((128, 64, 3, 2, 1, T_, 3, 9), 3, BF16)), ("case", find((32, 16, 3, 2, 1, T_, 6, 5), 2, F32))],
    "ZeroPaddingForReflect": [("case", find((16, 32, 3, 1, 1, F_, 7, 9), 1, F32)), ("case", find((64, 128, 3, 1, 1, F_, 4, 32), 3, BF16)),
                              ("case", find((64, 3, 7, 1, 3, F_, 9, 20), 3, BF16))],
    "SwapIndexFormulaForThePlainOne": [("reduce", REDUCE[1], False), ("reduce", REDUCE[0], True), ("reduce", REDUCE[6], False)],
    "AccumulateIgnored": [("acc", ACCUMULATE[0]), ("acc", ACCUMULATE[5]), ("reduce", REDUCE[5], True), ("bias", BIAS[1], 0)],
    "HaloOfDySummedIntoTheBiasGradient": [("bias", BIAS[1], 2), ("bias", BIAS[6], 2), ("case", find((16, 32, 3, 1, 1, F_, 7, 9), 1, BF16, 1))],
}


KEEP = set(ACCUMULATE + NAN_CASES + [BIAS_ACCUMULATE_DIFFERS] + [n[1] for v in REJECT_ON.values() for n in v if n[0] in ("case", "slab", "acc")])


def rejects(make, wrong, make_slabbed=None):
    """every named case fails its assertions against the wrong reference; `make_slabbed`: the op layer the per-slab cases run on"""
    failed, named = [], REJECT_ON[wrong.__name__]
    _rejecting.append(wrong.__name__)
    try:
        for kind, S, *rest in named:
            mk = make_slabbed if (kind == "slab" and make_slabbed is not None) else make
            if kind in ("case", "slab", "acc"):
                result(mk, S)              # planning and contract assertions are not what rejects a reference: they fail here, outside the try
            try:
                if kind in ("case", "slab"):
                    check(mk, S, wrong())
                elif kind == "acc":
                    check_accumulate(mk, S, wrong())
                elif kind == "reduce":
                    body_reduce(mk, S, rest[0], wrong())
                else:
                    body_bias(mk, S, rest[0], wrong())
            except AssertionError as e:
                failed.append((kind, str(e)[:100]))
    finally:
        _rejecting.clear()
    print(f"[wgrad-family] {wrong.__name__} rejected on {failed}")
    assert len(failed) == len(named), f"the assertions accept the wrong reference {wrong.__name__} on a case it was tried on: {failed}"


def summary(make):
    """Worst error / bound per kernel variant on this device; results are cached, so nothing that a test of its own already ran runs again.
    A miss fails in the case's own test and is only listed here; a variant without a figure of THIS device fails here."""
    dev = make(BF16).device.type
    for S in CASES:
        if S not in _count.get((dev, kernel_of(S)), ()):
            try:
                check(make, S)
            except AssertionError as e:
                print(f"[wgrad-family] SUMMARY MISS {str(e)[:200]}")
    for r in REDUCE:
        if (dev, f"reduce-G{r.lanes}") not in _worst:
            body_reduce(make, r, False)
    for b in BIAS:
        if (dev, f"bias-{NAME[b.dtype]}") not in _worst:
            body_bias(make, b, 0)
    want = KERNELS + [f"reduce-G{G}" for G in (1, 2, 4, 8, 16, 32)] + ["bias-bf16", "bias-fp32"]
    for k in want:
        assert (dev, k) in _worst and math.isfinite(_worst[(dev, k)]), f"no figure for {k} on {dev}"
        n = len(_count.get((dev, k), ()))
        print(f"[wgrad-family] SUMMARY {dev} {k}: worst error / bound = {_worst[(dev, k)]:.3g}" + (f" over {n} cases" if n else ""))
    print(f"[wgrad-family] SUMMARY {dev}: {len(CASES)} launch cases, {len(REDUCE) + len(REDUCE_PAST_THE_GRID)} reduction cases, {len(BIAS)} bias cases")
    for (d, what), n in sorted(_excused.items()):
        if d == dev:
            print(f"[wgrad-family] SUMMARY excused footprint {what}: {n} elements")


# ------------------------------------------------------------------------------------------------ refused descriptors
def body_refused(hip_ops, device):
    """Descriptors and arguments the host rejects before any launch: each returns the library's error and the sentinel-filled outputs are
    unchanged.  Nothing here launches a kernel: every mutation fails a check of gan_conv_wgrad, of the kernel's own launcher, of
    gan_wgrad_reduce or of gan_bias_grad that precedes the launch."""
    import ctypes
    lib = hip_ops.lib
    bigs = []

    def planned(g, B):
        ctx = Ctx(None, device, BF16)
        ops = Guarding(hip_ops, ctx, launch=False)
        ctx.ops = ops
        g = Geom(*g)
        Ho, Wo = out_hw(g)
        w = torch.zeros((g.cout, g.cin, g.k, g.k), device=ctx.device)
        gw, gw_big = guarded_f32(ctx, w.numel(), GW_FILL)
        layer = ConvLayer(ctx, w, None, gw.view(w.shape), None, g.k, g.s, g.p, g.tr)
        x, dy = ctx.view(B, g.H, g.W, cpad(g.cin), g.p), ctx.view(B, Ho, Wo, cpad(g.cout), 0)
        layer.wgrad(x, dy, False)
        ops.part.fill_(ST_FILL)
        bigs.extend([(ops.part_big, ST_FILL), (gw_big, GW_FILL)])
        return ops.call, (layer, x, dy, ops)
    c0, keep0 = planned((16, 32, 3, 1, 1, F_, 7, 9), 1)
    c1, keep1 = planned((64, 128, 3, 1, 1, F_, 4, 32), 3)
    c2, keep2 = planned((64, 3, 7, 1, 3, F_, 9, 20), 3)
    assert (c0.variant, c1.variant, c2.variant) == (0, 1, 2)
    cases = [("Cx = 24", c0, dict(Cx=24), b"Cx=24 must be a power of two"),
             ("N = 12", c0, dict(N=12), b"wgrad: N=12"),
             ("N > g_C", c0, dict(N=c0.g.C + 8), b"wgrad: N="),
             ("ntaps = 0", c0, dict(ntaps=0), b"wgrad: ntaps=0"),
             ("ntaps = 129", c0, dict(ntaps=129), b"wgrad: ntaps=129"),
             ("nsplit = 0", c0, dict(nsplit=0), b"nsplit=0"),
             ("x 8 bytes off alignment", c0, dict(x=c0.x.ptr() + 8), b"16-byte aligned"),
             ("M = 100 with nsplit = 3", c0, dict(B=1, Ho=10, Wo=10, nsplit=3), b"leaves empty splits"),
             ("variant 2 with another nsplit", c2, dict(nsplit=c2.nsplit + 1), b"variant 2 needs nsplit"),
             ("variant 1 with an nsplit the planner would not give", c1, dict(nsplit=2 * c1.nsplit), b"wgrad"),
             ("variant 1 on a descriptor that does not qualify", c0, dict(variant=1), b"does not qualify for the range-patch kernel")]
    for what, c, change, msg in cases:
        d = hip_ops._wgrad_desc(c)
        for k, v in change.items():
            setattr(d, k, v)
        rc = lib.gan_conv_wgrad(ctypes.byref(d), None)
        err = lib.gan_last_error()
        assert rc != 0 and msg in err, f"{what}: rc = {rc}, error {err!r}"
    ctx = Ctx(hip_ops, device, BF16)
    part, part_big = guarded_f32(ctx, 4 * 8 * 9 * 8, ST_FILL)
    grad, grad_big = guarded_f32(ctx, 8 * 8 * 9, GW_FILL)
    khw = ctx.i32(K9)
    bigs.extend([(part_big, ST_FILL), (grad_big, GW_FILL)])
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    for what, args, msg in [("Cx % 4 != 0", (p(part), 4, 8, 9, 6, 8, 6), b"Cx must be a multiple of 4"),
                            ("N_real > N", (p(part), 4, 8, 9, 8, 9, 8), b"wgrad_reduce: bad arguments"),
                            ("part 4 bytes off alignment", (p(part, 4), 4, 8, 9, 8, 8, 8), b"16-byte aligned")]:
        rc = lib.gan_wgrad_reduce(*args, 0, 8, 9, p(khw), p(grad), 0, None)
        err = lib.gan_last_error()
        assert rc != 0 and msg in err, f"gan_wgrad_reduce with {what}: rc = {rc}, error {err!r}"
    v = View(torch.zeros(2 * 3 * 3 * 24, dtype=torch.bfloat16, device=ctx.device), 2, 3, 3, 24, 0, BF16)
    ws = ctx.f32(256 * 256, ST_FILL)
    bigs.append((ws, ST_FILL))
    rc = lib.gan_bias_grad(ctypes.byref(v.struct()), 24, p(grad), 0, p(ws), None)
    err = lib.gan_last_error()
    assert rc != 0 and b"C=24" in err, f"gan_bias_grad with C = 24: rc = {rc}, error {err!r}"
    if ctx.device.type == "cuda":
        try:        # the op layer raises the same error as a GanError
            hip_ops.bias_grad(v, 24, grad, False, ws)()
            raise AssertionError("HipOps.bias_grad with C = 24 did not raise")
        except GanError as e:
            assert "C=24" in str(e)
        torch.cuda.synchronize()
    for big, fill in bigs:
        assert bool((big == fill).all()), "a refused call wrote to an output"
    return len(cases) + 4
