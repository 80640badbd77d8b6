"""TEST INFRASTRUCTURE: the cases and assertions for the kernels that MAKE the e4m3 operands and their scales -- gan_quantize_fp8 (unit
scale and per-image amax), gan_quantize_fp8_pow2, the y8 store of gan_in_apply_parts_fp8, gan_in_bwd_amax, gan_weight_scale_batch and the
GAN_FP8 branch of gan_pack_weight_batch.  Every case is written against an op layer: tests/test_fp8_producers_cpu.py runs it on the
emulator's statements, tests/test_fp8_producers_gpu.py on HipOps, with the same shapes and the same assertions.

The byte contract (`check_bytes`).  q = source element / the scale THE PRODUCER ITSELF WROTE, in float64.
  * scale 1 or a power of two: the kernel's v * (1 / scale) is exact in fp32, so the byte equals e4m3_ref.encode(q), no exceptions;
  * otherwise the kernel multiplies by a rounded reciprocal: its fp32 quotient is within 2^-22 relative of q (two roundings of 2^-24,
    doubled), so the byte equals encode(q) except where q lies within 2^-22 |q| of the midpoint of two adjacent codes -- there either
    neighbour is accepted, and the share of such elements is capped (0.1 % per case: the codes are 2^-4 apart at the coarsest, so a
    window of 2^-21 around a midpoint holds ~2^-17 of uniformly spread data).
A `Ref` names the reference the assertions hold a result to; the tests that show that the assertions bite pass a deliberately wrong one.
"""
import numpy as np
import pytest
import torch

from gan_variant_research_amd import BF16, F32, FP8
from tests import e4m3_ref as R
from tests.emulator import EmuOps, _reflect
from tests.norm_ref64 import bwd_ref64, fold64, norm_ref64      # noqa: F401  (the float64 statements live in tests/norm_ref64.py)

REL = 2.0 ** -22
CAP = 1e-3
TDT = {BF16: torch.bfloat16, F32: torch.float32}
NAME = {BF16: "bf16", F32: "fp32"}
EPS = 1e-5
EPS64 = float(np.float32(EPS))          # the float the C ABI receives
FILL8 = 0x55


class Ref:
    encode = staticmethod(R.encode)
    halo_converted = True      # the producers convert / fill the halo
    amax_padded = False        # gan_in_bwd_amax looks at the interior only
    amax_reset = True          # ... and overwrites amax

    def scale_for(self, scale):
        return scale


class Truncating(Ref):
    encode = staticmethod(R.encode_truncate)


class NeighbourScale(Ref):
    def scale_for(self, scale):
        return torch.roll(scale, -1)


class HaloUnconverted(Ref):
    halo_converted = False


class AmaxPadded(Ref):
    amax_padded = True


class AmaxNotReset(Ref):
    amax_reset = False


def sync(ctx):
    if ctx.device.type == "cuda":
        torch.cuda.synchronize()


def ulp32(ref64: torch.Tensor) -> torch.Tensor:
    """spacing of fp32 at |ref| (normal range)"""
    return torch.exp2(torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** -126))) - 23)


def is_pow2(s64: torch.Tensor) -> torch.Tensor:
    return torch.frexp(s64)[0] == 0.5


def interior_mask(v) -> torch.Tensor:
    m = torch.zeros(v.B, v.Hp, v.Wp, v.C, dtype=torch.bool, device=v.t.device)
    m[:, v.halo:v.halo + v.H, v.halo:v.halo + v.W] = True
    return m


def check_bytes(got, q, exact, encode, what, cap=CAP):
    """The byte contract on tensors of one shape; `exact`: bool tensor (broadcastable), True where no exception is allowed.  Returns
    the share of elements of the not-exact part that lie near a midpoint."""
    want = encode(q)
    ok = (got == want) | (R.is_nan_code(got) & R.is_nan_code(want))
    exact = exact.expand_as(ok)
    amb, lo, hi = R.near_midpoint(q, REL)
    amb = amb & ~exact
    ok = ok | (amb & ((got == lo) | (got == hi)))
    n_open = int((~exact).sum())
    share = float(amb.sum()) / n_open if n_open else 0.0
    print(f"[fp8-producers] {what}: {got.numel()} bytes, {int((~ok).sum())} off contract, near-midpoint share {share:.2e} (cap {cap:.0e})")
    if not bool(ok.all()):
        i = int((~ok).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} bytes break the contract; first at flat index {i}: q = "
                             f"{float(q.flatten()[i])!r}, byte {int(got.flatten()[i]):#04x}, expected {int(want.flatten()[i]):#04x}")
    assert share <= cap, f"{what}: {share:.3e} of the elements lie near a midpoint (cap {cap})"
    return share


# ------------------------------------------------------------------------------------------------ a. gan_quantize_fp8, unit scale
def bf16_patterns() -> torch.Tensor:
    """all 65 536 bf16 bit patterns"""
    return (torch.arange(65536) - 32768).to(torch.int16).view(torch.bfloat16)


def fp32_set() -> torch.Tensor:
    """every bf16 pattern as fp32, every midpoint between adjacent codes and its two fp32 neighbours, both signs; 62 x 64 x 16 halo-1 view"""
    mids = R.MIDS.float()
    assert bool((mids.double() == R.MIDS).all())
    near = torch.cat([mids, torch.nextafter(mids, torch.zeros_like(mids)), torch.nextafter(mids, torch.full_like(mids, 1e9))])
    v = torch.cat([bf16_patterns().float(), near, -near])
    out = torch.zeros(64 * 66 * 16)
    out[:v.numel()] = v
    return out


def run_unit(ctx, dtype, vals, shape):
    B, H, W, C, halo = shape
    src, dst = ctx.view(B, H, W, C, halo, dtype=dtype), ctx.view(B, H, W, C, halo, dtype=FP8)
    src.t.copy_(vals.to(ctx.device))
    dst.t.fill_(FILL8)
    ctx.ops.quantize_fp8(src, dst)()
    sync(ctx)
    return {"src": src, "got": dst.padded().clone(), "q": src.padded().double()}


def unit_patterns_case(ctx, dtype):
    return run_unit(ctx, dtype, bf16_patterns() if dtype == BF16 else fp32_set(), (1, 62, 62 if dtype == BF16 else 64, 16, 1))


GRID_SHAPE = (4, 254, 254, 144, 1)      # 2 359 296 sixteen-element chunks > 8192 blocks x 256 threads: a thread converts two


def unit_grid_case(ctx):
    B, H, W, C, halo = GRID_SHAPE
    g = torch.Generator(device=ctx.device).manual_seed(5)
    vals = torch.randn(B * (H + 2) * (W + 2) * C, generator=g, device=ctx.device) * 150.0        # 0.3 % beyond +-448
    return run_unit(ctx, BF16, vals.to(torch.bfloat16), GRID_SHAPE)


def check_unit(res, ref, what, finite_only=True):
    """unit scale: byte-exact, halo included (NaN sources are the subject of check_nan_bytes)"""
    got, q = res["got"], res["q"]
    inner = interior_mask(res["src"])
    sel = ~torch.isnan(q) if finite_only else torch.ones_like(inner)
    if not ref.halo_converted:
        assert bool((got[~inner] == FILL8).all()), f"{what}: halo bytes were written"
        sel = sel & inner
    one = torch.ones((), dtype=torch.bool, device=got.device)
    for i in range(got.shape[0]):          # image by image: bounds the reference's memory
        check_bytes(got[i][sel[i]], q[i][sel[i]], one, ref.encode, f"{what}[{i}]")
    inf = torch.isinf(q) & sel
    assert bool((got[inf] == torch.where(q[inf] > 0, 0x7E, 0xFE).to(torch.uint8)).all()), f"{what}: +-inf must become +-448"


def check_nan_bytes(got, src_is_nan, what):
    assert int(src_is_nan.sum()) > 0
    bad = src_is_nan & ~R.is_nan_code(got)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {int(src_is_nan.sum())} NaN sources became finite bytes, e.g. {int(got[bad][0]):#04x}"
    assert not bool((R.is_nan_code(got) & ~src_is_nan).any()), f"{what}: a finite source became a NaN byte"


# ------------------------------------------------------------------------------------------------ b. gan_quantize_fp8 with amax
AMAX_B = 8
AMAX_SHAPES = [(9, 11, 16, 2), (16, 16, 64, 1)]
POW2_IMAGES = (0, 6)
ZERO_IMAGE, TINY_IMAGE = 4, 7


def amax_mags(dtype):
    """per-image magnitudes, neighbours more than 2x apart.  The last is below 448 * 2^-126 (bf16's smallest subnormal is 2^-133)."""
    return [1.75 * 2.0 ** -3, 0.013, 448.0, 6e4, 0.0, 2.0 ** -20, 1.75 * 2.0 ** 5, 2.0 ** -135 if dtype == F32 else 2.0 ** -130]


def amax_data(dtype, shape, seed=3):
    H, W, C, halo = shape
    B, Hp, Wp = AMAX_B, H + 2 * halo, W + 2 * halo
    g = torch.Generator().manual_seed(seed)
    mags = torch.tensor(amax_mags(dtype), dtype=torch.float64)
    v = torch.randn(B, Hp, Wp, C, generator=g, dtype=torch.float64).clamp(-1, 1) * mags.view(B, 1, 1, 1)
    table = torch.cat([R.MAGS, R.MIDS])
    for b in POW2_IMAGES:       # scale 2^k exactly: every code and every tie between two codes, so a wrong rounding mode shows at once
        idx = torch.randint(0, table.numel(), (Hp, Wp, C), generator=g)
        sgn = torch.randint(0, 2, (Hp, Wp, C), generator=g) * 2.0 - 1.0
        v[b] = table[idx] * sgn * (float(mags[b]) / 448.0)
    peak = (halo + 1, halo + 2, 3)
    for b in range(B):
        v[(b,) + peak] = float(mags[b]) * (1.0 if b % 2 == 0 else -1.0)
    vals = v.to(TDT[dtype])
    # The images with a generic scale.  bf16 values have 8-bit mantissas, so exact ties with the 5-bit midpoints are structural there (amax =
    # 2^-20: q = 7 m 2^n is a midpoint for every m = 3 * 2^k, 1 % of the image).  Such elements are moved away, so that the midpoint
    # exception of the byte contract stays the rare event its cap assumes; test_fp8_producers_cpu checks the share that is left.
    generic = torch.zeros(B, 1, 1, 1, dtype=torch.bool)
    generic[[b for b in range(B) if b not in POW2_IMAGES + (ZERO_IMAGE, TINY_IMAGE)]] = True
    for _ in range(3):
        v64 = vals.double()
        sc = (v64.abs().amax((1, 2, 3)) / 448.0).float().double().clamp_min(2.0 ** -126).view(B, 1, 1, 1)
        tie, _, _ = R.near_midpoint(v64 / sc, 8 * REL)
        tie = tie & generic & (v64.abs() < mags.view(B, 1, 1, 1))
        vals = torch.where(tie, (v64 * 0.9).to(TDT[dtype]), vals)
    return vals, peak


def amax_case(ctx, dtype, shape, vals=None):
    H, W, C, halo = shape
    B = AMAX_B
    peak = None
    if vals is None:
        vals, peak = amax_data(dtype, shape)
    src, dst = ctx.view(B, H, W, C, halo, dtype=dtype), ctx.view(B, H, W, C, halo, dtype=FP8)
    src.padded().copy_(vals.to(ctx.device))
    dst.t.fill_(FILL8)
    amax, scale = ctx.f32(B + 4, 7.25), ctx.f32(B + 4, -3.0)
    amax[:B] = torch.nan_to_num(src.padded().float(), nan=0.0).abs().amax((1, 2, 3))
    ctx.ops.quantize_fp8(src, dst, amax, scale)()
    sync(ctx)
    return {"src": src, "got": dst.padded().clone(), "q": src.padded().double(), "amax": amax.clone(), "scale": scale.clone(), "peak": peak,
            "dtype": dtype}


def check_scale(scale, amax, what):
    """scale_out[b] within one fp32 ulp of float64 amax[b] / 448; exactly 1 for amax == 0 and exactly 2^-126 below 448 * 2^-126"""
    s, a = scale.double().cpu(), amax.double().cpu()
    want = torch.where(a > 0, (a / 448.0).clamp_min(2.0 ** -126), torch.ones_like(a))
    err = (s - want).abs() / ulp32(want)
    print(f"[fp8-producers] {what}: scale {s.tolist()} error in ulp {err.tolist()}")
    assert bool((err <= 1.0).all()), f"{what}: scale off by {err.tolist()} ulp"
    pinned = (a == 0) | (a / 448.0 <= 2.0 ** -126)
    assert bool((s[pinned] == want[pinned]).all()), f"{what}: {s[pinned].tolist()} != {want[pinned].tolist()}"


def check_amax(res, ref, what):
    B = AMAX_B
    got, q0, scale, amax = res["got"], res["q"], res["scale"], res["amax"]
    assert bool((scale[B:] == -3.0).all()) and bool((amax[B:] == 7.25).all()), f"{what}: floats past B were written"
    check_scale(scale[:B], amax[:B], what)
    assert float(scale[ZERO_IMAGE]) == 1.0 and float(scale[TINY_IMAGE]) == 2.0 ** -126
    own = scale[:B].double()
    assert bool(is_pow2(own[list(POW2_IMAGES)]).all()), f"{what}: 1.75 * 2^k / 448 must give a power of two: {own.tolist()}"
    used = ref.scale_for(own)
    q = q0 / used.view(B, 1, 1, 1)
    inner = interior_mask(res["src"])
    sel = torch.ones_like(inner)
    if not ref.halo_converted:
        assert bool((got[~inner] == FILL8).all()), f"{what}: halo bytes were written"
        sel = inner
    exact = is_pow2(used).view(B, 1, 1, 1).expand_as(got)
    check_bytes(got[sel], q[sel], exact[sel], ref.encode, what)           # every image against ITS scale
    peak = res["peak"]
    for b in range(B):
        byte = int(got[(b,) + peak])
        if b == ZERO_IMAGE:
            assert bool(((got[b] & 0x7F) == 0).all()) and byte == 0x00, f"{what}: the zero image holds non-zero bytes"
        elif b != TINY_IMAGE:           # (the tiny image's scale is clamped: its bytes are small, and held to the byte contract above)
            assert byte == (0x7E if b % 2 == 0 else 0xFE), f"{what}: image {b}: +-amax became {byte:#04x}, not +-448"
    assert not bool(R.is_nan_code(got).any())


# ------------------------------------------------------------------------------------------------ c. gan_in_apply_parts_fp8
NORM_SHAPES = [(2, 9, 9, 16, 1), (3, 12, 20, 256, 1), (2, 16, 16, 512, 1), (2, 5, 7, 64, 2)]
APPLY_COMBOS = [(act, res, mode) for act in (0, 1) for res in (False, True) for mode in (2, 0)]      # halo_mode: 2 reflect, 0 none
Y_FILL = 3.0
AMB_CAP_NORM = 5e-3


def _fill_view(v, gen, scale=1.0, shift=0.0, off_ties=False):
    """off_ties: values that are exactly the midpoint of two e4m3 codes (1 in 16 bf16 values) move to the next value of the dtype"""
    t = (torch.randn(v.t.shape, generator=gen) * scale + shift).to(v.t.dtype)
    if off_ties:
        tie, _, _ = R.near_midpoint(t.double(), 0.0)
        bits = t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
        bits += tie.to(bits.dtype)
    v.t.copy_(t.to(v.t.device))


def apply_case(ctx, dtype, shape, act, res, mode, nan_at=None):
    B, H, W, C, halo = shape
    gen = torch.Generator().manual_seed(17 + 2 * act + res)
    ops = ctx.ops
    x = ctx.view(B, H, W, C, 0, dtype=dtype)
    _fill_view(x, gen, 1.5, 0.3)
    r = ctx.view(B, H, W, C, halo, dtype=dtype) if res else None
    if res:
        _fill_view(r, gen, off_ties=True)       # where the ReLU gives 0 the result IS the residual: no structural ties in the bf16 run
        if nan_at is not None:
            r.nhwc()[nan_at] = float("nan")
    nparts = ops.in_partial_count(x)
    parts = ctx.f32(B * nparts * C * 2)
    ops.in_partial(x, parts)()
    out = {"x": x, "r": r, "act": act, "mode": mode, "dtype": dtype}
    for name, with8 in (("plain", False), ("fp8", True)):
        y, stats = ctx.view(B, H, W, C, halo, dtype=dtype), ctx.f32(B * C * 2)
        y.t.fill_(Y_FILL)
        y8 = None
        if with8:
            y8 = ctx.view(B, H, W, C, halo, dtype=FP8)
            y8.t.fill_(FILL8)
        ops.in_apply_parts(x, parts, nparts, EPS, stats, act, r, y, mode, y8=y8)()
        sync(ctx)
        out[name] = (y, stats, y8)
    return out


def apply_delta(res):
    """largest |y - y_ref64| / (1 + |y_ref64|) of an fp32 run"""
    assert res["dtype"] == F32
    ref, _, _ = norm_ref64(res["x"], res["act"], res["r"])
    return float(((res["fp8"][0].nhwc().double() - ref).abs() / (1 + ref.abs())).max())


def check_apply(res, ref, what, delta=None):
    (y0, s0, _), (y, stats, y8) = res["plain"], res["fp8"]
    mode, dtype = res["mode"], res["dtype"]
    # the bf16 / fp32 result is what the same kernel writes without the y8 pointer
    assert torch.equal(y.t.view(torch.int16 if dtype == BF16 else torch.int32), y0.t.view(torch.int16 if dtype == BF16 else torch.int32)), f"{what}: y differs from gan_in_apply_parts'"
    assert torch.equal(stats.view(torch.int32), s0.view(torch.int32)), f"{what}: stats differ from gan_in_apply_parts'"
    got, inner = y8.padded(), interior_mask(y8)
    p = y8.halo
    if mode == 2 and ref.halo_converted:
        ys, xs = _reflect(torch.arange(-p, y8.H + p), y8.H).to(got.device), _reflect(torch.arange(-p, y8.W + p), y8.W).to(got.device)
        assert torch.equal(got, y8.nhwc()[:, ys][:, :, xs]), f"{what}: halo bytes are not the bytes at their reflect pre-images"
        written = torch.ones_like(inner)
    else:
        assert bool((got[~inner] == FILL8).all()), f"{what}: halo bytes were written"
        if mode != 2:
            assert bool((y.padded()[~inner].float() == Y_FILL).all())
        written = inner
    yv = y.padded().double()
    one = torch.ones((), dtype=torch.bool, device=got.device)
    if dtype == F32:        # y IS the value converted
        check_bytes(got[written], yv[written], one, ref.encode, what)
    else:                   # the kernel converts its fp32 value, which the stored bf16 y no longer shows: float64 InstanceNorm, margin delta (1 + |v|)
        v, _, _ = norm_ref64(res["x"], res["act"], res["r"])
        gi = y8.nhwc()
        want = ref.encode(v)
        amb, lo, hi = R.near_midpoint_abs(v, delta * (1 + v.abs()))
        ok = (gi == want) | (R.is_nan_code(gi) & R.is_nan_code(want)) | (amb & ((gi == lo) | (gi == hi)))
        share = float(amb.float().mean())
        print(f"[fp8-producers] {what}: delta {delta:.3e}, {int((~ok).sum())} off contract, near-midpoint share {share:.2e} (cap {AMB_CAP_NORM:.0e})")
        assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} bytes are not encode(float64 InstanceNorm)"
        assert share <= AMB_CAP_NORM, f"{what}: near-midpoint share {share}"
        fin = ~R.is_nan_code(gi) & ~R.is_nan_code(want)
        step = (gi.long() & 0x7F) - (want.long() & 0x7F)
        same_sign = (gi & 0x80) == (want & 0x80)
        assert bool((torch.where(same_sign, step.abs() <= 1, ((gi | want) & 0x7F) == 0) | ~fin).all()), f"{what}: a byte is more than one code off"
    # a y8 chunk at the wrong pixel: the byte is within one e4m3 spacing of the stored y
    fin = written & ~torch.isnan(yv)
    d = (R.decode(got[fin]) - yv[fin].clamp(-448, 448)).abs()
    assert bool((d <= R.spacing(yv[fin])).all()), f"{what}: y8 is not a copy of y (max distance {float(d.max())})"
    check_nan_in_place = torch.isnan(yv) & written
    assert torch.equal(R.is_nan_code(got) & written, check_nan_in_place), f"{what}: NaN in y and NaN bytes in y8 differ"


# ------------------------------------------------------------------------------------------------ d. gan_in_bwd_amax
DX_FILL = 1e6
BWD_COMBOS = [(act, bias) for act in (1, 0) for bias in (True, False)]
BWD_TOL = {F32: 1e-4, BF16: 1e-1}        # 5 x test_instance_norm_twins' (rtol = atol) for dx


def bwd_case(ctx, dtype, shape, act, bias):
    B, H, W, C, halo = shape
    ops = ctx.ops
    gen = torch.Generator().manual_seed(29 + act)
    fold = H >= 2 * halo + 2 and W >= 2 * halo + 2
    x, gy = ctx.view(B, H, W, C, 0, dtype=dtype), ctx.view(B, H, W, C, halo, dtype=dtype)
    _fill_view(x, gen, 1.5, 0.3)
    gy.padded().copy_((torch.randn(B, H + 2 * halo, W + 2 * halo, C, generator=gen) * 0.5
                       * torch.tensor([1.0, 1e-3, 30.0][:B]).view(B, 1, 1, 1)).to(TDT[dtype]).to(ctx.device))      # images of different size
    ws, stats = ctx.f32(B * 96 * C * 2 + B * C * 2), ctx.f32(B * C * 2)
    ops.in_stats(x, EPS, stats, ws)()
    nbp = ops.in_bwd_bias_parts(x)
    out = {"x": x, "gy": gy, "act": act, "fold": fold, "dtype": dtype, "bias": bias}

    def fresh():
        dx = ctx.view(B, H, W, C, halo, dtype=dtype)
        dx.t.fill_(DX_FILL)
        return dx, (ctx.f32(nbp * C, -5.0) if bias else None)
    dx0, bp0 = fresh()
    (ops.in_bwd_bias_deferred(x, stats, act, gy, fold, None, dx0, ws, bp0) if bias else ops.in_bwd(x, stats, act, gy, fold, None, dx0, ws))()
    dx, bp = fresh()
    amax = ctx.f32(B + 3, 9.5)
    op = ops.in_bwd_amax(x, stats, act, gy, fold, dx, ws, bp, amax)
    op()
    sync(ctx)
    out.update(dx0=dx0, bp0=bp0, dx=dx, bp_first=bp.clone() if bias else None, amax=amax.clone(), dx_first=dx.t.clone())
    gy.t.mul_(2.0 ** -6)                 # the same op again on a gradient 64 times smaller: amax is overwritten, not accumulated
    op()
    sync(ctx)
    out.update(amax2=amax.clone(), dx_second=dx.t.clone())
    gy.t.mul_(2.0 ** 6)
    dx8, scale = ctx.view(B, H, W, C, halo, dtype=FP8), ctx.f32(B)
    ops.quantize_fp8(dx, dx8, amax, scale)()
    sync(ctx)
    out.update(dx8=dx8, scale=scale)
    return out


def check_bwd(res, ref, what):
    x, dx, dx0, dtype = res["x"], res["dx"], res["dx0"], res["dtype"]
    B = x.B
    bits = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(res["dx_first"].view(bits), dx0.t.view(bits)), f"{what}: dx differs from the op without amax"
    if res["bias"]:
        assert torch.equal(res["bp_first"].view(torch.int32), res["bp0"].view(torch.int32)), f"{what}: bias_part differs from gan_in_bwd_bias_deferred's"
    inner = interior_mask(dx)
    fill = torch.full((), DX_FILL).to(TDT[dtype])
    first = res["dx_first"].view(B, dx.Hp, dx.Wp, dx.C)
    assert bool((first[~inner] == fill).all()), f"{what}: the halo of dx was written"
    amax, amax2 = res["amax"], res["amax2"]
    assert bool((amax[B:] == 9.5).all()) and bool((amax2[B:] == 9.5).all()), f"{what}: floats past B were written"

    def stored_max(t):
        v = t.view(B, dx.Hp, dx.Wp, dx.C).float()
        if not ref.amax_padded:
            v = v * inner
        return v.abs().amax((1, 2, 3)).double()
    for name, a, t, prev in (("first", amax[:B].double(), res["dx_first"], None), ("second", amax2[:B].double(), res["dx_second"], amax[:B].double())):
        m = stored_max(t)
        if prev is not None and not ref.amax_reset:
            m = torch.maximum(m, prev)
        print(f"[fp8-producers] {what} {name}: amax {a.tolist()} max|dx stored| {m.tolist()}")
        if dtype == F32:
            assert torch.equal(a, m), f"{what} {name} call: amax {a.tolist()} is not max|dx| {m.tolist()}"
        else:       # the maximum before the store's rounding to bf16
            assert bool((m * (1 - 2.0 ** -8) <= a).all()) and bool((a <= m * (1 + 2.0 ** -8)).all()), f"{what} {name} call: amax {a.tolist()} vs max|dx stored| {m.tolist()}"
    if dtype == F32:
        assert torch.equal(amax2[:B], amax[:B] * 2.0 ** -6), f"{what}: a gradient 2^-6 as large must give 2^-6 the amax exactly"
    want = bwd_ref64(x, res["act"], res["gy"], res["fold"]).abs().amax((1, 2, 3))
    tol = BWD_TOL[dtype]
    assert bool(((amax[:B].double() - want).abs() <= tol + tol * want).all()), f"{what}: amax {amax[:B].tolist()} vs float64 {want.tolist()}"
    # chained quantiser (second call's dx and amax)
    b8 = res["dx8"].padded()
    assert not bool(R.is_nan_code(b8).any()), f"{what}: NaN bytes in the e4m3 copy of dx"
    top = ((b8 & 0x7F) * inner).amax((1, 2, 3))
    nz = amax2[:B] > 0
    assert bool((top[nz] == 0x7E).all()), f"{what}: largest interior byte magnitude per image {top.tolist()}, expected 0x7e"
    check_scale(res["scale"], amax2[:B], what)


# ------------------------------------------------------------------------------------------------ e. weight scale + fp8 pack
def weight_descs():
    """(weight [d0][I2][3][3], Nw, ntaps, Cin, N_real, C_real, swap, khw)"""
    g = torch.Generator().manual_seed(41)
    k9, k10 = list(range(9)), list(range(9)) + [-1]
    w0 = torch.randn(256, 256, 3, 3, generator=g) * 0.02
    w1 = torch.randn(128, 256, 3, 3, generator=g) * 0.3
    w2 = torch.zeros(16, 64, 3, 3)
    w3 = torch.randn(100, 60, 3, 3, generator=g).clamp(-2, 2)        # 54 000 elements: no multiple of 1024; rows, channels and one tap padded
    w3.view(-1)[-1] = -2.5
    return [(w0, 256, 9, 256, 256, 256, 0, k9), (w1, 256, 9, 128, 256, 128, 1, k9), (w2, 16, 9, 64, 16, 64, 0, k9), (w3, 112, 10, 64, 100, 60, 0, k10)]


def weights_case(ctx, descs=None):
    ops = ctx.ops
    packs, keep = [], []
    for w, Nw, ntaps, Cin, N_real, C_real, swap, khw in (descs or weight_descs()):
        src = w.to(ctx.device).contiguous()
        dst = torch.full((Nw * ntaps * Cin,), FILL8, dtype=torch.uint8, device=ctx.device)
        scale = ctx.f32(1, -3.0)
        op = ops.pack_weight(src, dst, FP8, Nw, ntaps, Cin, N_real, C_real, swap, w.shape[1], 9, ctx.i32(khw), 1, scale)
        packs.append(op.pack_args)
        keep.append((src, dst, scale, Nw, ntaps, Cin, N_real, C_real, swap, khw))
    ops.pack_weight_batch(packs)()
    sync(ctx)
    return keep


def weight_matrix64(src, Nw, ntaps, Cin, N_real, C_real, swap, khw):
    """[Nw][ntaps][Cin] float64: the operand the copy holds, padding 0"""
    out = torch.zeros(Nw, ntaps, Cin, dtype=torch.float64, device=src.device)
    w = src.double()
    for t, k in enumerate(khw):
        if k >= 0:
            out[:N_real, t, :C_real] = (w[:, :, k // 3, k % 3].t() if swap else w[:, :, k // 3, k % 3])[:N_real, :C_real]
    return out


def check_weights(keep, ref, what):
    for i, (src, dst, scale, Nw, ntaps, Cin, N_real, C_real, swap, khw) in enumerate(keep):
        m = src.double().abs().max()
        check_scale(scale, torch.nan_to_num(m, nan=0.0).view(1), f"{what}[{i}]")
        got = EmuOps._unfrag(dst, Nw, ntaps * Cin // 2, 2).view(Nw, ntaps, Cin)
        wm = weight_matrix64(src, Nw, ntaps, Cin, N_real, C_real, swap, khw)
        s = scale.double()
        check_bytes(got, wm / s, is_pow2(s), ref.encode, f"{what}[{i}]")
        pad = torch.ones(Nw, ntaps, Cin, dtype=torch.bool, device=dst.device)
        pad[:N_real, :len([k for k in khw if k >= 0]), :C_real] = False
        assert bool((got[pad] == 0).all()), f"{what}[{i}]: padded rows / channels / taps are not zero bytes"
        if float(m) == 0:
            assert float(scale) == 1.0 and bool((got == 0).all())
        else:
            top = wm.abs() == m
            assert bool((got[top] == torch.where(wm[top] > 0, 0x7E, 0xFE).to(torch.uint8)).all()), f"{what}[{i}]: the largest element is not +-448"


# ------------------------------------------------------------------------------------------------ f. gan_quantize_fp8_pow2
def pow2_case(ctx, dtype):
    """the inputs of test_basic_fp8_gpu.test_pow2_quantiser_equals_its_emulator_statement"""
    B, H, C_ = 12, 16, 64
    g = torch.Generator().manual_seed(11)
    mag = torch.tensor([1.0, 448.0, 447.0, 449.0, 1.75, 1.7578125, 3e-5, 7e-9, 6e4, 0.0, 2.0 ** -20, 0.013])
    v = torch.randn(B, H + 4, H + 4, C_, generator=g).clamp(-1, 1) * mag.view(B, 1, 1, 1)
    v[:, 3, 3, 0] = mag
    src, dst = ctx.view(B, H, H, C_, 2, dtype=dtype), ctx.view(B, H, H, C_, 2, dtype=FP8)
    src.padded().copy_(v.to(TDT[dtype]).to(ctx.device))
    amax = src.padded().float().abs().amax((1, 2, 3)).contiguous()
    sc = ctx.f32(B)
    ctx.ops.quantize_fp8_pow2(src, dst, amax, sc)()
    sync(ctx)
    return {"src": src, "got": dst.padded().clone(), "q": src.padded().double(), "scale": sc}


def check_pow2(res, ref, what):
    s = ref.scale_for(res["scale"].double())
    assert bool(is_pow2(s).all())
    one = torch.ones((), dtype=torch.bool, device=s.device)
    check_bytes(res["got"], res["q"] / s.view(-1, 1, 1, 1), one, ref.encode, what)


# ------------------------------------------------------------------------------------------------ the test bodies, by op layer
# `make` returns a fresh Ctx on the op layer under test.  Results are kept per (op layer, case), so that the tests which hold a result to
# a deliberately wrong reference launch nothing again.
# The cache lives for the test session and keeps its (small) results on the device; a test that finds no entry runs the case itself, so
# every test passes alone and in any order.
_results = {}


def _cached(make, key, fn):
    ctx = make()
    k = (ctx.device.type,) + key
    if k not in _results:
        _results[k] = fn(ctx)
    return _results[k]


def unit_result(make, dtype):
    return _cached(make, ("unit", dtype), lambda ctx: unit_patterns_case(ctx, dtype))


def amax_result(make, dtype, shape):
    return _cached(make, ("amax", dtype, shape), lambda ctx: amax_case(ctx, dtype, shape))


def apply_result(make, dtype, shape, combo):
    return _cached(make, ("apply", dtype, shape, combo), lambda ctx: apply_case(ctx, dtype, shape, *combo))


def apply_delta_of(make, shape):
    """2 x the largest relative distance between the fp32 run of this shape (all eight variants) and the float64 InstanceNorm: MEASURED on
    the op layer under test, and the margin of the bf16 run of the same shape"""
    d = 2.0 * max(apply_delta(apply_result(make, F32, shape, c)) for c in APPLY_COMBOS)
    print(f"[fp8-producers] in_apply_parts_fp8 {shape}: delta = {d:.3e}")
    return d


def bwd_result(make, dtype, shape, combo):
    return _cached(make, ("bwd", dtype, shape, combo), lambda ctx: bwd_case(ctx, dtype, shape, *combo))


def weights_result(make):
    return _cached(make, ("weights",), weights_case)


def pow2_result(make, dtype):
    return _cached(make, ("pow2", dtype), lambda ctx: pow2_case(ctx, dtype))


def body_unit(make, dtype, ref=Ref()):
    check_unit(unit_result(make, dtype), ref, f"quantize_fp8 unit {NAME[dtype]}")


def body_unit_grid(make, ref=Ref()):
    check_unit(unit_grid_case(make()), ref, "quantize_fp8 unit grid-stride")


def body_amax(make, dtype, shape, ref=Ref()):
    check_amax(amax_result(make, dtype, shape), ref, f"quantize_fp8 amax {NAME[dtype]} {shape}")


def body_apply(make, dtype, shape, ref=Ref(), combos=APPLY_COMBOS):
    delta = apply_delta_of(make, shape) if dtype == BF16 else None
    for combo in combos:
        check_apply(apply_result(make, dtype, shape, combo), ref, f"in_apply_parts_fp8 {NAME[dtype]} {shape} act/res/halo {combo}", delta)


def body_bwd(make, dtype, shape, ref=Ref(), combos=BWD_COMBOS):
    for combo in combos:
        check_bwd(bwd_result(make, dtype, shape, combo), ref, f"in_bwd_amax {NAME[dtype]} {shape} act/bias {combo}")


def body_weights(make, ref=Ref()):
    check_weights(weights_result(make), ref, "fp8 pack")


def body_pow2(make, dtype, ref=Ref()):
    check_pow2(pow2_result(make, dtype), ref, f"quantize_fp8_pow2 {NAME[dtype]}")


def body_nan(make, producer):
    """A NaN source element yields an e4m3 NaN byte (0x7F / 0xFF) from every producer, and nothing else does."""
    ctx = make()
    if producer in ("unit-bf16", "unit-fp32"):
        res = unit_result(make, BF16 if producer == "unit-bf16" else F32)
        check_nan_bytes(res["got"], torch.isnan(res["q"]), producer)
    elif producer in ("amax-bf16", "amax-fp32"):
        dtype = BF16 if producer == "amax-bf16" else F32
        vals, _ = amax_data(dtype, AMAX_SHAPES[0])
        vals[1, 0, 0, 5] = float("nan")             # in the halo of image 1 ...
        vals[3, 4, 5, 6] = float("nan")             # ... and inside image 3
        res = amax_case(ctx, dtype, AMAX_SHAPES[0], vals)
        check_nan_bytes(res["got"], torch.isnan(res["q"]), producer)
        q = res["q"] / res["scale"][:AMAX_B].double().view(-1, 1, 1, 1)
        check_bytes(res["got"], q, is_pow2(res["scale"][:AMAX_B].double()).view(-1, 1, 1, 1), R.encode, producer)
    elif producer in ("y8-bf16", "y8-fp32"):
        dtype = BF16 if producer == "y8-bf16" else F32
        res = apply_case(ctx, dtype, NORM_SHAPES[0], 1, True, 2, nan_at=(1, 1, 3, 7))      # row 1: the reflect halo copies it
        y, _, y8 = res["fp8"]
        assert int(torch.isnan(y.padded().float()).sum()) >= 2
        check_nan_bytes(y8.padded(), torch.isnan(y.padded().float()), producer)
    else:
        assert producer == "pack"
        descs = weight_descs()[3:]
        descs[0][0][7, 5, 1, 2] = float("nan")
        src, dst, scale, Nw, ntaps, Cin, N_real, C_real, swap, khw = weights_case(ctx, descs)[0]
        got = EmuOps._unfrag(dst, Nw, ntaps * Cin // 2, 2).view(Nw, ntaps, Cin)
        assert bool(R.is_nan_code(got[7, 5, 5])), f"pack: the NaN weight became {int(got[7, 5, 5]):#04x}"


def body_tiny_weight(make):
    """max|W| below 448 * 2^-126: the weight scale has gan_quantize_fp8's floor, 2^-126, and the bytes are finite ones on that scale"""
    w = torch.zeros(16, 64, 3, 3)
    w[3, 5, 1, 1], w[9, 60, 2, 0] = 2.0 ** -135, -(2.0 ** -140)
    src, dst, scale, Nw, ntaps, Cin, N_real, C_real, swap, khw = weights_case(make(), [(w, 16, 9, 64, 16, 64, 0, list(range(9)))])[0]
    assert float(scale) == 2.0 ** -126, float(scale)
    got = EmuOps._unfrag(dst, Nw, ntaps * Cin // 2, 2).view(Nw, ntaps, Cin)
    wm = weight_matrix64(src, Nw, ntaps, Cin, N_real, C_real, swap, khw)
    check_bytes(got, wm / scale.double(), is_pow2(scale.double()), R.encode, "fp8 pack, tiny weight")
    assert int(got[3, 4, 5]) == 0x01 and not bool(R.is_nan_code(got).any())          # 2^-135 / 2^-126 = 2^-9, the smallest subnormal


# ------------------------------------------------------------------------------------------------ the assertions bite
WRONG = {
    "unit": [Truncating, HaloUnconverted],
    "amax": [Truncating, NeighbourScale, HaloUnconverted],
    "apply": [Truncating, HaloUnconverted],
    "bwd": [AmaxPadded, AmaxNotReset],
    "weights": [Truncating],
    "pow2": [Truncating, NeighbourScale],
}


def rejects(make, group, wrong, dtype):
    with pytest.raises(AssertionError):
        if group == "unit":
            body_unit(make, dtype, wrong())
        elif group == "amax":
            body_amax(make, dtype, AMAX_SHAPES[0], wrong())
        elif group == "apply":
            body_apply(make, dtype, NORM_SHAPES[0], wrong(), combos=[(1, True, 2)])
        elif group == "bwd":
            body_bwd(make, dtype, NORM_SHAPES[0], wrong(), combos=[(1, True)])
        elif group == "weights":
            body_weights(make, wrong())
        else:
            body_pow2(make, dtype, wrong())
