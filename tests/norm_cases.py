"""TEST INFRASTRUCTURE: cases, derived bounds and assertions for the InstanceNorm kernel family of csrc/norm.hip, written against an op
layer: tests/test_norm_family_cpu.py runs them on the emulator, tests/test_norm_family_gpu.py on HipOps, with the same shapes and the same
assertions.  The float64 statements are in tests/norm_ref64.py.

Bounds (convention of tests/cases.py: BOUND_C, U_BF16, U_F32 = 2^-24 =: u, sqrt(K)); none of them is fitted to a result.

  SUMS.  A kernel adds HW fp32 terms per channel in some order (lanes, row lanes, chunks; the partials are combined in fp64).  As in
  cases.py every partial sum is at most the sum of the absolute terms, and HW independent roundings of 2^-24 of it stay, with the
  BOUND_C margin, below
        dS = BOUND_C sqrt(HW) u sum|x|,     dQ = BOUND_C sqrt(HW) u sum x^2          (x^2 itself is rounded once: inside the margin)
  Hence, with mean = S / HW and var = Q / HW - mean^2 evaluated in fp64 from those sums and stored as floats,
        tol(mean) = dS / HW + u |mean|
        tol(var)  = dQ / HW + 2 |mean| dS / HW + (dS / HW)^2
        rstd in [ (var + tol(var) + eps)^-1/2 (1 - 2u),  (max(var - tol(var), 0) + eps)^-1/2 (1 + 2u) ]
  The interval is the exact image of tol(var); for tol(var) << var + eps it is 1/2 rstd^3 tol(var) + 2u rstd.  THE CONTRACT this states:
  the relative error of the variance grows with kappa = (mean^2 + var) / var, because the kernels evaluate E[x^2] - mean^2 from fp32 sums
  (about 4 sqrt(HW) 2^-24 kappa; torch's float32 instance_norm, which subtracts the mean first, does not have this growth).
  A (image, channel) pair is WELL CONDITIONED if tol(var) <= (var + eps) / 4: `stats_tol` computes that from the reference, and the
  case builder asserts which data classes must satisfy it.  The interval is asserted for every pair; pairs that are not well conditioned
  are additionally held to 0 < rstd <= eps^-1/2 (1 + 2u) and finite.

  APPLY, GIVEN STATS.  v' = (v - mean) * rstd: two fp32 roundings of |xhat|; LeakyReLU: two more of |0.2 xhat| (the constant 0.2f and
  the product); tanh: tanhf within 2 ulp (4u |tanh|) and Lipschitz 1; residual: one rounding of the sum; then the store:
        tol = e + u_out (|ref| + e),      e = u (2 |xhat| [+ 2 |act| | + 4 |act|] [+ |ref|])
  The sign of fl(v - mean) is that of v - mean and rstd > 0, so the ReLU / LeakyReLU branch is the reference's.

  BACKWARD, GIVEN STATS.  dx = fma(g', A, fma(x, Bc, Cc)), A = rstd, Bc = -rstd^2 m2, Cc = -rstd m1 + rstd^2 m2 mean, the coefficients
  computed in fp64 and rounded to float (one rounding of each), then two fma roundings:
        e = 3 u (|g' A| + |x| |Bc|^ + |Cc|^)  +  rstd dm1  +  |xhat| rstd^2 d2  +  (the uncertainty of g', below)
        dm1 = BOUND_C sqrt(HW) u mean|g'|,    d2 = BOUND_C sqrt(HW) u (mean|g' x| + |mean| mean|g'|)     [m2 = rstd (S2 - mean S1) / HW]
        |Bc|^ = rstd^2 (|m2| + rstd d2),   |Cc|^ = rstd (|m1| + dm1) + |mean| |Bc|^
        tol = e + u_out (|ref| + e)
  x Bc and Cc cancel where the data has a mean: this bound, too, grows with |mean| / sigma, as the kernel's expression does.
  g' is not exact where the kernel folds: every pre-image added is rounded to the buffer's dtype in the two-pass backward (bf16: 2^-8 of
  the running sum), and gan_in_bwd with g2 first stores fold(gy) + g2 in dx's dtype: dg = (roundings) x (sum of |terms|), which enters dx
  as rstd (dg + mean dg) + |xhat| rstd mean(dg |xhat|).  gan_in_bwd_parts takes S1, S2 from its caller: dm1 = d2 = 0 there.

  BIAS GRADIENT.  Exactly 0.  The kernel evaluates T1 + T2 + T3 = rstd S1 + Bc (HW mean) + HW Cc in fp64 from float inputs: at most 10
  fp64 roundings in each term (m2 alone: two for S2 - mean S1, times rstd, / HW; rstd^2; products) and two additions:
        |bias_part row of block 0| <= 12 * 2^-53 (|T1| + |T2| + |T3|)  (+ its float rounding), every other row exactly 0,
  with |T1| + |T2| + |T3| <= 2 HW rstd (|m1| + dm1) + 2 HW |mean| |Bc|^ (the kernel's own m1, m2, not the reference's, set the size of the terms),
  and bias_grad (+)= their fp32 sum, in one level or -- B * nblk > 64 rows -- in two (32 segments, then the 32).  THE SUM is held to the
  float64 sum of the rows themselves, which gan_in_bwd_bias_deferred hands out bit for bit (the same kernel writes them):
        |bias_grad - sum rows (- prior)| <= BOUND_C sqrt(nrows) u sum|rows| + u |result|
  (against 0 alone, a sum that dropped or repeated a segment of these ~1e-10 residues would pass).  The emulator states the op as the column sum of the stored dx instead; it is held to the sum of
  the dx tolerances of the column (each stored dx is within its tolerance of values that add up to 0).

  FOLD / ACTIVATION GRADIENT.  fp32 sum of n terms: (n - 1) u sum|terms|; act' from the output y: LeakyReLU 0.2f (u), tanh 1 - y^2 (two
  roundings of 1 + y^2); the product one more; then the store.
"""
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from tests import norm_ref64 as R
from tests.cases import BOUND_C, U_BF16, U_F32

U = U_F32
EPS = R.EPS
EPS64 = R.EPS64
TDT = {BF16: torch.bfloat16, F32: torch.float32}
NAME = {BF16: "bf16", F32: "fp32"}
BITS = {BF16: torch.int16, F32: torch.int32}
U_OUT = {BF16: U_BF16, F32: U_F32}
EPC = {BF16: 8, F32: 4}                 # elements per 16-byte chunk
Y_FILL, DX_FILL, WS_FILL, ST_FILL = 7.5, 2.0 ** 20, 3e5, -9.0            # exact in bf16 and fp32
IMG_SCALE = 2.0 ** 10                   # images differ in size by ~1e3 (a power of two: the constant channel's sums stay exact)

# documented constants of csrc/norm.hip (the library's queries are used where one exists)
NTHR, MAXCH, MAXPARTS, WORK_PER_BLOCK, PART_WORK, LAUNCH_BLOCKS, MAXBLK, BWD_MAXC, SUMS_MAXC = 256, 96, 16, 4096, 2048, 512, 1024, 512, 1024


def cdiv(a, b):
    return -(-a // b)


def geometry(shape, dtype):
    B, H, W, C, halo = shape
    cl, HW = C // EPC[dtype], H * W
    g = {"cl": cl, "RL": NTHR // cl, "HW": HW,
         "nch": max(1, min(MAXCH, cdiv(HW * cl, WORK_PER_BLOCK))),
         "nparts": max(1, min(MAXPARTS, cdiv(LAUNCH_BLOCKS, B), cdiv(HW * cl, PART_WORK))),
         "nblk": max(1, min(MAXBLK, cdiv(HW * cl, WORK_PER_BLOCK)))}
    for k, n in (("ch", g["nch"]), ("pt", g["nparts"])):
        per = cdiv(HW, n)
        g["per_" + k] = per
        g["empty_" + k] = sum(1 for i in range(n) if i * per >= HW)
        g["short_" + k] = sum(1 for i in range(n) if i * per < HW < (i + 1) * per)
    g["rows_per_step"] = g["RL"] // W
    g["two_level"] = B * g["nblk"] > 64
    return g


# shape (B, H, W, C, halo), dtypes, the regime the case names (checked by `check_regime`), backward?, every combination?
Case = namedtuple("Case", "shape dtypes regime bwd full")
CASES = [
    Case((1, 96, 128, 256, 1), (BF16,), dict(nch=96, nparts=16, per_ch=128, empty_ch=0), True, False),
    Case((1, 64, 96, 256, 1), (F32,), dict(nch=96, nparts=16, per_ch=64, empty_ch=0), True, False),
    Case((1, 5, 1229, 256, 0), (F32,), dict(nch=96, per_ch=65, empty_ch=1, short_ch=1), True, False),
    Case((1, 3, 43, 1024, 0), (F32,), dict(nparts=16, per_pt=9, empty_pt=1, cl=256, RL=1), False, False),
    Case((2, 300, 5, 8, 1), (BF16,), dict(cl=1, RL=256, rows_per_step=51, nch=1), True, True),
    # fp32: gan_check_view wants C % 8 == 0 for every dtype, so the narrowest accepted fp32 buffer has two chunk lanes (C = 4 is refused:
    # test_unsupported_widths_return_their_error)
    Case((2, 300, 5, 8, 1), (F32,), dict(cl=2, RL=128, rows_per_step=25, nch=1), True, True),
    Case((2, 4, 4, 64, 1), (BF16, F32), dict(fold_min="HW"), True, True),
    Case((2, 8, 9, 64, 3), (BF16, F32), dict(fold_min="H"), True, True),
    Case((2, 6, 20, 16, 2), (BF16, F32), dict(fold_min="H"), True, True),
    Case((2, 9, 9, 512, 1), (BF16, F32), dict(C=BWD_MAXC), True, False),
    Case((2, 6, 7, 2048, 0), (BF16,), dict(cl=256, RL=1), False, False),
    Case((65, 4, 4, 16, 1), (BF16, F32), dict(two_level=True, nparts=1), True, False),
    # B = 600: ceil(512 / B) = 1 partial per image.  (That cap only BINDS where HW * cl > 2048 as well, i.e. from B * HW * C of about 8 M
    # elements on: beyond the buffers of this suite.  The case holds the count the library reports to the documented formula.)
    Case((600, 3, 3, 16, 0), (BF16, F32), dict(two_level=True, nparts=1, want=1), True, False),
    Case((3, 1, 1, 64, 0), (BF16, F32), dict(HW=1), True, True),
    Case((3, 12, 20, 256, 1), (BF16, F32), dict(), True, True),
]
CASE_IDS = [(i, dt) for i, c in enumerate(CASES) for dt in c.dtypes]


def case_id(p):
    i, dt = p
    return "x".join(map(str, CASES[i].shape)) + "-" + NAME[dt]


def check_regime(ctx, case, dtype, x):
    """the case is in the regime it names: through the library's queries where there is one, else from the documented constants"""
    B, H, W, C, halo = case.shape
    g = geometry(case.shape, dtype)
    if ctx.ops.is_hip:
        assert ctx.ops.in_partial_count(x) == g["nparts"], (ctx.ops.in_partial_count(x), g)
        assert ctx.ops.in_bwd_bias_parts(x) == B * g["nblk"], (ctx.ops.in_bwd_bias_parts(x), g)
    for k, want in case.regime.items():
        if k == "fold_min":
            assert H == 2 * halo + 2 and (W == 2 * halo + 2 if want == "HW" else W > 2 * halo + 2)
        elif k == "C":
            assert C == want
        elif k == "want":
            assert cdiv(LAUNCH_BLOCKS, B) == want
        else:
            assert g[k] == want, f"{case.shape} {NAME[dtype]}: {k} = {g[k]}, the case names {want}"
    return g


# ------------------------------------------------------------------------------------------------ the reference a result is held to
class Ref:
    drop_last_chunk = divisor_padded = unbiased = eps_outside = False                   # statistics
    residual_first = halo_replicate = False                                            # forward apply
    slope = 0.2
    fold_corners, fold_pad_less = True, 0                                              # fold
    m2_unmasked = drop_m2 = ignore_g2 = acc_overwrites = bias_halo = swap_desc = drop_segment = False  # backward


def _wrong(name, **kw):
    return type(name, (Ref,), kw)


WRONG = {
    "stats": [_wrong("LastChunkLeftOut", drop_last_chunk=True), _wrong("PaddedDivisor", divisor_padded=True), _wrong("Unbiased", unbiased=True),
              _wrong("EpsOutsideSqrt", eps_outside=True)],
    "apply": [_wrong("ResidualBeforeAct", residual_first=True), _wrong("ReplicateHalo", halo_replicate=True), _wrong("Slope001", slope=0.01)],
    "fold": [_wrong("NoCorners", fold_corners=False), _wrong("FoldOfPadLess1", fold_pad_less=1)],
    "bwd": [_wrong("M2Unmasked", m2_unmasked=True), _wrong("NoM2Term", drop_m2=True), _wrong("G2Ignored", ignore_g2=True),
            _wrong("AccumulateOverwrites", acc_overwrites=True), _wrong("BiasOverHalo", bias_halo=True), _wrong("SecondDescriptorForFirst", swap_desc=True),
            _wrong("FirstLevelSegmentLeftOut", drop_segment=True)],
}


# ------------------------------------------------------------------------------------------------ data
CLASSES = ["c2^-10", "off+10", "c2^10", "off-100", "c1", "off+100", "c2^3", "off-10"]
WELL = ("off+10", "off-10", "zero", "outlier")      # classes that must be well conditioned (tol(var) <= (var + eps) / 4) at HW > 1


def channel_classes(C):
    cls = [CLASSES[c % 8] for c in range(C)]
    cls[C - 1], cls[C - 2], cls[C - 3] = "zero", "const", "outlier"
    return cls


def make_x(shape, dtype, seed=7):
    """(B, H, W, C) values in the buffer's dtype: centred channels of scale 2^-10 .. 2^10, channels with mean / sigma = +-10 and +-100,
    one constant, one zero and one N(0,1) channel with a single 1e4 outlier (at pixel 0); odd images 2^10 times as large."""
    B, H, W, C, _ = shape
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    for c, k in enumerate(channel_classes(C)):
        if k.startswith("c2^"):
            v[..., c] *= 2.0 ** int(k[3:])
        elif k.startswith("off"):
            v[..., c] += float(k[3:])
        elif k == "zero":
            v[..., c] = 0.0
        elif k == "const":
            v[..., c] = 3.25
        elif k == "outlier" and H * W > 1:
            v[:, 0, 0, c] = 1e4
    v[1::2] *= IMG_SCALE
    if H * W == 1:      # even channels bf16-representable in both dtypes: x^2 is then exact in fp32 and the kernel's var is exactly 0; the odd
        v[..., 0::2] = v[..., 0::2].to(torch.bfloat16).double()      # fp32 channels keep full mantissas: there var is the rounding error of x^2
    return v.to(TDT[dtype])


def make_g(shape, dtype, seed, halo=None):
    """gradient on the padded domain, N(0, 0.5) halo included; with three or more images image 1 is all zero and image 2 is 1e-3 as
    large, with two images image 1 is 1e-3 as large and the upper half of its channels zero"""
    B, H, W, C, h = shape
    h = h if halo is None else halo
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, H + 2 * h, W + 2 * h, C, generator=g, dtype=torch.float64) * 0.5
    if B >= 3:
        v[1] = 0.0
        v[2] *= 1e-3
    elif B == 2:
        v[1] *= 1e-3
        v[1, ..., C // 2:] = 0.0
    return v.to(TDT[dtype])


def new_view(ctx, shape, dtype, vals=None, halo=None, fill=None):
    B, H, W, C, h = shape
    h = h if halo is None else halo
    v = ctx.view(B, H, W, C, h, dtype=dtype)
    if fill is not None:
        v.t.fill_(fill)
    if vals is not None:
        (v.padded() if vals.shape[1] == H + 2 * h else v.nhwc()).copy_(vals.to(ctx.device))
    return v


Geo = namedtuple("Geo", "B H W C halo Hp Wp")


def geo(v):
    """what `interior` and `halo_mask` need of a view, without its device buffer (results are cached for the session)"""
    return Geo(v.B, v.H, v.W, v.C, v.halo, v.Hp, v.Wp)


def sync(ctx):
    if ctx.device.type == "cuda":
        torch.cuda.synchronize()


def interior(t, v):
    """interior of a CPU copy t of view v's padded buffer"""
    return t[:, v.halo:v.halo + v.H, v.halo:v.halo + v.W]


def snap(v):
    """CPU copy of a view's whole padded buffer"""
    return v.padded().detach().cpu().clone()


def halo_mask(v):
    m = torch.ones(v.B, v.Hp, v.Wp, v.C, dtype=torch.bool)
    m[:, v.halo:v.halo + v.H, v.halo:v.halo + v.W] = False
    return m


def ratio(got, ref, tol):
    """max |got - ref| / tol; a zero tolerance admits only an exact match"""
    r = (got.double() - ref).abs() / (tol + 1e-300)
    assert not bool(torch.isnan(r).any()), "NaN in a result or its reference"
    return float(r.max()) if r.numel() else 0.0


_worst = {}


_rejecting = []        # non-empty while `rejects` holds results to a wrong reference: those ratios are not the kernels'


def report(group, dtype, what, r):
    if _rejecting:
        print(f"[norm-family] (against the wrong reference {_rejecting[0]}) {group} {NAME[dtype]} {what}: {r:.3g}")
        return r
    k = (group, NAME[dtype])
    _worst[k] = max(_worst.get(k, 0.0), r)
    print(f"[norm-family] {group:6s} {NAME[dtype]} {what}: error / bound = {r:.3g}   (worst of the group so far {_worst[k]:.3g})")
    return r


# ------------------------------------------------------------------------------------------------ statistics
def stats_tol(v, eps=EPS64, k=None):
    """(mean, var, rstd, tol_mean, tol_var, rstd_lo, rstd_hi, well_conditioned) per (image, channel) from the float64 data v"""
    HW = v.shape[1] * v.shape[2]
    k = BOUND_C * math.sqrt(HW) * U if k is None else k
    S, Q = R.sums64(v)
    mean, var, rstd = R.stats_from_sums64(S, Q, HW, eps)
    dS, dQ = k * v.abs().sum((1, 2)) / HW, k * Q / HW
    tm = dS + U * mean.abs()
    tv = dQ + 2 * mean.abs() * dS + dS * dS
    lo = (1 - 2 * U) / torch.sqrt(var + tv + eps)
    hi = (1 + 2 * U) / torch.sqrt((var - tv).clamp_min(0) + eps)
    return mean, var, rstd, tm, tv, lo, hi, tv <= (var + eps) / 4


def wrong_stats(v, ref, n_chunks, Hp, Wp, eps=EPS64):
    """(mean, rstd) as a deliberately wrong reference states them"""
    B, H, W, C = v.shape
    HW = H * W
    flat = v.reshape(B, HW, C)
    if ref.drop_last_chunk:
        per = cdiv(HW, n_chunks)
        flat = flat[:, :(cdiv(HW, per) - 1) * per]
    S, Q = flat.sum(1), (flat * flat).sum(1)
    div = Hp * Wp if ref.divisor_padded else HW
    mean = S / div
    var = (Q / div - mean * mean).clamp_min(0)
    if ref.unbiased:
        var = var * HW / max(HW - 1, 1)
    return mean, (1.0 / (torch.sqrt(var) + eps) if ref.eps_outside else 1.0 / torch.sqrt(var + eps))


def check_stats(res, ref, what):
    """every producer's (mean, rstd) against float64 sums of the stored x"""
    v, dtype, shape = res["x64"], res["dtype"], res["shape"]
    B, H, W, C, halo = shape
    mean, var, rstd, tm, tv, lo, hi, well = stats_tol(v)
    cls = channel_classes(C)
    if H * W > 1:       # the condition of the bounded group, asserted where the data is meant to be well conditioned
        must = torch.tensor([k in WELL or k.startswith("c2^") or k == "c1" for k in cls])
        assert bool(well[:, must].all()), f"{what}: a channel meant to be well conditioned has tol(var) > (var + eps) / 4"
    up, dn = hi - rstd, rstd - lo            # the interval's two half widths, around whatever the reference states
    if type(ref) is not Ref:
        mean, rstd = wrong_stats(v, ref, res["geom"]["nch"], H + 2 * halo, W + 2 * halo)
    worst = 0.0
    for name, st in res["stats"].items():
        if name == "finalize":
            continue
        st = st.double()
        assert bool(torch.isfinite(st).all()), f"{what} {name}: non-finite statistics"
        gm, gr = st[..., 0], st[..., 1]
        rm = ratio(gm, mean, tm)
        rr = float(torch.where(gr >= rstd, (gr - rstd) / (up + 1e-300), (rstd - gr) / (dn + 1e-300)).max())
        assert bool(((gr > 0) & (gr <= (1 + 2 * U) / math.sqrt(EPS64))).all()), f"{what} {name}: rstd outside (0, eps^-1/2]"
        rel = ((gr - rstd).abs() / rstd)
        print(f"[norm-family] stats  {NAME[dtype]} {what} {name}: mean {rm:.3g}, rstd {rr:.3g} of the bound; rstd relative error: well conditioned "
              f"{float(rel[well].max()) if bool(well.any()) else 0.0:.2e} ({int(well.sum())} pairs), other {float(rel[~well].max()) if bool((~well).any()) else 0.0:.2e} ({int((~well).sum())})")
        worst = max(worst, rm, rr)
        if name == "in_stats" and type(ref) is Ref and H * W > 1:       # the conditioning contract in figures: by data class
            fam = {"centred": lambda k: k.startswith("c2^") or k == "c1", "|mean|/sigma=10": lambda k: k in ("off+10", "off-10"),
                   "|mean|/sigma=100": lambda k: k in ("off+100", "off-100"), "outlier": lambda k: k == "outlier"}
            parts_ = [f"{n_} {float(rel[:, torch.tensor([f(k) for k in cls])].max()):.1e}" for n_, f in fam.items()]
            print(f"[norm-family] kappa  {NAME[dtype]} {what} HW={H * W}: rstd relative error by class: " + ", ".join(parts_))
    # gan_in_finalize: whole-image float totals in, so only the fp64 evaluation and the final roundings are its own
    tot = res["totals"].double()
    fm, fv, fr = R.stats_from_sums64(tot[..., 0], tot[..., 1], H * W)
    ftv = 8 * 2.0 ** -53 * (tot[..., 1] / (H * W) + fm * fm)
    fup = (1 + 2 * U) / torch.sqrt((fv - ftv).clamp_min(0) + EPS64) - fr
    fdn = fr - (1 - 2 * U) / torch.sqrt(fv + ftv + EPS64)
    if type(ref) is not Ref:
        fm, fr = mean, rstd
    st = res["stats"]["finalize"].double()
    gr = st[..., 1]
    rf = max(ratio(st[..., 0], fm, U * fm.abs()), float(torch.where(gr >= fr, (gr - fr) / (fup + 1e-300), (fr - gr) / (fdn + 1e-300)).max()))
    print(f"[norm-family] stats  {NAME[dtype]} {what} finalize: {rf:.3g} of the bound")
    worst = max(worst, rf)
    if H * W == 1 and type(ref) is Ref:
        one = np.float32(1.0) / np.sqrt(np.float32(EPS))
        sq = (v * v)[:, 0, 0]
        exact = sq.float().double() == sq                # x^2 exact in fp32: every bf16 value, and the even channels of the fp32 run
        assert bool(exact[:, 0::2].all()) and (dtype == BF16 or not bool(exact[:, 1::2].all()))
        for name, st in res["stats"].items():
            assert torch.equal(st[..., 0].double(), v[:, 0, 0]), f"{what} {name}: the mean of one pixel is not that pixel"
            assert bool(((st[..., 1].double() - 1 / math.sqrt(EPS64)).abs() <= float(np.spacing(one)))[exact].all()), f"{what} {name}: rstd is not eps^-1/2 to one ulp"
        if dtype == F32:        # the contract's other side: where x^2 is rounded, var is that rounding error and rstd leaves eps^-1/2 (inside the interval)
            off = (res["stats"]["in_stats"][..., 1].double() - 1 / math.sqrt(EPS64)).abs() / (1 / math.sqrt(EPS64))
            print(f"[norm-family] stats  fp32 {what}: HW = 1, x^2 not exact in fp32: rstd up to {float(off[~exact].max()):.3g} (relative) below eps^-1/2")
    report("stats", dtype, what, worst)
    assert worst <= 1.0, f"{what}: statistics at {worst:.3g} of the derived bound"


# ------------------------------------------------------------------------------------------------ forward apply
def apply_tol(v, mean, rstd, act, res, ref, u_out):
    xh = ((v - mean[:, None, None, :]) * rstd[:, None, None, :]).abs()
    e = 2 * U * xh
    if act == R.ACT_LRELU:
        e = e + 2 * U * R.act64(-xh, act).abs()
    elif act == R.ACT_TANH:
        e = e + 4 * U * torch.tanh(xh)
    if res is not None:
        e = e + U * ref.abs()
    return e + u_out * (ref.abs() + e)


def check_apply(res, ref, what):
    v, dtype, r64 = res["x64"], res["dtype"], res["r64"]
    worst, at = 0.0, what
    for (entry, act, with_res, mode), (y, y2, st) in res["apply"].items():
        st = st.double()
        mean, rstd = st[..., 0], st[..., 1]
        rr = r64 if with_res else None
        want = R.apply64(v, mean, rstd, act, rr, ref.slope, ref.residual_first)
        tol = apply_tol(v, mean, rstd, act, rr, R.apply64(v, mean, rstd, act, rr), U_OUT[dtype])
        yv = res["yview"]
        r = ratio(interior(y, yv), want, tol)
        tag = f"{what} {entry} act {act} res {int(with_res)} halo {mode}"
        if r > worst:
            worst, at = r, tag
        assert r <= 1.0, f"{tag}: y at {r:.3g} of the derived bound"
        assert torch.equal(y.view(BITS[dtype]), y2.view(BITS[dtype])), f"{tag}: a repeated call gave other bits"
        hm = halo_mask(yv)
        if mode == R.HALO_REFLECT:
            src = R.halo64(interior(y, yv), yv.halo, R.HALO_REPLICATE if ref.halo_replicate else R.HALO_REFLECT)
            assert torch.equal(y.view(BITS[dtype]), src.contiguous().view(BITS[dtype])), f"{tag}: a halo element is not the value at its reflect pre-image"
        else:
            assert bool((y[hm].float() == Y_FILL).all()), f"{tag}: the halo was written"
        if v.shape[1] * v.shape[2] == 1 and type(ref) is Ref:
            assert torch.equal(interior(y, yv).double(), rr if with_res else torch.zeros_like(v)), f"{tag}: one pixel must give exactly 0 (+ residual)"
    report("apply", dtype, at, worst)


# ------------------------------------------------------------------------------------------------ fold, activation gradient
def check_fold(res, ref, what):
    dtype, p = res["dtype"], res["shape"][4]
    u_out = U_OUT[dtype]
    g, a64, y64s = res["g64"], res["a64"], res["y64"]

    def fold(t, mode=R.HALO_REFLECT):
        return R.fold_full64(t, p, mode, ref.fold_corners, p - ref.fold_pad_less)
    n_r = R.fold_full64(torch.ones_like(g), p)
    worst = 0.0
    for key, (out, out2, ov) in res["fold"].items():
        kind = key[0]
        assert torch.equal(out.view(BITS[dtype]), out2.view(BITS[dtype])), f"{what} {key}: a repeated call gave other bits"
        assert bool((out[halo_mask(ov)].float() == DX_FILL).all()), f"{what} {key}: the halo was written"
        if kind == "pad_fold":
            mode = key[1]
            want, A, n = fold(g, mode), R.fold_full64(g.abs(), p, mode), R.fold_full64(torch.ones_like(g), p, mode)
            tol = n * U * A
            tol = tol + u_out * (want.abs() + tol)
        elif kind == "fold_add":
            with_a, fo = key[1], key[2]
            base = fold(g) if fo else interior(g, res["gview"])
            A = (R.fold_full64(g.abs(), p) if fo else base.abs()) + (a64.abs() if with_a else 0)
            want = base + (a64 if with_a else 0)
            tol = ((n_r if fo else 1) + 1) * U * A
            tol = tol + u_out * (want.abs() + tol)
        else:       # act_bwd: (fold(g) + g2) * act'(y)
            act = key[1]
            y64 = y64s[act]
            d = R.act_grad_from_out64(y64, act)
            s = fold(g) + a64
            want = s * d
            e = (n_r + 1) * U * (R.fold_full64(g.abs(), p) + a64.abs()) * d.abs()
            e = e + s.abs() * U * {R.ACT_NONE: 0, R.ACT_RELU: 0, R.ACT_LRELU: 0.2, R.ACT_TANH: 2 * (1 + y64 * y64)}[act] + U * want.abs()
            tol = e + u_out * (want.abs() + e)
        r = ratio(interior(out, ov), want, tol)
        worst = max(worst, r)
        assert r <= 1.0, f"{what} {key}: at {r:.3g} of the derived bound"
    report("fold", dtype, what, worst)


# ------------------------------------------------------------------------------------------------ backward
def bwd_parts_of(S_terms1, S_terms2, n):
    """float [B][n][C][2] partial sums of the per-pixel terms (B, HW, C), the pixels cut into n pieces of ceil(HW / n) (the last may be
    short or empty)"""
    B, HW, C = S_terms1.shape
    per = cdiv(HW, n)
    out = torch.zeros(B, n, C, 2, dtype=torch.float64)
    for i in range(n):
        out[:, i, :, 0] = S_terms1[:, i * per:(i + 1) * per].sum(1)
        out[:, i, :, 1] = S_terms2[:, i * per:(i + 1) * per].sum(1)
    return out.float()


def bwd_terms(res, act, ref, fold, g2=False, slope=0.2, own_sums=True, parts=None, mode=2):
    """reference dx, its tolerance and the closed-form bias bound for one backward call"""
    v, dtype, st = res["x64"], res["dtype"], res["st64"]
    B, H, W, C, p = res["shape"]
    HW = H * W
    u_T = U_OUT[dtype]
    mean, rstd = st[..., 0], st[..., 1]
    bc = lambda t: t[:, None, None, :]
    gfull = res["g64"]
    if fold:
        gf, Ag = R.fold_full64(gfull, p), R.fold_full64(gfull.abs(), p)
        npre = R.fold_full64(torch.ones_like(gfull), p) - 1
    else:
        gf = interior(gfull, res["gview"]).clone()
        Ag, npre = gf.abs(), torch.zeros_like(gf)
    if g2:
        Ag = Ag + res["a64"].abs()
        dg = (npre + 1) * U * Ag + u_T * (gf + res["a64"]).abs()
        if not ref.ignore_g2:
            gf = gf + res["a64"]
    else:
        dg = npre * u_T * Ag
    gm = R.act_mask64(gf, v, mean, act, slope)
    xh = (v - bc(mean)) * bc(rstd)
    if parts is None:
        S1, S2 = gm.sum((1, 2)), (gm * v).sum((1, 2))
        if ref.m2_unmasked:
            S2 = (gf * v).sum((1, 2))
        k = BOUND_C * math.sqrt(HW) * U
        dm1 = k * gm.abs().mean((1, 2))
        d2 = k * ((gm * v).abs().mean((1, 2)) + mean.abs() * gm.abs().mean((1, 2)))
        m1, m2 = S1 / HW, rstd * (S2 - mean * S1) / HW
    else:
        P = parts.double().sum(1)
        S1, S2 = P[..., 0], P[..., 1]
        m1, m2 = S1 / HW, (S2 / HW if mode == 1 else rstd * (S2 - mean * S1) / HW)
        dm1 = torch.zeros_like(m1)
        d2 = 4 * 2.0 ** -53 * (S2.abs() + (mean * S1).abs()) / HW
    if ref.drop_m2:
        m2 = torch.zeros_like(m2)
    want = R.bwd64(v, mean, rstd, gm, m1, m2)
    Bc = rstd * rstd * (m2.abs() + rstd * d2)
    Cc = rstd * (m1.abs() + dm1) + mean.abs() * Bc
    e = 3 * U * (gm.abs() * bc(rstd) + v.abs() * bc(Bc) + bc(Cc)) + bc(rstd * dm1) + xh.abs() * bc(rstd * rstd * d2)
    e = e + bc(rstd) * (dg + bc(dg.mean((1, 2)))) + xh.abs() * bc(rstd * (dg * xh.abs()).mean((1, 2)))
    tol = e + u_T * (want.abs() + e)
    # the terms as the kernel holds them: its m1, m2 come from ITS sums, which are within dm1 / rstd d2 of the reference's (at HW = 1 the
    # reference's m2 is exactly 0 and the kernel's is the rounding of one fp32 product)
    T = 2 * HW * rstd * (m1.abs() + dm1) + 2 * HW * mean.abs() * Bc
    bias_tol = 12 * 2.0 ** -53 * T * (1 + U) + 2.0 ** -149
    return want, tol, bias_tol


def check_bias_rows(rows, tol_dx, bias_tol, is_hip, nblk, what):
    """rows: [B][nblk or 1][C] bias partials; exact value 0"""
    if is_hip:
        r = ratio(rows[:, 0], torch.zeros_like(bias_tol), bias_tol)
        assert bool((rows[:, 1:] == 0).all()), f"{what}: a bias partial row of a later block is not zero"
    else:
        r = ratio(rows[:, 0], torch.zeros_like(bias_tol), tol_dx.sum((1, 2)) * (1 + BOUND_C * U * math.sqrt(tol_dx.shape[1] * tol_dx.shape[2])))
    assert r <= 1.0, f"{what}: bias partials at {r:.3g} of the bound"
    return r


def check_bwd(res, ref, what):
    dtype, shape = res["dtype"], res["shape"]
    B, H, W, C, p = shape
    worst = wb = 0.0
    dv = res["dxview"]
    hm = halo_mask(dv)
    for key, out in res["bwd"].items():
        entry, act, fold, g2 = key[:4]
        dx, dx2 = out["dx"], out["dx2"]
        tag = f"{what} {key}"
        kw = {}
        if entry == "parts":
            kw = dict(parts=out["parts"], mode=key[4])
        want, tol, bias_tol = bwd_terms(res, act, ref, fold, g2, **kw)
        r = ratio(interior(dx, dv), want, tol)
        worst = max(worst, r)
        assert r <= 1.0, f"{tag}: dx at {r:.3g} of the derived bound"
        assert torch.equal(dx.view(BITS[dtype]), dx2.view(BITS[dtype])), f"{tag}: a repeated call gave other bits"
        assert bool((dx[hm].float() == DX_FILL).all()), f"{tag}: the halo of dx was written"
        if "ws_tail" in out:
            assert bool((out["ws_tail"] == WS_FILL).all()), f"{tag}: floats past the workspace's documented extent were written"
        if "bias_part" in out:
            bp, nbp = out["bias_part"], res["nbp"]
            assert bool((bp[nbp * C:] == ST_FILL).all()), f"{tag}: floats past the bias partials were written"
            rows = bp[:nbp * C].view(B, nbp // B, C).double()
            if ref.bias_halo:
                rows = rows - dx.double().sum((1, 2))[:, None, :] * (torch.arange(nbp // B) == 0).double()[None, :, None]
            wb = max(wb, check_bias_rows(rows, tol, bias_tol, res["is_hip"], nbp // B, tag))
        if "bias_grad" in out:
            n = out["bias_n"]
            prior = out["prior"].double()
            allow = bias_tol.sum(0) * (1 + B * U) if res["is_hip"] else (tol.sum((1, 2)) * (1 + BOUND_C * U * math.sqrt(H * W))).sum(0) * (1 + B * U)
            assert torch.equal(out["dx_acc"].view(BITS[dtype]), dx.view(BITS[dtype])), f"{tag}: the accumulating call wrote another dx (or its halo)"
            # THE SUM ITSELF (one level, or two where B * nblk > 64): bias_grad against the float64 sum of the per-(image, block) rows, which
            # gan_in_bwd_bias_deferred hands out for the same activation and fold -- the same kernel writes them, so they are the summands bit
            # for bit.  fp32 sum of `nrows` terms: BOUND_C sqrt(nrows) u sum|rows|.  (Against 0 alone a dropped segment would pass.)
            rows = res["bwd"][("deferred", act, fold, False)]["bias_part"][:res["nbp"] * C].view(res["nbp"], C).double()
            nrows = rows.shape[0]
            used = rows
            if ref.drop_segment and nrows > 64:          # 32 first-level segments of ceil(nrows / 32) rows: the second one left out
                per = cdiv(nrows, 32)
                used = torch.cat([rows[:per], rows[2 * per:]])
            total, tol_sum = used.sum(0), BOUND_C * math.sqrt(nrows) * U * rows.abs().sum(0)
            for name, base in (("bias_grad_over", None), ("bias_grad_acc", None if ref.acc_overwrites else prior)):
                want_b = total if base is None else total + base
                rs = ratio(out[name].double()[:n], want_b[:n], tol_sum[:n] + U * want_b[:n].abs())
                wb = max(wb, rs)
                print(f"[norm-family] bias   {NAME[dtype]} {tag} {name}: sum of {nrows} rows ({'two levels' if nrows > 64 else 'one level'}) at {rs:.3g} of the bound; "
                      f"|sum| up to {float(total.abs().max()):.2e}, sum|rows| up to {float(rows.abs().sum(0).max()):.2e}")
                assert rs <= 1.0, f"{tag} {name}: the sum of the bias partial rows at {rs:.3g} of the bound"
            for name, base in (("bias_grad_over", torch.zeros(C, dtype=torch.float64)), ("bias_grad_acc", torch.zeros(C, dtype=torch.float64) if ref.acc_overwrites else prior)):
                bg = out[name].double()
                assert bool((out[name][n:] == ST_FILL).all()), f"{tag}: bias_grad[bias_n:] was written"
                rb = ratio(bg[:n], base[:n], allow[:n] + U * base[:n].abs())
                wb = max(wb, rb)
                assert rb <= 1.0, f"{tag} {name}: at {rb:.3g} of the bound"
    report("bwd", dtype, what, worst)
    report("bias", dtype, what, wb)
    # gan_bias_finalize_batch on partials of its own (the norm's are all ~0): two descriptors in one launch
    fb = res.get("finalize_batch")
    if fb is not None:
        descs = fb["descs"]
        for i, (part, nparts, Cc, n_real, acc, prior, got) in enumerate(descs):
            src = descs[1 - i][0] if (ref.swap_desc and i == 0) else part
            flat = src.double().view(-1)
            m = min(nparts, flat.numel() // Cc)
            pv = flat[:m * Cc].view(m, Cc)
            want = pv.sum(0)[:n_real] + (prior[:n_real].double() if acc else 0)
            tolb = BOUND_C * math.sqrt(nparts) * U * part.double().view(-1, Cc)[:nparts].abs().sum(0)[:n_real] + U * want.abs()
            rb = ratio(got[:n_real], want, tolb)
            assert rb <= 1.0, f"{what} bias_finalize_batch descriptor {i}: at {rb:.3g} of the bound"
            assert bool((got[n_real:] == ST_FILL).all()), f"{what} bias_finalize_batch descriptor {i}: grad[N_real:] was written"
            report("bias", dtype, f"{what} finalize_batch[{i}]", rb)


# ------------------------------------------------------------------------------------------------ running a case
ACTS_ALL = (R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU, R.ACT_TANH)


def run_case(ctx, idx, dtype):
    case = CASES[idx]
    shape = case.shape
    B, H, W, C, p = shape
    HW = H * W
    ops = ctx.ops
    xh = 1 if p else 0                                  # x carries a halo of its own, filled with a value that would wreck the sums
    x = new_view(ctx, shape, dtype, halo=xh, fill=3e4)
    x.nhwc().copy_(make_x(shape, dtype).to(ctx.device))
    geom = check_regime(ctx, case, dtype, x)
    res = {"shape": shape, "dtype": dtype, "geom": geom, "is_hip": ops.is_hip, "x64": x.nhwc().detach().cpu().double(), "case": case}
    x64 = res["x64"]

    # ---- producers
    stats = {}
    ws_n = B * MAXCH * C * 2 + B * C * 2
    ws = ctx.f32(ws_n + 64, WS_FILL)
    tail = 64

    def fresh_stats():
        return ctx.f32(B * C * 2 + tail, ST_FILL)

    def cut(st):
        return st[:B * C * 2]

    def take(st, name):
        sync(ctx)
        assert bool((st[B * C * 2:] == ST_FILL).all()), f"{name}: floats past stats[B][C][2] were written"
        return st[:B * C * 2].view(B, C, 2).detach().cpu().clone()
    st_a = fresh_stats()
    ops.in_stats(x, EPS, cut(st_a), ws)()
    stats["in_stats"] = take(st_a, "in_stats")
    assert bool((ws[B * geom["nch"] * C * 2:] == WS_FILL).all()), "in_stats: floats past ws[B][nchunks][C][2] were written"
    st_a2 = fresh_stats()
    ops.in_stats(x, EPS, cut(st_a2), ws)()
    assert torch.equal(take(st_a2, "in_stats").view(torch.int32), stats["in_stats"].view(torch.int32)), "in_stats: a repeated call gave other bits"
    nparts = ops.in_partial_count(x)
    parts = ctx.f32(B * nparts * C * 2 + tail, ST_FILL)
    ops.in_partial(x, parts)()
    st_b = fresh_stats()
    ops.in_stats_from_parts(parts, nparts, B, C, HW, EPS, cut(st_b))()
    stats["partial+from_parts"] = take(st_b, "in_stats_from_parts")
    parts2, st_b2 = ctx.f32(B * nparts * C * 2 + tail, ST_FILL), fresh_stats()
    ops.in_partial(x, parts2)()
    ops.in_stats_from_parts(parts2, nparts, B, C, HW, EPS, cut(st_b2))()
    sync(ctx)
    assert torch.equal(parts2.view(torch.int32), parts.view(torch.int32)), "in_partial: a repeated call gave other bits"
    assert torch.equal(take(st_b2, "in_stats_from_parts").view(torch.int32), stats["partial+from_parts"].view(torch.int32)), "in_stats_from_parts: a repeated call gave other bits"
    assert bool((parts[B * nparts * C * 2:] == ST_FILL).all()), "in_partial: floats past parts[B][nparts][C][2] were written"
    totals = torch.stack(R.sums64(x64), -1).float()                     # [B][C][2] whole-image sums, as a float producer would hand them over
    st_d = fresh_stats()
    st_d[:B * C * 2] = totals.view(-1).to(ctx.device)
    ops.in_finalize(cut(st_d), B * C, HW, EPS)()
    stats["finalize"] = take(st_d, "in_finalize")
    st_d2 = fresh_stats()
    st_d2[:B * C * 2] = totals.view(-1).to(ctx.device)
    ops.in_finalize(cut(st_d2), B * C, HW, EPS)()
    assert torch.equal(take(st_d2, "in_finalize").view(torch.int32), stats["finalize"].view(torch.int32)), "in_finalize: a repeated call gave other bits"
    res["totals"] = totals

    r = new_view(ctx, shape, dtype, make_g(shape, dtype, 11) * 2.0)
    res["r64"] = r.nhwc().detach().cpu().double()
    yv = new_view(ctx, shape, dtype)
    res["yview"] = geo(yv)
    res["apply"] = {}

    def run_apply(entry, act, with_res, mode):
        outs = []
        st = st_a
        for _ in range(2):
            y = new_view(ctx, shape, dtype, fill=Y_FILL)
            if entry == "apply":
                ops.in_apply(x, cut(st_a), act, r if with_res else None, y, mode)()
            else:
                st = fresh_stats()
                ops.in_apply_parts(x, parts, nparts, EPS, cut(st), act, r if with_res else None, y, mode)()
            sync(ctx)
            outs.append(snap(y))
        res["apply"][(entry, act, with_res, mode)] = (outs[0], outs[1], take(st, entry) if entry == "parts" else stats["in_stats"])
        return st
    parts_ok = C <= SUMS_MAXC
    if case.full:
        combos = [(act, wr, mode) for act in ACTS_ALL for wr in (False, True) for mode in (R.HALO_NONE, R.HALO_REFLECT)]
        combos += [(R.ACT_RELU, True, R.HALO_ZERO), (R.ACT_LRELU, False, R.HALO_REPLICATE)]
    else:
        combos = [(R.ACT_RELU, True, R.HALO_REFLECT), (R.ACT_LRELU, False, R.HALO_NONE), (R.ACT_TANH, True, R.HALO_ZERO)]
    for i, (act, wr, mode) in enumerate(combos):
        run_apply("apply", act, wr, mode)
        if parts_ok and (case.full or i < 2) and mode != R.HALO_REPLICATE:
            st_c = run_apply("parts", act, wr, mode)
    if parts_ok:
        stats["apply_parts"] = take(st_c, "in_apply_parts")
    res["stats"] = stats
    res["st64"] = stats["in_stats"].double()
    if not case.bwd:
        return res

    # ---- backward
    gv = new_view(ctx, shape, dtype, make_g(shape, dtype, 13))
    a = new_view(ctx, shape, dtype, make_g(shape, dtype, 17, halo=0), halo=0)
    res.update(gview=geo(gv), g64=snap(gv).double(), a64=a.nhwc().detach().cpu().double())
    can_fold = p >= 1 and H >= 2 * p + 2 and W >= 2 * p + 2
    nbp = ops.in_bwd_bias_parts(x)
    res["nbp"] = nbp
    res["bwd"] = {}
    dxv = new_view(ctx, shape, dtype)
    res["dxview"] = geo(dxv)
    ws_b = B * MAXCH * C * 2 + B * C * 2 + (B * MAXBLK + 32) * C

    def run_bwd(key, make_op, side=None, **extra):
        """the op twice on fresh dx buffers; `side`: a float buffer the op also writes (bias partials, bias_grad), refilled before the
        second call and required to come out with the same bits"""
        outs, sides = [], []
        for _ in range(2):
            dx = new_view(ctx, shape, dtype, fill=DX_FILL)
            if side is not None:
                side.fill_(ST_FILL)
            make_op(dx)()
            sync(ctx)
            outs.append(snap(dx))
            if side is not None:
                sides.append(side.detach().cpu().clone())
        if side is not None:
            assert torch.equal(sides[0].view(torch.int32), sides[1].view(torch.int32)), f"{key}: a repeated call gave other bits in its bias output"
        res["bwd"][key] = dict(dx=outs[0], dx2=outs[1], **extra)
        return res["bwd"][key]
    acts = (R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU) if case.full else (R.ACT_RELU,)
    for act in acts:
        for fo in ((False, True) if (can_fold and case.full) else (can_fold,)):
            wsb = ctx.f32(ws_n + tail, WS_FILL)
            o = run_bwd(("in_bwd", act, fo, False), lambda dx: ops.in_bwd(x, cut(st_a), act, gv, fo, None, dx, wsb))
            o["ws_tail"] = wsb[ws_n:].detach().cpu()
    run_bwd(("in_bwd", R.ACT_RELU, can_fold, True), lambda dx: ops.in_bwd(x, cut(st_a), R.ACT_RELU, gv, can_fold, a, dx, ws))
    # bias: overwrite, then accumulate onto a prior value
    bias_n = C - 3
    wsb = ctx.f32(ws_b + tail, WS_FILL)
    bg = ctx.f32(C, ST_FILL)
    o = run_bwd(("in_bwd_bias", R.ACT_LRELU, can_fold, False), lambda dx: ops.in_bwd_bias(x, cut(st_a), R.ACT_LRELU, gv, can_fold, None, dx, wsb, bg[:bias_n], bias_n, False), side=bg)
    o.update(bias_grad=True, bias_n=bias_n, bias_grad_over=bg.detach().cpu().clone(), ws_tail=wsb[ws_b:].detach().cpu())
    prior = torch.linspace(-5.0, 5.0, C)
    bg[:bias_n] = prior[:bias_n].to(ctx.device)
    dx_acc = new_view(ctx, shape, dtype, fill=DX_FILL)
    ops.in_bwd_bias(x, cut(st_a), R.ACT_LRELU, gv, can_fold, None, dx_acc, wsb, bg[:bias_n], bias_n, True)()
    sync(ctx)
    o.update(prior=prior, bias_grad_acc=bg.detach().cpu().clone(), dx_acc=snap(dx_acc))
    # deferred bias partials (LeakyReLU: the rows gan_in_bwd_bias above summed -- the same kernel writes them)
    for act in ((R.ACT_LRELU, R.ACT_RELU, R.ACT_NONE) if case.full else (R.ACT_LRELU, R.ACT_RELU)):
        bp = ctx.f32(nbp * C + tail, ST_FILL)
        o = run_bwd(("deferred", act, can_fold, False), lambda dx: ops.in_bwd_bias_deferred(x, cut(st_a), act, gv, can_fold, None, dx, ws, bp), side=bp)
        o["bias_part"] = bp.detach().cpu().clone()
    # the apply half alone, on partial sums made here
    if C <= BWD_MAXC:
        for mode, act, n in ([(2, R.ACT_LRELU, 1), (2, R.ACT_RELU, 4), (2, R.ACT_NONE, MAXCH), (1, R.ACT_RELU, 5)] if case.full else [(2, R.ACT_RELU, MAXCH)]):
            st = res["st64"]
            gf = R.fold_full64(res["g64"], p) if can_fold else interior(res["g64"], gv)
            gm = R.act_mask64(gf, x64, st[..., 0], act)
            second = x64 if mode == 2 else (x64 - st[:, None, None, :, 0]) * st[:, None, None, :, 1]
            pt = bwd_parts_of(gm.reshape(B, HW, C), (gm * second).reshape(B, HW, C), n)
            ptd = pt.to(ctx.device).contiguous().view(-1)
            bp = ctx.f32(nbp * C + tail, ST_FILL)
            o = run_bwd(("parts", act, can_fold, False, mode, n), lambda dx: ops.in_bwd_parts(x, cut(st_a), act, gv, can_fold, dx, ptd, n, mode, bp), side=bp)
            o.update(parts=pt, bias_part=bp.detach().cpu().clone())
    if case.full or res["geom"]["two_level"]:
        g = torch.Generator().manual_seed(23)
        d = []
        for nparts_, Cc, n_real, acc in ((B * geom["nblk"] + 3, C, C, False), (200, 40, 37, True)):
            part = torch.randn(nparts_ * Cc, generator=g)
            prior = torch.randn(Cc, generator=g)
            grad = ctx.f32(Cc, ST_FILL)
            grad[:n_real] = prior[:n_real].to(ctx.device)
            d.append([part, nparts_, Cc, n_real, acc, prior, grad, part.to(ctx.device)])
        ops.bias_finalize_batch([(e[7], e[1], e[2], e[6][:e[3]], e[3], e[4]) for e in d])()
        sync(ctx)
        res["finalize_batch"] = {"descs": [(e[0], e[1], e[2], e[3], e[4], e[5], e[6].detach().cpu().double()) for e in d]}

    # ---- fold, padding gradient, activation gradient
    res["fold"] = {}
    res["y64"] = {}

    def run_fold(key, make_op, ov_halo):
        outs = []
        for _ in range(2):
            out = new_view(ctx, shape, dtype, halo=ov_halo, fill=DX_FILL)
            make_op(out)()
            sync(ctx)
            outs.append(snap(out))
        res["fold"][key] = (outs[0], outs[1], geo(out))
    if p >= 1:
        run_fold(("pad_fold", R.HALO_REPLICATE), lambda out: ops.pad_fold(gv, R.HALO_REPLICATE, out), 0)
        if p < H and p < W:
            run_fold(("pad_fold", R.HALO_REFLECT), lambda out: ops.pad_fold(gv, R.HALO_REFLECT, out), p)
    for with_a in (False, True):
        for fo in ((False, True) if can_fold else (False,)):
            run_fold(("fold_add", with_a, fo), lambda out: ops.fold_add(a if with_a else None, gv, fo, out), p)
    if can_fold:
        for act in (ACTS_ALL if case.full else (R.ACT_TANH,)):
            yk = res["apply"].get(("apply", act, False, R.HALO_NONE))
            yact = new_view(ctx, shape, dtype, (make_g(shape, dtype, 19, halo=0).double() * 1.5).tanh().to(TDT[dtype]) if yk is None else interior(yk[0], yv), halo=0)
            res["y64"][act] = yact.nhwc().detach().cpu().double()
            run_fold(("act_bwd", act), lambda out: ops.act_bwd(yact, act, gv, True, a, out), p)
    return res


_results = {}


def result(make, idx, dtype):
    ctx = make()
    k = (ctx.device.type, idx, dtype)
    if k not in _results:
        _results[k] = run_case(ctx, idx, dtype)
    return _results[k]


GROUPS = {"stats": check_stats, "apply": check_apply, "bwd": check_bwd, "fold": check_fold}


def body(make, group, idx, dtype, ref=None):
    res = result(make, idx, dtype)
    what = case_id((idx, dtype))
    if group in ("bwd", "fold") and group not in res:
        assert not CASES[idx].bwd
        return False
    if group == "fold" and not res["fold"]:
        return False
    GROUPS[group](res, ref or Ref(), what)
    return True


# the cases a wrong reference is tried on (small ones; the statistics also on the 96-chunk case, where a chunk is 1 % of the image)
REJECT_ON = {"stats": [((1, 96, 128, 256, 1), BF16), ((2, 300, 5, 8, 1), BF16), ((2, 6, 20, 16, 2), F32), ((3, 12, 20, 256, 1), F32)],
             "apply": [((2, 8, 9, 64, 3), BF16), ((3, 12, 20, 256, 1), F32)],
             "fold": [((2, 8, 9, 64, 3), BF16), ((2, 6, 20, 16, 2), F32)],
             "bwd": [((2, 8, 9, 64, 3), F32), ((3, 12, 20, 256, 1), BF16), ((65, 4, 4, 16, 1), F32), ((600, 3, 3, 16, 0), BF16)]}


def case_index(shape, dtype):
    hits = [i for i, c in enumerate(CASES) if c.shape == shape and dtype in c.dtypes]
    assert len(hits) == 1, f"{shape} {NAME[dtype]} names {len(hits)} cases"
    return hits[0]


def rejects(make, group, wrong):
    """the wrong reference fails the group's assertions on at least one of the group's cases"""
    failed = []
    _rejecting.append(wrong.__name__)
    try:
        for shape, dtype in REJECT_ON[group]:
            idx = case_index(shape, dtype)
            try:
                body(make, group, idx, dtype, wrong())
            except AssertionError as e:
                failed.append((case_id((idx, dtype)), str(e)[:120]))
    finally:
        _rejecting.clear()
    print(f"[norm-family] {group}: {wrong.__name__} rejected on {failed}")
    assert failed, f"{group}: the assertions accept the wrong reference {wrong.__name__} on every case tried"


# ------------------------------------------------------------------------------------------------ unsupported widths
def body_unsupported(make):
    """C = 2048 bf16 is the widest buffer the forward passes take; gan_in_apply_parts stops at 1024 channels and the backward at 512;
    fp32 C = 4 is no view at all.  Each returns its error; nothing is launched."""
    ctx = make()
    from gan_variant_research_amd._lib import GanError
    import ctypes
    from gan_variant_research_amd._lib import GanView
    with pytest.raises(AssertionError):
        ctx.view(2, 3, 3, 4, 0, dtype=F32)
    buf = ctx.f32(2 * 3 * 3 * 4)
    narrow = GanView(buf.data_ptr(), 2, 3, 3, 4, 0, 0, 3, 3, F32, 0)
    assert ctx.ops.lib.gan_in_partial_count(ctypes.byref(narrow)) < 0 and b"C=4" in ctx.ops.lib.gan_last_error()
    shape = (2, 6, 7, 2048, 0)
    x, y, gy = (new_view(ctx, shape, BF16) for _ in range(3))
    st, ws, parts = ctx.f32(2 * 2048 * 2), ctx.f32(2 * MAXCH * 2048 * 2 + 2 * 2048 * 2), ctx.f32(2 * 16 * 2048 * 2)
    for what, op in (("in_apply_parts", lambda: ctx.ops.in_apply_parts(x, parts, 1, EPS, st, 0, None, y, 0)),
                     ("in_bwd", lambda: ctx.ops.in_bwd(x, st, 0, gy, False, None, y, ws)),
                     ("in_bwd_parts", lambda: ctx.ops.in_bwd_parts(x, st, 0, gy, False, y, parts, 1, 2))):
        with pytest.raises(GanError, match="C=2048"):
            op()()


# ------------------------------------------------------------------------------------------------ the known limit
LIMIT_SHAPES = [(2, 32, 32, 16, 0), (1, 64, 64, 8, 0), (1, 256, 256, 8, 0)]


def body_limit(make, shape, dtype):
    """mean / sigma = 1000 / 1 and 30 / 0.1: outside the well-conditioned range.  Only: rstd finite, in (0, eps^-1/2 (1 + 2u)], and inside
    the interval of the contract.  The errors are printed beside torch's float32 instance_norm's on the same data."""
    ctx = make()
    B, H, W, C, _ = shape
    g = torch.Generator().manual_seed(31)
    v = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    v[..., 0::2] = v[..., 0::2] + 1000.0
    v[..., 1::2] = v[..., 1::2] * 0.1 + 30.0
    x = new_view(ctx, shape, dtype, v.to(TDT[dtype]))
    x64 = x.nhwc().detach().cpu().double()
    st = ctx.f32(B * C * 2)
    ctx.ops.in_stats(x, EPS, st, ctx.f32(B * MAXCH * C * 2))()
    sync(ctx)
    got = st.view(B, C, 2).detach().cpu().double()
    mean, var, rstd, tm, tv, lo, hi, well = stats_tol(x64)
    xt = x64.float().permute(0, 3, 1, 2)
    yt = torch.nn.functional.instance_norm(xt, eps=EPS)
    rt = (yt.double().flatten(2).std(2, unbiased=False) / x64.permute(0, 3, 1, 2).flatten(2).std(2, unbiased=False))       # the rstd torch applied
    gr = got[..., 1]
    for j, name in ((0, "1000/1"), (1, "30/0.1")):
        print(f"[norm-family] limit  {NAME[dtype]} {shape} mean/sigma {name}: rstd relative error {float(((gr - rstd).abs() / rstd)[:, j::2].max()):.3e} "
              f"(torch float32 instance_norm: {float(((rt - rstd).abs() / rstd)[:, j::2].max()):.3e}; contract interval [{float(((lo - rstd) / rstd)[:, j::2].min()):.2e}, "
              f"{float(((hi - rstd) / rstd)[:, j::2].max()):.2e}]; well conditioned: {bool(well[:, j::2].all())})")
    assert bool(torch.isfinite(got).all())
    assert bool(((gr > 0) & (gr <= (1 + 2 * U) / math.sqrt(EPS64))).all())
    assert bool(((gr >= lo) & (gr <= hi)).all()), "rstd outside the interval the conditioning contract allows"
    assert ratio(got[..., 0], mean, tm) <= 1.0


# ------------------------------------------------------------------------------------------------ non-finite data (apply group)
def body_nan_plane(make, dtype):
    """One NaN in x makes the mean and xhat of its (image, channel) NaN: that whole plane of y -- reflect halo included -- is NaN for every
    activation (ReLU keeps a NaN, as torch.relu does; it never writes 0 over the plane), with and without a residual, through gan_in_apply
    and gan_in_apply_parts; every other plane is bit-identical to the clean run."""
    ctx = make()
    shape = (3, 6, 7, 16, 1)
    B, H, W, C, p = shape
    ops = ctx.ops
    vals = make_x(shape, dtype)
    bad = vals.clone()
    bad[1, 1, 2, 5] = float("nan")
    r = new_view(ctx, shape, dtype, make_g(shape, dtype, 11) * 2.0)
    plane = torch.zeros(B, H + 2 * p, W + 2 * p, C, dtype=torch.bool)
    plane[1, :, :, 5] = True
    planes = 0
    for act in ACTS_ALL:
        for with_res in (False, True):
            for entry in ("apply", "parts"):
                outs = []
                for data in (vals, bad):
                    x = new_view(ctx, shape, dtype, halo=0)
                    x.nhwc().copy_(data.to(ctx.device))
                    y = new_view(ctx, shape, dtype, fill=Y_FILL)
                    st = ctx.f32(B * C * 2, ST_FILL)
                    if entry == "apply":
                        ops.in_stats(x, EPS, st, ctx.f32(B * MAXCH * C * 2 + B * C * 2, WS_FILL))()
                        ops.in_apply(x, st, act, r if with_res else None, y, R.HALO_REFLECT)()
                    else:
                        nparts = ops.in_partial_count(x)
                        parts = ctx.f32(B * nparts * C * 2, ST_FILL)
                        ops.in_partial(x, parts)()
                        ops.in_apply_parts(x, parts, nparts, EPS, st, act, r if with_res else None, y, R.HALO_REFLECT)()
                    sync(ctx)
                    outs.append(snap(y))
                clean, got = outs
                what = f"{entry} act {act} residual {with_res} {NAME[dtype]}"
                assert bool(torch.isfinite(clean.float()).all()), what
                assert bool(torch.isnan(got.float())[plane].all()), f"{what}: the plane of the NaN is not NaN everywhere ({int((~torch.isnan(got.float())[plane]).sum())} finite elements)"
                assert torch.equal(got.view(BITS[dtype])[~plane], clean.view(BITS[dtype])[~plane]), f"{what}: a plane without a NaN differs from the clean run"
                planes += 1
    print(f"[norm-family] apply  {NAME[dtype]} NaN plane: {planes} launches, the poisoned plane NaN, all others bit-identical")
    return planes
