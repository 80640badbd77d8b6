"""TEST INFRASTRUCTURE: cases, derived bounds and assertions for the loss, augmentation, pooling and layout kernels (all of
csrc/pointwise.hip; gan_nchw_to_view, gan_view_to_nchw and gan_view_copy of csrc/norm.hip), written against an op layer:
tests/test_pointwise_family_cpu.py runs them on the emulator, tests/test_pointwise_family_gpu.py on HipOps, with the same shapes and the
same assertions.  The float64 statements are in tests/pointwise_ref64.py.

Bounds (convention of tests/cases.py: BOUND_C, U_BF16, U_F32 = 2^-24 =: u, sqrt(K)); none of them is fitted to a result.  Inputs are the
stored bf16 / fp32 values, read exactly, and the scalar arguments are the floats the C ABI receives.

  SUM of K fp32 terms, in any order:  k(K) sum|terms|,  k(K) = BOUND_C sqrt(K) u.  Where a kernel documents its order the worst case of
  that order is used if it is smaller: every addition errs by at most u of its own partial sum, the partial sums of one level of the
  order add up to at most sum|terms|, so D levels err by at most D u sum|terms| (x 1.01 for the second order).  The loss kernels' levels:
  a thread's own trips x C summands in order, the wave's butterfly (6), the block's waves in order (4 of 256 threads, 16 of 1024), and for
  L1 / R1 the 512 block partials in the second launch: 2 per thread, 6, 4.   ks(K, D) = min(k(K), 1.01 D u).
  ELEMENTWISE CHAIN.  `Fl` carries a float64 value with a bound on the error of its fp32 evaluation: every +, -, * adds u of the magnitude
  of ITS OWN result to the propagated errors of its operands (a product also eta = 2^-126: it may underflow).  The kernel's expression is
  replayed operation by operation, so a line that cancels about a mean -- (s - mu) * con + mu -- is charged on |s - mu| and |mu|, and the
  error of mu itself (the image sum: k(C H W) mean|x|, the product with 1 / n, the brightness) passes through with the factor |1 - con|
  ... |1 + con|.  THE CONTRACT this states: the contrast line errs by about 4 sqrt(C H W) 2^-24 |image mean|, whatever the spread, so
  relative to the spread it grows with |mean| / spread (the `mean100` case runs images whose mean is 100 times their spread).
  An fma in place of a product and a sum only removes a rounding.
  STORE.  u_out (|ref| + e) on top of the fp32 error e.
  COPIES.  The layout kernels, and everything else that only moves or zeroes values, are exact: bit equality with the float64 value
  rounded once to the destination type.
  AVGPOOL FORWARD.  cnt <= 9 taps: cnt - 1 additions of at most sum|taps|, one division:  e = (cnt - 1) u sum|taps| / cnt + u |ref|.
  AVGPOOL TRANSPOSE.  m <= 4 terms gy * fl(1 / cnt) (the reciprocal and the product round: 2u each), added in fp32 onto 0 or the prior:
        e = 2u sum|terms| + m u (|prior| + sum|terms|) + eta.
  LOSS SCALARS.  The summands are fp32 functions of exact inputs, e_f each (below); their sum of n terms; then * fl(scale / n):
        tol(loss) = |scale| / n (sum e_f + k(n) sum|f|) + 3u |loss| + eta          -- the same for bf16 and fp32 logits.
    hinge: 1 -+ v rounds once (e_f = u |1 -+ v|); -v exact; (v - t)^2: 3u f; L1 |x - t|: u |x - t|; R1 g^2: u g^2 for fp32 g and
    exact for bf16 g (the square of an 8-bit significand has 16 bits).
    BCE: ex = expf(-|v|) and log1pf within 2 ulp of their values (4u relative, the allowance norm_cases gives tanhf; + eta where they
    underflow), log1p 1-Lipschitz:  e_l = 4u ex + 4u l + 2 eta;  v * t, the difference and the sum round once each.
  GRADIENTS.  f' is exact for the hinges and -mean (+-1, 0), u |f'| for 2 (v - t), and for the sigmoid 1 / (1 + expf(-v)):
  6u sig + eta (expf 4u of ex, and ex / (1 + ex) < 1; the sum; the division; expf(-v) = Inf gives 0 for a value below eta), then - t.
  The factor fl(scale / n) (and * *dev_grad_scale, and scale * 2 / B) and the product: 2u |g| + eta, then the store.

What the header leaves unspecified -- the gradient of a NaN or Inf element -- is not compared.
"""
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from tests import pointwise_ref64 as R
from tests.cases import BOUND_C, U_BF16, U_F32

U = U_F32
ETA = 2.0 ** -126
TDT = {BF16: torch.bfloat16, F32: torch.float32}
NAME = {BF16: "bf16", F32: "fp32"}
BITS = {BF16: torch.int16, F32: torch.int32}
U_OUT = {BF16: U_BF16, F32: U_F32}
EPC = {BF16: 8, F32: 4}
SENT, WS_FILL, JUNK, LOSS_PRIOR = 7.5, 3e5, 2.0 ** 15, 3.25       # exact in bf16 and fp32 (WS_FILL: an fp32 workspace)
GUARD = 64                                                        # floats allocated past a workspace's documented extent
SCALE, DEV_SCALE, TARGET3 = 0.7, 0.3, 0.3                         # none a power of two
NONE, REFLECT, REPLICATE = R.HALO_NONE, R.HALO_REFLECT, R.HALO_REPLICATE
NAN, INF = float("nan"), float("inf")

# documented constants of csrc/pointwise.hip and the layout entry points
ONE_BLOCK, L1_THREADS, GRID_CAP, L1_WS = 1024, 512 * 256, 4096 * 256, 512


def k(n):
    return BOUND_C * math.sqrt(n) * U


def ks(n, depth):
    """bound factor of an fp32 sum of n terms added in an order of `depth` levels (module docstring: SUM)"""
    return min(k(n), 1.01 * depth * U)


def t32(v):
    return float(np.float32(v))


def trips(total, threads):
    """trips of the grid-stride loop taken by the busiest thread"""
    return -(-total // threads)


class Fl:
    """a float64 value and a bound on the error of its fp32 evaluation (module docstring: ELEMENTWISE CHAIN)"""

    def __init__(self, v, e=None):
        self.v = v if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else e

    @classmethod
    def of(cls, a):          # results take the class of the left operand, so a subclass (tests/optim_cases.py: E) keeps its operations
        return a if isinstance(a, Fl) else cls(a)

    def __add__(self, o):
        o = self.of(o)
        v = self.v + o.v
        return type(self)(v, self.e + o.e + U * v.abs())

    def __sub__(self, o):
        o = self.of(o)
        v = self.v - o.v
        return type(self)(v, self.e + o.e + U * v.abs())

    def __rsub__(self, o):
        return self.of(o) - self

    def __mul__(self, o):
        o = self.of(o)
        v = self.v * o.v
        return type(self)(v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e + U * v.abs() + ETA)

    __radd__, __rmul__ = __add__, __mul__

    def stored(self, dtype):
        return self.e + U_OUT[dtype] * (self.v.abs() + self.e)


def channel_mean(t):
    """mc = (t_0 + ... + t_{C-1}) / (float)C: C - 1 additions and a division"""
    C = t.v.shape[3]
    m = t.v.sum(3, keepdim=True) / C
    return Fl(m, t.e.sum(3, keepdim=True) / C + (C - 1) * U * t.v.abs().sum(3, keepdim=True) / C + U * m.abs())


# ------------------------------------------------------------------------------------------------ cases
Case = namedtuple("Case", "group shape dtype opt")
DTYPES = (BF16, F32)
PATCH_VARIANTS = [(0, 0.0), (1, 0.0), (2, 0.0), (3, TARGET3), (4, 0.0), (4, 1.0)]           # (mode, target)
PATCH_SHAPES = [((1, 1, 1), 0, 0), ((3, 6, 6), 1, 2), ((1, 32, 32), 0, 2), ((3, 19, 19), 1, 0), ((2, 70, 70), 1, 2)]      # shape, logits halo, grad halo
LOSS_SHAPES = [(1, 1, 1), (3, 24, 24), (2, 256, 256), (2, 256, 257)]
AUG_SIZES = [(1, 1), (24, 24), (33, 31), (32, 32), (33, 32)]
AUG_BIG = (2, 725, 725)
POOL_SIZES = [(1, 1), (1, 2), (2, 1), (3, 3), (7, 2), (24, 24), (25, 31)]
POOL_BIG = {BF16: ((2, 513, 513), 64), F32: ((2, 513, 513), 32)}
# (B, H, W), halo, mode of nchw_to_view, mode of view_copy
LAYOUT_GEOMS = [((2, 5, 7), 0, NONE, NONE), ((2, 5, 7), 2, NONE, NONE), ((3, 24, 24), 1, REFLECT, REFLECT), ((2, 4, 5), 3, REFLECT, REFLECT),
                ((2, 1, 4), 3, REPLICATE, NONE)]
LAYOUT_BIG = ((2, 420, 420), 0, NONE, NONE)
NF_CLASSES = ("nan", "pinf", "ninf", "unread")


def _cases():
    out = []
    for dt in DTYPES:
        for shape, lh, gh in PATCH_SHAPES:
            out.append(Case("patch", shape, dt, (lh, gh, "plain")))
        for cls in NF_CLASSES:
            out.append(Case("patch", (3, 6, 6), dt, (1, 2, cls)))
        for shape in LOSS_SHAPES:
            for Cr in (1, 3, 4):
                out += [Case("l1", shape, dt, (Cr, "plain")), Case("r1", shape, dt, (Cr, "plain"))]
        for cls in NF_CLASSES:
            out += [Case("l1", (3, 24, 24), dt, (3, cls)), Case("r1", (3, 24, 24), dt, (3, cls))]
        for H, W in AUG_SIZES:
            for Cr in (1, 3):
                for yh in (1, 0):
                    out.append(Case("aug", (10, H, W), dt, (Cr, yh, "plain")))
        out += [Case("aug", (10, 24, 24), dt, (3, 1, "mean100")), Case("aug", (10, 24, 24), dt, (3, 1, "nan")), Case("aug", AUG_BIG, dt, (3, 1, "plain"))]
        for H, W in POOL_SIZES:
            for C in (8, 64):
                out.append(Case("pool", (2, H, W), dt, (C, "plain")))
        out += [Case("pool", (2, 7, 2), dt, (8, "nan")), Case("pool", POOL_BIG[dt][0], dt, (POOL_BIG[dt][1], "plain"))]
        for shape, halo, m1, m2 in LAYOUT_GEOMS:
            for Cr, C in ((1, 8), (3, 8), (8, 8), (3, 16), (8, 16)):
                out.append(Case("layout", shape, dt, (Cr, C, halo, m1, m2, "plain")))
        out += [Case("layout", (3, 24, 24), dt, (3, 8, 1, REFLECT, REFLECT, "nan")), Case("layout", LAYOUT_BIG[0], dt, (3, 8) + LAYOUT_BIG[1:] + ("plain",))]
    return out


CASES = _cases()
GROUPS = ("patch", "l1", "r1", "aug", "pool", "layout")


def case_id(c):
    return f"{c.group}-" + "x".join(map(str, c.shape)) + f"-{NAME[c.dtype]}-" + "-".join(map(str, c.opt))


def seed_of(c):
    return (sum(a * b for a, b in zip(c.shape, (3, 5, 7))) * 31 + GROUPS.index(c.group) * 101 + c.dtype * 1009
            + sum((i + 1) * (hash(o) if isinstance(o, int) else sum(map(ord, o))) for i, o in enumerate(c.opt))) % (2 ** 31)


def check_regime(c):
    """the case reaches the regime it is listed for, from the kernels' documented constants"""
    B, H, W = c.shape
    n = B * H * W
    if c.group == "patch":          # one block of 1024 threads
        t = trips(n, ONE_BLOCK)           # (trips, threads that take the last one)
        assert (t, n - ONE_BLOCK * (t - 1)) == {1: (1, 1), 108: (1, 108), 1024: (1, 1024), 1083: (2, 59), 9800: (10, 584)}[n]
        assert n != 108 or n % 64 != 0    # its last wave is partial
    if c.group in ("l1", "r1"):     # 512 blocks of 256 threads, one pixel per thread and trip
        assert trips(n, L1_THREADS) == {1: 1, 1728: 1, 131072: 1, 131584: 2}[n] and (n != 131072 or n == L1_THREADS)
        assert c.shape != (2, 256, 257) or H != W
    if c.group == "aug":            # the one-block sums loop past 1024 pixels per image, the pointwise kernels past the grid cap
        assert trips(H * W, ONE_BLOCK) == {1: 1, 576: 1, 1023: 1, 1024: 1, 1056: 2, 525625: 514}[H * W]
        assert trips(n, GRID_CAP) == (2 if c.shape == AUG_BIG else 1) and (c.shape != AUG_BIG or (n == 1051250 and W % 2 == 1))
    if c.group == "pool":
        C = c.opt[0]
        chunks = B * R.pool_size(H) * R.pool_size(W) * (C // EPC[c.dtype])
        big = c.shape == POOL_BIG[c.dtype][0]
        assert trips(chunks, GRID_CAP) == (2 if big else 1) and (not big or (chunks == 1056784 and H % 2 == 1))
    if c.group == "layout":
        Cr, C, halo, m1, m2, _ = c.opt
        if m1 == REFLECT and halo == 3:
            assert halo == H - 1          # the limit y0 < H
        if c.shape == LAYOUT_BIG[0]:
            assert trips(B * Cr * H * W, GRID_CAP) == 2 and B * Cr * H * W == 1058400


# ------------------------------------------------------------------------------------------------ helpers
def sync(ctx):
    if ctx.device.type == "cuda":
        torch.cuda.synchronize()


def mkview(ctx, B, H, W, C, halo, dtype, fill, interior=None):
    v = ctx.view(B, H, W, C, halo, dtype=dtype)
    v.t.fill_(fill)
    if interior is not None:
        v.nhwc()[..., :interior.shape[3]].copy_(interior.to(ctx.device))
    return v


def cpu(t):
    return t.detach().cpu().clone()


def inner(p, H, W, halo):
    return p[:, halo:halo + H, halo:halo + W]


def halo_mask(p, H, W, halo):
    m = torch.ones(p.shape, dtype=torch.bool)
    m[:, halo:halo + H, halo:halo + W] = False
    return m


def same_bits(a, b):
    """equal bit for bit; a NaN matches any NaN"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return bool((na == nb).all()) and bool((a.contiguous().view(bits) == b.contiguous().view(bits))[~na].all())


def ratio(got, ref, tol):
    """max |got - ref| / tol.  Where the reference is NaN the result must be NaN, where it is +-Inf the same Inf; a zero tolerance admits
    only an exact match."""
    got = got.double()
    ref = torch.as_tensor(ref, dtype=torch.float64).expand_as(got)
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(got)
    nf = ~torch.isfinite(ref)
    same = torch.where(torch.isnan(ref), torch.isnan(got), got == ref)
    if bool((nf & ~same).any()) or bool((~nf & ~torch.isfinite(got)).any()):
        return INF
    r = ((got - ref).abs() / (tol + 1e-300))[~nf]
    assert not bool(torch.isnan(r).any()), "NaN in a tolerance"
    return float(r.max()) if r.numel() else 0.0


_rejecting = []
_worst = {}


def report(c, group, q, r):
    if _rejecting:
        print(f"[pointwise-family] (against the wrong reference {_rejecting[0]}) {case_id(c)} {q}: {r:.3g}")
    else:
        key = (group, NAME[c.dtype])
        _worst[key] = max(_worst.get(key, 0.0), r)
        print(f"[pointwise-family] {case_id(c)} {q}: error / bound = {r:.3g}")
    return r


def worst_table():
    """the worst error / bound per group and dtype of everything checked so far against the true reference"""
    for (group, dt), r in sorted(_worst.items()):
        print(f"[pointwise-family] WORST {group} {dt}: error / bound = {r:.3g}")
    return dict(_worst)


def check_written(what, padded, H, W, halo, Cr, whole=False):
    """the halo of an output keeps its sentinel unless the call writes the padded extent; channels >= Cr of a written pixel are exactly 0"""
    if not whole:
        assert bool((padded[halo_mask(padded, H, W, halo)].float() == SENT).all()), f"{what}: the halo was written"
    body = padded if whole else inner(padded, H, W, halo)
    pad = body[..., Cr:].float()
    assert bool((pad == 0).all()), f"{what}: channels >= {Cr} of a written pixel are not exactly zero"


def finish(c, worst):
    bad = {q: v for q, v in worst.items() if not v <= 1.0}
    assert not bad, f"{case_id(c)}: outside the derived bound (error / bound): {bad}"


# ------------------------------------------------------------------------------------------------ patch losses
def patch_data(c):
    B, H, W = c.shape
    lh, gh, cls = c.opt
    g = torch.Generator().manual_seed(seed_of(c))
    v = torch.randn(B * H * W, generator=g, dtype=torch.float64) * 2
    special = [1.0, -1.0, 0.0, 100.0, -100.0, 1 + 2.0 ** -7, 1 - 2.0 ** -8, -1 - 2.0 ** -7, -1 + 2.0 ** -8, 88.0, -88.0, 17.0]
    for i, s in enumerate(special):           # spread over the logits: the kinks, 0, and |v| where expf(-|v|) underflows
        if i < v.numel():
            v[(i * 97) % v.numel() if v.numel() > 97 * len(special) else i] = s
    v = v.to(TDT[c.dtype])
    x = torch.full((B, H, W, 8), JUNK, dtype=TDT[c.dtype])
    x[..., 0] = v.view(B, H, W)
    at = (B - 1, H // 2, W // 3)
    if cls in ("nan", "pinf", "ninf"):
        x[at + (0,)] = {"nan": NAN, "pinf": INF, "ninf": -INF}[cls]
    if cls == "unread":
        x[at + (3,)], x[0, 0, 0, 1] = NAN, INF
    return x


def patch_tol(v, mode, target, scale, dtype):
    n = v.numel()
    f, d = R.patch_f64(v, mode, target)
    if mode == 0:
        ef, ed = U * (1 - v).abs(), 0 * f
    elif mode == 1:
        ef, ed = U * (1 + v).abs(), 0 * f
    elif mode == 2:
        ef, ed = 0 * f, 0 * f
    elif mode == 3:
        ef, ed = 3 * U * f + ETA, U * d.abs()
    else:
        ex = torch.exp(-v.abs())
        lg = torch.log1p(ex)
        ef = 4 * U * ex + 4 * U * lg + 2 * ETA + U * (v * target).abs() + U * (torch.relu(v) - v * target).abs() + U * f.abs()
        ed = 6 * U * torch.sigmoid(v) + ETA + U * d.abs()
    inv = abs(scale) / n
    loss = scale * f.sum() / n
    tl = inv * (ef.sum() + ks(n, trips(n, ONE_BLOCK) + 6 + 16) * f.abs().sum()) + 3 * U * loss.abs() + ETA
    gr = scale / n * d
    eg = inv * ed + 2 * U * gr.abs() + ETA
    return tl, eg + U_OUT[dtype] * (gr.abs() + eg)


def run_patch(ctx, c):
    B, H, W = c.shape
    lh, gh, cls = c.opt
    ops = ctx.ops
    x = patch_data(c)
    xv = mkview(ctx, B, H, W, 8, lh, c.dtype, NAN if cls == "unread" else JUNK, x)
    res = dict(v=x[..., 0].double(), runs={})
    for mode, target in PATCH_VARIANTS:
        outs = []
        for rep in range(2):
            gv = mkview(ctx, B, H, W, 8, gh, c.dtype, SENT)
            loss = ctx.f32(1, LOSS_PRIOR)
            ops.patch_loss(xv, mode, target, SCALE, loss, gv)()
            sync(ctx)
            outs.append((cpu(loss), cpu(gv.padded())))
        loss0 = ctx.f32(1, LOSS_PRIOR)
        ops.patch_loss(xv, mode, target, SCALE, loss0, None)()
        sync(ctx)
        res["runs"][(mode, target)] = outs + [cpu(loss0)]
    return res


def check_patch(c, res, ref):
    B, H, W = c.shape
    lh, gh, cls = c.opt
    v, scale, worst = res["v"], t32(SCALE), {}
    for (mode, target), (a, b, loss0) in res["runs"].items():
        what = f"{case_id(c)} mode {mode} target {target}"
        target = t32(target)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), f"{what}: a repeated call gave other bits"
        assert same_bits(a[0], loss0), f"{what}: the loss without a gradient view differs"
        check_written(what, a[1], H, W, gh, 1)
        want_l, want_g = R.patch_loss64(v, mode, target, scale, ref)
        tl, tg = patch_tol(v, mode, target, scale, c.dtype)
        fin = torch.isfinite(v)
        worst[f"loss{mode}/{target:g}"] = ratio(a[0][0], want_l, tl)
        worst[f"grad{mode}/{target:g}"] = ratio(inner(a[1], H, W, gh)[..., 0][fin], want_g[fin], tg[fin])
        if ref is R.Ref:
            if cls == "nan":
                assert math.isnan(float(want_l)), what
            if cls in ("pinf", "ninf") and (mode >= 2 or (mode == 0) == (cls == "ninf")):      # the hinges are flat on one side: relu(-Inf) = 0
                assert not math.isfinite(float(want_l)), what
            if cls in ("plain", "unread"):
                assert math.isfinite(float(want_l)), what
    for q, r in worst.items():
        report(c, "patch." + q[:4], q, r)
    finish(c, worst)


# ------------------------------------------------------------------------------------------------ L1 and R1
def loss_data(c):
    """x interior (B, H, W, 8) with junk in the pad channels; for L1 the NCHW fp32 target, equal to x on a lattice of pixels"""
    B, H, W = c.shape
    Cr, cls = c.opt
    g = torch.Generator().manual_seed(seed_of(c))
    x = torch.full((B, H, W, 8), JUNK, dtype=torch.float64)
    x[..., :Cr] = torch.randn(B, H, W, Cr, generator=g, dtype=torch.float64) * (3.0 if c.group == "r1" else 1.0)
    x[1::2, ..., :Cr] *= 2.0 ** -4
    x = x.to(TDT[c.dtype])
    t = x[..., :Cr].double() + 0.5 * torch.randn(B, H, W, Cr, generator=g, dtype=torch.float64)
    eq = (torch.arange(B * H * W * Cr) % 7 == 0).view(B, H, W, Cr)
    t = torch.where(eq, x[..., :Cr].double(), t).float().permute(0, 3, 1, 2).contiguous()         # a bf16 or fp32 value is an fp32 value
    at = (B - 1, H // 2, W // 3)
    if cls in ("nan", "pinf", "ninf"):
        bad = {"nan": NAN, "pinf": INF, "ninf": -INF}[cls]
        if c.group == "l1" and cls != "nan":
            t[at[0], Cr - 1, at[1], at[2]] = bad            # the target is read as well
        else:
            x[at + (Cr - 1,)] = bad
    if cls == "unread":
        x[at + (Cr,)], x[0, 0, 0, 7] = NAN, INF
    return x, t


def run_loss(ctx, c):
    B, H, W = c.shape
    Cr, cls = c.opt
    ops = ctx.ops
    x, t = loss_data(c)
    xv = mkview(ctx, B, H, W, 8, 1, c.dtype, NAN if cls == "unread" else JUNK, x)
    td, dev = t.to(ctx.device), ctx.f32(1, DEV_SCALE)
    res = dict(x=x[..., :Cr].double(), t=t.double(), runs={}, is_hip=ops.is_hip)
    variants = [("grad", True, dev), ("grad", True, dev), ("nodev", True, None), ("nograd", False, dev)] if c.group == "l1" else \
               [("grad", True, None), ("grad", True, None), ("nograd", False, None)]
    for name, has, dv in variants:
        gv = mkview(ctx, B, H, W, 8, 1, c.dtype, SENT) if has else None
        loss, ws = ctx.f32(1, LOSS_PRIOR), ctx.f32(L1_WS + GUARD, WS_FILL)
        if c.group == "l1":
            ops.l1_loss(xv, Cr, td, SCALE, dv, loss, gv, ws)()
        else:
            ops.r1_reduce(xv, Cr, SCALE, loss, gv, ws)()
        sync(ctx)
        res["runs"].setdefault(name, []).append((cpu(loss), cpu(gv.padded()) if has else None, cpu(ws)))
    return res


def check_loss(c, res, ref):
    B, H, W = c.shape
    Cr, cls = c.opt
    x, t, scale, dev, worst = res["x"], res["t"], t32(SCALE), t32(DEV_SCALE), {}
    n = x.numel()
    depth = trips(B * H * W, L1_THREADS) * Cr + 6 + 4 + 2 + 6 + 4          # levels of l1_kernel / r1_kernel and sum_scale_kernel
    a, b = res["runs"]["grad"]
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2]), f"{case_id(c)}: a repeated call gave other bits"
    for name, outs in res["runs"].items():
        loss, gp, ws = outs[0]
        what = f"{case_id(c)} {name}"
        assert same_bits(loss, a[0]), f"{what}: the loss depends on the gradient view or the device scale"
        if res["is_hip"]:
            assert bool((ws[L1_WS:] == WS_FILL).all()), f"{what}: workspace floats past ws[0 .. 512) were written"
        state = lambda rf: R.l1_loss64(x, t, scale, dev if name != "nodev" else None, rf) if c.group == "l1" else R.r1_reduce64(x, scale, rf)
        (want_l, want_g), (true_l, true_g) = state(ref), state(R.Ref)          # the tolerances are those of the true statement
        if c.group == "l1":
            d = x - t.permute(0, 2, 3, 1)
            tl = scale / n * (U + ks(n, depth)) * d.abs().sum() + 3 * U * true_l.abs() + ETA
            fin = torch.isfinite(d)
        else:
            tl = ((0.0 if c.dtype == BF16 else U) + ks(n, depth)) * (x * x).sum() / B + 3 * U * true_l.abs() + ETA
            fin = torch.isfinite(x)
        worst[f"loss/{name}"] = ratio(loss[0], want_l, tl)
        if gp is not None:
            check_written(what, gp, H, W, 1, Cr)
            eg = 2 * U * true_g.abs() + ETA
            worst[f"grad/{name}"] = ratio(inner(gp, H, W, 1)[..., :Cr][fin], want_g[fin], (eg + U_OUT[c.dtype] * (true_g.abs() + eg))[fin])
        if ref is R.Ref:
            assert math.isnan(float(want_l)) if cls == "nan" else math.isfinite(float(want_l)) == (cls in ("plain", "unread")), what
            if c.group == "l1" and cls == "plain":
                assert int((d == 0).sum()) >= n // 7, "no pixels with x == t"
    for q, r in worst.items():
        report(c, c.group + "." + q[:4], q, r)
    finish(c, worst)


# ------------------------------------------------------------------------------------------------ DiffAugment
def aug_rows(H, W):
    """the parameter rows of one batch: (brightness, saturation, contrast, tx, ty, lo_h, hi_h, lo_w, hi_w), all exact floats"""
    no = (1, 0, 1, 0)
    return [
        (0.0, 1.0, 1.0, 0, 0) + no,                                                        # 0 identity
        (0.25, 0.0, 0.5, H - 1, -(W - 1)) + no,                                             # 1 tx = +(H - 1), ty of the opposite sign
        (-0.3125, 2.0, 1.5, -(H - 1), W - 1) + no,                                          # 2 tx = -(H - 1)
        (0.125, 1.25, 0.75, H, 0) + no,                                                     # 3 |tx| >= H: nothing is read
        (0.125, 1.25, 0.75, -(H + 2), min(1, W - 1)) + no,                                  # 4
        (0.0625, 0.5, 1.5, min(1, H - 1), -min(2, W - 1), -2, H // 3, W - 1 - W // 4, W + 3),   # 5 a cutout clipped by the border
        (-0.125, 2.0, 0.5, 0, 0, 0, H - 1, 0, W - 1),                                       # 6 a cutout that covers the image
        (0.375, 0.0, 1.5, -min(1, H - 1), min(1, W - 1), H // 2, H // 2, W // 2, W // 2),   # 7 a cutout of one pixel
        (0.1875, 0.75, 1.25, min(2, H - 1), -min(3, W - 1), H // 4, H // 2, W // 3, 2 * W // 3),  # 8
        (-0.4375, 2.0, 0.5, 0, 0) + no,                                                     # 9
    ]


def aug_params(c):
    B, H, W = c.shape
    rows = aug_rows(H, W)
    rows = [rows[8], rows[5]] if c.shape == AUG_BIG else rows
    assert len(rows) == B
    p = torch.zeros(B, 12, dtype=torch.float32)
    p[:, :9] = torch.tensor(rows, dtype=torch.float32)
    return p


def aug_data(c):
    B, H, W = c.shape
    Cr, yh, cls = c.opt
    g = torch.Generator().manual_seed(seed_of(c))
    x = torch.full((B, H, W, 8), JUNK, dtype=torch.float64)
    x[..., :Cr] = 0.5 * torch.randn(B, H, W, Cr, generator=g, dtype=torch.float64) + (50.0 if cls == "mean100" else 0.1)
    gy = torch.full((B, H, W, 8), JUNK, dtype=torch.float64)
    gy[..., :Cr] = torch.randn(B, H, W, Cr, generator=g, dtype=torch.float64) * 2.0 ** -6 + 2.0 ** -9
    x, gy = x.to(TDT[c.dtype]), gy.to(TDT[c.dtype])
    if cls == "nan":
        x[8, 5, 5, 1] = NAN           # read: the image's mean and every pixel of it that takes a value
        x[3, 2, 2, 0] = NAN           # image 3 reads nothing (|tx| >= H): zeros
        x[0, 1, 1, 5] = NAN           # a pad channel
        gy[8, 3, 8, 0] = NAN          # a pixel that took a value
        gy[6, 4, 4, 2] = NAN          # cut
        gy[0, 2, 2, 6] = NAN          # a pad channel
    return x, gy


def aug_fwd_tol(x, prm, dtype):
    """Fl replay of diffaug_fwd_kernel per SOURCE pixel, and the image sums it reads from the workspace"""
    B, H, W, C = x.shape
    n = C * H * W
    br, sat, con = (prm[:, i].double().view(B, 1, 1, 1) for i in range(3))
    t = Fl(x) + br
    mc = channel_mean(t)
    s = (t - mc) * sat + mc
    S = Fl(x.sum((1, 2, 3), keepdim=True), k(n) * x.abs().sum((1, 2, 3), keepdim=True))
    mu = S * Fl(1.0 / n, torch.tensor(U / n, dtype=torch.float64)) + br
    v = (s - mu) * con + mu
    return v, S


def aug_bwd_tol(gs, g_valid, prm, dtype):
    """Fl replay of diffaug_bwd_kernel: gs the masked gradient at its source pixel, g_valid the same at the output pixel"""
    B, H, W, C = gs.shape
    n = C * H * W
    sat, con = (prm[:, i].double().view(B, 1, 1, 1) for i in (1, 2))
    G = Fl(g_valid.sum((1, 2, 3), keepdim=True), k(n) * g_valid.abs().sum((1, 2, 3), keepdim=True))
    gm = G * Fl(1.0 / n, torch.tensor(U / n, dtype=torch.float64))
    g1 = Fl(gs) * con + (1 - Fl(con)) * gm
    mc = channel_mean(g1)
    return g1 * sat + (1 - Fl(sat)) * mc, G


def run_aug(ctx, c):
    B, H, W = c.shape
    Cr, yh, cls = c.opt
    ops = ctx.ops
    x, gy = aug_data(c)
    prm = aug_params(c)
    pd = prm.reshape(-1).to(ctx.device)
    res = dict(prm=prm, is_hip=ops.is_hip, x=x[..., :Cr].double(), gy=gy[..., :Cr].double())
    if c.shape == AUG_BIG:             # the input arrives through gan_nchw_to_view, as the trainer's does; that launch passes the grid cap too
        src = x[..., :Cr].float().permute(0, 3, 1, 2).contiguous()
        xv = mkview(ctx, B, H, W, 8, 0, c.dtype, SENT)
        ops.nchw_to_view(src.to(ctx.device), Cr, xv, NONE)()
        sync(ctx)
        want = torch.zeros(B, H, W, 8, dtype=TDT[c.dtype])
        want[..., :Cr] = x[..., :Cr]
        assert same_bits(cpu(xv.padded()), want), f"{case_id(c)}: gan_nchw_to_view past the grid cap"
    else:
        xv = mkview(ctx, B, H, W, 8, 0, c.dtype, JUNK, x)
    gv = mkview(ctx, B, H, W, 8, yh, c.dtype, NAN if cls == "nan" else JUNK, gy)
    outs = []
    for rep in range(2):
        yv, gxv = mkview(ctx, B, H, W, 8, yh, c.dtype, SENT), mkview(ctx, B, H, W, 8, 0, c.dtype, SENT)
        ws1, ws2 = ctx.f32(B + GUARD, WS_FILL), ctx.f32(B + GUARD, WS_FILL)
        ops.diffaug_fwd(xv, Cr, pd, yv, ws1)()
        ops.diffaug_bwd(gv, Cr, pd, gxv, ws2)()
        sync(ctx)
        outs.append((cpu(yv.padded()), cpu(gxv.padded()), cpu(ws1), cpu(ws2)))
    res["outs"] = outs
    return res


def check_aug(c, res, ref):
    B, H, W = c.shape
    Cr, yh, cls = c.opt
    what, prm, x, gy = case_id(c), res["prm"], res["x"], res["gy"]
    a, b = res["outs"]
    assert all(same_bits(p, q) for p, q in zip(a, b)), f"{what}: a repeated call gave other bits"
    check_written(what + " y", a[0], H, W, yh, Cr)
    check_written(what + " gx", a[1], H, W, 0, Cr)
    # tolerances of the true statement
    sh, sw, valid = R.aug_geometry(prm, H, W)
    bb = torch.arange(B).view(B, 1, 1).expand(B, H, W)
    zero = torch.zeros((), dtype=torch.float64)
    v, S = aug_fwd_tol(x, prm, c.dtype)
    tol_y = torch.where(valid.unsqueeze(-1), v.stored(c.dtype)[bb, sh, sw], zero)
    g_valid = torch.where(valid.unsqueeze(-1), gy, zero)
    gs = torch.zeros_like(gy)
    gs.index_put_((bb[valid], sh[valid], sw[valid]), g_valid[valid], accumulate=True)
    w, G = aug_bwd_tol(gs, g_valid, prm, c.dtype)
    worst = {"y": ratio(inner(a[0], H, W, yh)[..., :Cr], R.diffaug_fwd64(x, prm, ref), tol_y),
             "gx": ratio(a[1][..., :Cr], R.diffaug_bwd64(gy, prm, ref), w.stored(c.dtype))}
    if res["is_hip"]:
        for name, ws, s in (("ws.sum", a[2], S), ("ws.gsum", a[3], G)):
            assert bool((ws[B:] == WS_FILL).all()), f"{what}: workspace floats past ws[0 .. B) were written"
            worst[name] = ratio(ws[:B], s.v.view(B), s.e.view(B) + U * s.v.view(B).abs())
    if ref is R.Ref:
        dead = ~valid.reshape(B, -1).any(1)
        gone = {i for i in range(B) if dead[i]}           # |tx| >= H twice and the whole cutout (on one pixel every cutout is whole)
        assert gone == set() if B == 2 else ({3, 4, 6} <= gone and (H * W == 1 or gone == {3, 4, 6}))
        assert bool((inner(a[0], H, W, yh)[dead].float() == 0).all()) and bool((a[1][dead][..., :Cr].float() == 0).all()), f"{what}: an image that reads nothing"
        if res["is_hip"]:
            assert bool((a[3][:B][dead] == 0).all()), f"{what}: the gradient sum of an image that reads nothing is not 0"
        if cls == "mean100":          # the growth the module docstring states: the contrast line's error against the spread
            e = (inner(a[0], H, W, yh)[..., :Cr].double() - R.diffaug_fwd64(x, prm)).abs().max()
            print(f"[pointwise-family] {what}: max |y - ref| = {float(e):.3g} for a spread of 0.5 about a mean of 50 (bound {float(tol_y.max()):.3g})")
        if cls == "nan":
            yy = inner(a[0], H, W, yh)[..., :Cr]
            assert bool(torch.isnan(yy[8][valid[8]]).all()) and not bool(torch.isnan(yy[[i for i in range(B) if i != 8]]).any())
            assert bool(torch.isnan(a[1][8][..., :Cr]).all()) and not bool(torch.isnan(a[1][[i for i in range(B) if i != 8]][..., :Cr]).any())
    report(c, "aug_fwd", "y", worst["y"])
    report(c, "aug_bwd", "gx", worst["gx"])
    for q in ("ws.sum", "ws.gsum"):
        if q in worst:
            report(c, "aug_sums", q, worst[q])
    finish(c, worst)


# ------------------------------------------------------------------------------------------------ AvgPool
def run_pool(ctx, c):
    B, H, W = c.shape
    C, cls = c.opt
    ops = ctx.ops
    Ho, Wo = R.pool_size(H), R.pool_size(W)
    g = torch.Generator().manual_seed(seed_of(c))
    x = (torch.randn(B, H, W, C, generator=g) + 0.25).to(TDT[c.dtype])
    gy = torch.randn(B, Ho, Wo, C, generator=g).to(TDT[c.dtype])
    prior = (torch.randn(B, H, W, C, generator=g) * 2.0 ** 6).to(TDT[c.dtype])
    if cls == "nan":
        x[1, H // 2, W - 1, 3], gy[0, Ho - 1, 0, 5] = NAN, NAN
    big = c.shape == POOL_BIG[c.dtype][0]
    res = dict(x=x, gy=gy, prior=prior, fwd={}, bwd={})
    gv = mkview(ctx, B, Ho, Wo, C, 1, c.dtype, NAN if cls == "nan" else JUNK, gy)
    for halo in ((1,) if big else (1, 0)):
        xv = mkview(ctx, B, H, W, C, halo, c.dtype, NAN if cls == "nan" else JUNK, x)
        for rep in range(2):
            yv = mkview(ctx, B, Ho, Wo, C, 1, c.dtype, SENT)
            ops.avgpool_fwd(xv, yv)()
            sync(ctx)
            res["fwd"].setdefault(halo, []).append(cpu(yv.padded()))
    for acc, halo in (((0, 1),) if big else ((0, 1), (1, 0))):
        for rep in range(2):
            gxv = mkview(ctx, B, H, W, C, halo, c.dtype, SENT, prior if acc else None)
            ops.avgpool_bwd(gv, gxv, bool(acc))()
            sync(ctx)
            res["bwd"].setdefault((acc, halo), []).append(cpu(gxv.padded()))
    return res


def check_pool(c, res, ref):
    B, H, W = c.shape
    C, cls = c.opt
    Ho, Wo = R.pool_size(H), R.pool_size(W)
    what, worst = case_id(c), {}
    parts = []
    for b in range(B):                # image by image: the float64 temporaries of the largest case stay small
        xb, gb = res["x"][b:b + 1].double(), res["gy"][b:b + 1].double()
        ty, mag_y = R.avgpool_fwd64(xb)
        tg, mag_g, terms = R.avgpool_bwd64(gb, H, W)
        y, gx = (ty, tg) if ref is R.Ref else (R.avgpool_fwd64(xb, ref)[0], R.avgpool_bwd64(gb, H, W, ref)[0])
        parts.append((y, mag_y, gx, mag_g, terms, ty, tg))
    want_y, mag_y, want_g, mag_g, terms, true_y, true_g = (torch.cat(t) for t in zip(*parts))      # the tolerances are the true statement's
    cnt = R.pool_counts(H, W)
    for halo, (a, b_) in res["fwd"].items():
        assert same_bits(a, b_), f"{what}: a repeated call gave other bits"
        check_written(what + " y", a, Ho, Wo, 1, C)
        e = (cnt - 1) * U * mag_y / cnt + U * true_y.abs()
        worst[f"y/halo{halo}"] = ratio(inner(a, Ho, Wo, 1), want_y, e + U_OUT[c.dtype] * (true_y.abs() + e))
    prior = res["prior"].double()
    for (acc, halo), (a, b_) in res["bwd"].items():
        assert same_bits(a, b_), f"{what}: a repeated call gave other bits"
        check_written(what + " gx", a, H, W, halo, C)
        p = prior if acc else torch.zeros_like(prior)
        e = 2 * U * mag_g + terms * U * (p.abs() + mag_g) + ETA
        worst[f"gx/acc{acc}"] = ratio(inner(a, H, W, halo), p + want_g, e + U_OUT[c.dtype] * ((p + true_g).abs() + e))
    if ref is R.Ref and cls == "nan":
        y = inner(res["fwd"][1][0], Ho, Wo, 1)
        hit = torch.zeros(B, Ho, Wo, C, dtype=torch.bool)
        iy, ix = H // 2, W - 1
        for oy in range(Ho):
            for ox in range(Wo):
                hit[1, oy, ox, 3] = abs(2 * oy - iy) <= 1 and abs(2 * ox - ix) <= 1
        assert bool(hit.any()) and torch.equal(torch.isnan(y), hit), f"{what}: the NaN reached other outputs than the windows that read it"
        gx = inner(res["bwd"][(0, 1)][0], H, W, 1)
        hit = torch.zeros(B, H, W, C, dtype=torch.bool)
        for y_ in range(H):
            for x_ in range(W):
                hit[0, y_, x_, 5] = abs(2 * (Ho - 1) - y_) <= 1 and abs(0 - x_) <= 1
        assert bool(hit.any()) and torch.equal(torch.isnan(gx), hit), f"{what}: the NaN of gy reached other pixels than its window"
    for q, r in worst.items():
        report(c, "pool_fwd" if q[0] == "y" else "pool_bwd", q, r)
    finish(c, worst)


# ------------------------------------------------------------------------------------------------ layout
def run_layout(ctx, c):
    B, H, W = c.shape
    Cr, C, halo, m1, m2, cls = c.opt
    ops = ctx.ops
    g = torch.Generator().manual_seed(seed_of(c))
    src = torch.randn(B, Cr, H, W, generator=g) * 3            # fp32 values that bf16 has to round
    if cls == "nan":
        src[1, Cr - 1, 0, 1], src[2, 0, H - 2, W - 1] = NAN, NAN
    res = dict(src=src)
    d1, d2 = mkview(ctx, B, H, W, C, halo, c.dtype, SENT), mkview(ctx, B, H, W, C, halo, c.dtype, SENT)
    back = torch.full((B, Cr, H, W), SENT, dtype=torch.float32, device=ctx.device)
    ops.nchw_to_view(src.to(ctx.device), Cr, d1, m1)()
    ops.view_copy(d1, d2, m2)()
    ops.view_to_nchw(d2, Cr, back)()
    sync(ctx)
    res.update(d1=cpu(d1.padded()), d2=cpu(d2.padded()), back=cpu(back))
    d1b, backb = mkview(ctx, B, H, W, C, halo, c.dtype, SENT), torch.full((B, Cr, H, W), SENT, dtype=torch.float32, device=ctx.device)
    ops.nchw_to_view(src.to(ctx.device), Cr, d1b, m1)()
    ops.view_to_nchw(d1b, Cr, backb)()
    sync(ctx)
    assert same_bits(cpu(d1b.padded()), res["d1"]) and same_bits(cpu(backb), res["back"]), f"{case_id(c)}: a repeated call gave other bits"
    return res


def layout_want(v64, halo, mode, dtype, ref):
    """the padded extent after a call that writes the interior (NONE) or the whole of it"""
    B, H, W, C = v64.shape
    if mode == NONE:
        out = torch.full((B, H + 2 * halo, W + 2 * halo, C), SENT, dtype=torch.float64)
        inner(out, H, W, halo).copy_(v64)
    else:
        out = R.with_halo64(v64, halo, mode, ref)
    return out.to(TDT[dtype])


def check_layout(c, res, ref):
    B, H, W = c.shape
    Cr, C, halo, m1, m2, cls = c.opt
    what = case_id(c)
    v = R.nchw_to_nhwc64(res["src"], C)
    want1 = layout_want(v, halo, m1, c.dtype, ref)
    ok = {"nchw_to_view": same_bits(res["d1"], want1)}
    check_written(what + " nchw_to_view", res["d1"], H, W, halo, Cr, whole=m1 != NONE)
    stored = inner(res["d1"], H, W, halo).double()          # view_copy moves what nchw_to_view stored
    ok["view_copy"] = same_bits(res["d2"], layout_want(stored, halo, m2, c.dtype, ref))
    ok["view_to_nchw"] = same_bits(res["back"], res["src"].to(TDT[c.dtype]).float())
    if ref is R.Ref and cls == "nan" and m1 == REFLECT:
        assert int(torch.isnan(res["d1"]).sum()) > 2 and int(torch.isnan(res["back"]).sum()) == 2, f"{what}: NaN copies"
    worst = {q: 0.0 if good else INF for q, good in ok.items()}
    for q, r in worst.items():
        report(c, "layout", q, r)
    finish(c, worst)


# ------------------------------------------------------------------------------------------------ running and checking a case
RUN = dict(patch=run_patch, l1=run_loss, r1=run_loss, aug=run_aug, pool=run_pool, layout=run_layout)
CHECK = dict(patch=check_patch, l1=check_loss, r1=check_loss, aug=check_aug, pool=check_pool, layout=check_layout)
_results = {}
KEEP_PIXELS = 1 << 18          # results of larger cases are not cached (no wrong reference is tried on them)


def result(make, c):
    ctx = make()
    key = (ctx.device.type, c)
    if key in _results:
        return _results[key]
    check_regime(c)
    res = RUN[c.group](ctx, c)
    if c.shape[0] * c.shape[1] * c.shape[2] < KEEP_PIXELS:
        _results[key] = res
    return res


def body(make, c, ref=None):
    CHECK[c.group](c, result(make, c), ref or R.Ref)


# ------------------------------------------------------------------------------------------------ wrong references
def _wrong(name, **kw):
    return type(name, (R.Ref,), kw)


def _find(group, shape, dtype, *opt):
    c = Case(group, shape, dtype, opt)
    assert c in CASES, c
    return c


# every wrong statement with the named cases it must fail on
WRONG = [
    (_wrong("CountIncludePad", count_include_pad=True), [_find("pool", (2, 7, 2), F32, 8, "plain"), _find("pool", (2, 24, 24), BF16, 64, "plain")]),
    (_wrong("TransposeDividesBy9", pool_t_div9=True), [_find("pool", (2, 3, 3), F32, 8, "plain"), _find("pool", (2, 25, 31), BF16, 8, "plain")]),
    (_wrong("ExclusiveCutout", cut_exclusive=True), [_find("aug", (10, 24, 24), F32, 3, 1, "plain"), _find("aug", (10, 33, 31), BF16, 1, 0, "plain")]),
    (_wrong("TranslationSignSwapped", shift_sign=-1), [_find("aug", (10, 24, 24), BF16, 3, 1, "plain"), _find("aug", (10, 33, 32), F32, 1, 1, "plain")]),
    (_wrong("ContrastMeanPerChannel", contrast_per_channel=True), [_find("aug", (10, 24, 24), F32, 3, 0, "plain"), _find("aug", (10, 32, 32), BF16, 3, 1, "plain")]),
    (_wrong("ContrastMeanBeforeBrightness", contrast_mean_raw=True), [_find("aug", (10, 24, 24), BF16, 3, 1, "plain"), _find("aug", (10, 1, 1), F32, 1, 1, "plain")]),
    (_wrong("SignOfZeroIsOne", sign0=1.0), [_find("l1", (3, 24, 24), BF16, 3, "plain"), _find("l1", (1, 1, 1), F32, 1, "plain")]),
    (_wrong("NoDeviceGradScale", no_dev_scale=True), [_find("l1", (3, 24, 24), F32, 4, "plain"), _find("l1", (2, 256, 257), BF16, 1, "plain")]),
    (_wrong("L1DividedByNMinus1", n_minus_1=True), [_find("l1", (3, 24, 24), BF16, 3, "plain"), _find("l1", (3, 24, 24), F32, 4, "plain")]),
    (_wrong("HingeKinkDerivative", kink=1.0), [_find("patch", (3, 6, 6), F32, 1, 2, "plain"), _find("patch", (3, 19, 19), BF16, 1, 0, "plain")]),
    (_wrong("PatchDividedByNMinus1", n_minus_1=True), [_find("patch", (3, 19, 19), F32, 1, 0, "plain"), _find("patch", (2, 70, 70), BF16, 1, 2, "plain")]),
    (_wrong("R1WithoutFactor2", r1_factor=1.0), [_find("r1", (3, 24, 24), BF16, 3, "plain"), _find("r1", (1, 1, 1), F32, 1, "plain")]),
    (_wrong("ReflectAsReplicate", reflect_as_replicate=True), [_find("layout", (2, 4, 5), BF16, 3, 8, 3, REFLECT, REFLECT, "plain"),
                                                               _find("layout", (3, 24, 24), F32, 8, 16, 1, REFLECT, REFLECT, "plain")]),
]


def rejects(make, wrong, cases):
    """the results held to the wrong reference fail on every case listed for it"""
    failed = []
    _rejecting.append(wrong.__name__)
    try:
        for c in cases:
            res = result(make, c)
            try:
                CHECK[c.group](c, res, wrong)
            except AssertionError as e:
                failed.append((case_id(c), str(e)[:100]))
    finally:
        _rejecting.clear()
    print(f"[pointwise-family] {wrong.__name__} rejected on {failed}")
    assert len(failed) == len(cases), f"the assertions accept the wrong reference {wrong.__name__} on a case it was tried on"


# ------------------------------------------------------------------------------------------------ refused arguments (the C ABI's checks)
def body_refused(make):
    """each returns its error and launches nothing: every output, loss and workspace keeps its sentinel"""
    from gan_variant_research_amd._lib import GanError
    ctx = make()
    ops = ctx.ops
    B, H, W = 2, 6, 6
    made = []

    def out(dtype=F32, H_=H, W_=W, C=8, halo=1):
        made.append(mkview(ctx, B, H_, W_, C, halo, dtype, SENT))
        return made[-1]
    x = mkview(ctx, B, H, W, 8, 1, F32, 1.0)
    x3 = mkview(ctx, B, 3, 3, 8, 3, F32, 1.0)
    prm = aug_params(Case("aug", (10, H, W), F32, (3, 1, "plain")))[:B].reshape(-1).contiguous().to(ctx.device)
    tgt = torch.zeros(B, 5, H, W, device=ctx.device)
    nchw = torch.zeros(B, 3, 3, 3, device=ctx.device)
    loss, ws = ctx.f32(1, LOSS_PRIOR), ctx.f32(L1_WS + GUARD, WS_FILL)
    calls = {}
    for Cr in (0, 5):
        calls[f"diffaug_fwd C={Cr}"] = lambda Cr=Cr: ops.diffaug_fwd(x, Cr, prm, out(), ws)
        calls[f"diffaug_bwd C={Cr}"] = lambda Cr=Cr: ops.diffaug_bwd(x, Cr, prm, out(), ws)
        calls[f"l1_loss C={Cr}"] = lambda Cr=Cr: ops.l1_loss(x, Cr, tgt, SCALE, None, loss, out(), ws)
        calls[f"r1_reduce C={Cr}"] = lambda Cr=Cr: ops.r1_reduce(x, Cr, SCALE, loss, out(), ws)
    calls.update({
        "patch_loss grad C=16": lambda: ops.patch_loss(x, 0, 0.0, SCALE, loss, out(C=16)),
        "l1_loss grad C=16": lambda: ops.l1_loss(x, 3, tgt, SCALE, None, loss, out(C=16), ws),
        "r1_reduce u C=16": lambda: ops.r1_reduce(x, 3, SCALE, loss, out(C=16), ws),
        "patch_loss grad dtype": lambda: ops.patch_loss(x, 0, 0.0, SCALE, loss, out(BF16)),
        "patch_loss grad shape": lambda: ops.patch_loss(x, 0, 0.0, SCALE, loss, out(H_=H + 1)),
        "l1_loss grad dtype": lambda: ops.l1_loss(x, 3, tgt, SCALE, None, loss, out(BF16), ws),
        "l1_loss grad shape": lambda: ops.l1_loss(x, 3, tgt, SCALE, None, loss, out(W_=W - 1), ws),
        "r1_reduce u dtype": lambda: ops.r1_reduce(x, 3, SCALE, loss, out(BF16), ws),
        "r1_reduce u shape": lambda: ops.r1_reduce(x, 3, SCALE, loss, out(H_=H - 1), ws),
        "diffaug_fwd dtype": lambda: ops.diffaug_fwd(x, 3, prm, out(BF16), ws),
        "diffaug_fwd shape": lambda: ops.diffaug_fwd(x, 3, prm, out(H_=H + 1), ws),
        "diffaug_bwd dtype": lambda: ops.diffaug_bwd(x, 3, prm, out(BF16), ws),
        "diffaug_bwd shape": lambda: ops.diffaug_bwd(x, 3, prm, out(W_=W + 2), ws),
        "diffaug_fwd y C=16": lambda: ops.diffaug_fwd(x, 3, prm, out(C=16), ws),
        "patch_loss mode 5": lambda: ops.patch_loss(x, 5, 0.0, SCALE, loss, out()),
        "patch_loss mode -1": lambda: ops.patch_loss(x, -1, 0.0, SCALE, loss, out()),
        "avgpool_fwd size H/2+1": lambda: ops.avgpool_fwd(x, out(H_=4, W_=3)),
        "avgpool_fwd dtype": lambda: ops.avgpool_fwd(x, out(BF16, H_=3, W_=3)),
        "avgpool_fwd channels": lambda: ops.avgpool_fwd(x, out(H_=3, W_=3, C=16)),
        "avgpool_bwd size": lambda: ops.avgpool_bwd(x, out(H_=2 * H + 1, W_=2 * W), False),
        "avgpool_bwd dtype": lambda: ops.avgpool_bwd(x, out(BF16, H_=2 * H, W_=2 * W), True),
        "nchw_to_view reflect y0 == H": lambda: ops.nchw_to_view(nchw, 3, out(H_=3, W_=3, halo=3), REFLECT),
        "nchw_to_view C=0": lambda: ops.nchw_to_view(nchw, 0, out(H_=3, W_=3), NONE),
        "nchw_to_view C=9": lambda: ops.nchw_to_view(nchw, 9, out(H_=3, W_=3), NONE),
        "view_copy reflect y0 == H": lambda: ops.view_copy(x3, out(H_=3, W_=3, halo=3), REFLECT),
        "view_copy shape": lambda: ops.view_copy(x, out(H_=H + 1), NONE),
        "view_copy dtype": lambda: ops.view_copy(x, out(BF16), NONE),
    })
    back = torch.full((B, 3, H, W), SENT, device=ctx.device)
    for Cr in (0, 9):
        calls[f"view_to_nchw C={Cr}"] = lambda Cr=Cr: ops.view_to_nchw(x, Cr, back)
    for name, call in calls.items():
        with pytest.raises(GanError):
            call()()
        sync(ctx)
        assert float(loss[0]) == LOSS_PRIOR and bool((ws == WS_FILL).all()), f"{name}: a refused call wrote the loss or the workspace"
        assert all(bool((v.t.float() == SENT).all()) for v in made) and bool((back == SENT).all()), f"{name}: a refused call wrote its output"
