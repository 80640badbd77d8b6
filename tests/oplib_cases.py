"""TEST INFRASTRUCTURE: cases, references and assertions for the operator library torch.ops.mi355x_gan.* and its drop-in modules
(gan_variant_research_amd/ops_library.py), op by op.  A body takes a device: tests/test_oplib_family_cpu.py runs it on the emulator (through
autograd._OPS_FACTORY), tests/test_oplib_family_gpu.py on the kernels, with the same shapes and the same assertions.

Every case calls the op through torch.ops.mi355x_gan (or the module), takes gradients with torch.autograd.grad and compares every element
with float64 on the same operands (rounded to bf16 first in BF16 mode).  No tolerance is new:

  CONVOLUTIONS.  y: tests/conv_ref64.elem_tol (cases.derived_bound for the plain epilogue).  The activation's backward is an op of its own
  (act_bwd, from the saved output y, header: relu y > 0 ? 1 : 0, lrelu y > 0 ? 1 : 0.2, tanh 1 - y^2): its result g' is held to
  gy * act'(y) with the act_bwd bound of tests/norm_cases.check_fold, e = u |gy act'| + |gy| u {lrelu 0.2, tanh 2 (1 + y^2)} + u |want|,
  tol = e + u (|want| + e).  The gradients are then held to float64 on the operand the library stages, g' as the op returned it (rounded
  to bf16 in BF16 mode, as nchw_to_view rounds it): dx to cases.derived_bound, dw and db to the weight-gradient family's
  derived_bound(., ., K, 0).  A reflect-padded layer's dx is the fold of the padded-domain gradient: every pre-image is stored (u_out) and
  then added in fp32, so with n the number of pre-images of a pixel (tests/norm_cases.check_fold, fold_add)
        tol = T + u_out (|want| + T),   T = fold(tol_p) + (n + 1) u fold(|ref_p| + tol_p),   tol_p = derived_bound on the padded domain.

  INSTANCE NORM.  The returned statistics against float64 sums inside tests/norm_cases.stats_tol (mean) and its rstd interval; y and dx
  GIVEN those statistics inside norm_cases.apply_tol and norm_cases.bwd_terms -- the norm family's own statement, unchanged
  (tests/test_norm_family_cpu.py holds tests/norm_ref64 to float64 torch).  d(residual) is gy bit for bit; H * W = 1 gives exactly 0 (+ residual).

  BATCH NORM against float64 nn.BatchNorm2d, the whole chain: the kernel's (mean, rstd) are within (tm, [lo, hi]) of the exact ones, so
  with dr = max(hi - rstd, rstd - lo), d = dr / rstd and c = hi tm
        |xhat_k - xhat| <= apply_tol + |v - mean| dr + c
        y  = xhat w + b:   |w| (that) + 2u (|xhat w| + |y|)                                   (a product and a sum in fp32)
        dx = rstd (g' - m1 - xhat m2):  bwd_terms' tol + rstd [((1 + d)^3 - 1) (|g' - m1| + |xhat m2|) + c (|m2| + |xhat| |m1|) + c^2 |m1|]
        dweight = sum gy xhat: sum |gy| (|xhat_k - xhat|) + BOUND_C sqrt(n) u sum |gy xhat|;   dbias: BOUND_C sqrt(n) u sum |gy|
        running_mean, running_var: m tm, m tv n / (n - 1) per step (+ 4u of the value: the fp32 update), accumulated over the steps.

  Pads, layouts, the residual gradient and everything in the plumbing group are exact (bit for bit).
"""
import math
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd import autograd as AG
from gan_variant_research_amd import ops_library as L
from gan_variant_research_amd._lib import GanError
from gan_variant_research_amd.runtime import cpad
from tests import conv_ref64 as R
from tests import norm_cases as N
from tests import norm_ref64 as NR
from tests.cases import BOUND_C, U_BF16, U_F32, conv_ref64, derived_bound
from tests.conv_cases import Recorder, key_of

U = U_F32
NAME = {BF16: "bf16", F32: "fp32"}
U_OUT = {BF16: U_BF16, F32: U_F32}
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
OPS = torch.ops.mi355x_gan


# ------------------------------------------------------------------------------------------------ recording op layers, compute dtype
class Recording:
    """autograd._OPS_FACTORY for a test: every op layer the library builds is wrapped in a conv_cases.Recorder and kept"""

    def __init__(self, factory):
        self.factory, self.made = factory, []

    def __call__(self, device):
        r = Recorder(self.factory(device))
        self.made.append(r)
        return r


class compute_dtype:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        L.set_compute_dtype(self.dtype)

    def __exit__(self, *a):
        L.set_compute_dtype(F32)


def _gen(*seed):
    return torch.Generator().manual_seed(hash(seed) % (2 ** 31))


def rnd(t, dtype):
    return t.bfloat16().float() if dtype == BF16 else t.float()


def ratio(got, ref, tol):
    r = (got.double().cpu() - ref).abs() / (tol + 1e-300)
    assert not bool(torch.isnan(r).any()), "NaN in a result or its reference"
    return float(r.max()) if r.numel() else 0.0


_worst = {}
_rejecting = []
_done = {}           # (device type, case) -> figures against the honest reference, for the summary (a case runs once per session)


def report(dev, group, dtype, what, figs):
    r = max(figs.values())
    txt = ", ".join(f"{k} {v:.3g}" for k, v in figs.items())
    if _rejecting:
        print(f"[oplib-family] (against the wrong reference {_rejecting[0]}) {group} {NAME[dtype]} {what}: {txt}")
        return r
    k = (dev, group, NAME[dtype])
    _worst[k] = max(_worst.get(k, 0.0), r)
    print(f"[oplib-family] {group:17s} {NAME[dtype]} {what}: error / bound: {txt}   (worst of the group so far {_worst[k]:.3g})")
    return r


# ------------------------------------------------------------------------------------------------ wrong references
class Ref:
    drop_tap = zero_pad = act_from_pre = unbiased = res_grad_masked = last_row_out = False


def _wrong(name, **kw):
    return type(name, (Ref,), kw)


WRONG = [_wrong("TapDropped", drop_tap=True), _wrong("ZeroPaddingForReflect", zero_pad=True), _wrong("ActDerivativeFromThePreActivation", act_from_pre=True),
         _wrong("UnbiasedVariance", unbiased=True), _wrong("ResidualGradientMasked", res_grad_masked=True), _wrong("OddStridedGradientWithoutLastRow", last_row_out=True)]


# ------------------------------------------------------------------------------------------------ convolutions
_ConvT = namedtuple("Conv", "B cin cout H W k s p reflect act bias tr dtype reach")


def Conv(B, cin, cout, H, W, k, s, p, reflect=False, act=ACT_NONE, bias=True, tr=False, dtype=F32, **reach):
    """reach: what the launches planned for the case must be, from the recording layer: fwd / dgrad = (layout, launches)"""
    return _ConvT(B, cin, cout, H, W, k, s, p, reflect, act, bias, tr, dtype, tuple(sorted(reach.items())))


def conv_id(S):
    return (f"{'convT' if S.tr else 'conv'}-B{S.B}-{S.cin}-{S.cout}-{S.H}x{S.W}-k{S.k}s{S.s}p{S.p}{'r' if S.reflect else 'z'}-act{S.act}"
            f"{'' if S.bias else '-nobias'}-{NAME[S.dtype]}")


CONV_F32 = [
    Conv(2, 5, 6, 8, 12, 3, 2, 1), Conv(2, 5, 6, 7, 13, 3, 2, 1),
    Conv(1, 3, 8, 9, 5, 4, 2, 1, act=ACT_LRELU), Conv(1, 3, 8, 10, 6, 4, 2, 1, act=ACT_LRELU),
    Conv(1, 8, 8, 9, 9, 3, 2, 0), Conv(1, 8, 8, 10, 10, 3, 2, 0, bias=False),
    Conv(2, 8, 8, 5, 7, 3, 1, 1, reflect=True, act=ACT_RELU), Conv(1, 4, 3, 9, 8, 7, 1, 3, reflect=True, act=ACT_TANH, bias=False),
    Conv(1, 16, 1, 4, 6, 4, 1, 1), Conv(1, 8, 8, 3, 3, 1, 1, 0), Conv(1, 8, 8, 5, 5, 3, 1, 2), Conv(1, 8, 8, 1, 1, 3, 1, 1),
]
# the epilogue group's geometries (tests/conv_cases.py), so that each case reaches a named kernel: layout 1 range-patch, 2 the 7x7 window, 0 generic
CONV_BF16 = [Conv(3, 64, 128, 6, 11, 3, 1, 1, reflect=True, act=a, dtype=BF16, fwd=(1, 1)) for a in (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH)] + [
    Conv(3, 64, 3, 9, 20, 7, 1, 3, reflect=True, act=ACT_TANH, dtype=BF16, fwd=(2, 1)),
    Conv(3, 3, 64, 17, 33, 7, 1, 3, reflect=True, dtype=BF16, fwd=(2, 1)),
    Conv(3, 64, 128, 7, 13, 3, 2, 1, dtype=BF16, fwd=(1, 1), dgrad=(0, 4)),            # odd, strided: four single phases, never paired
]
CONV_T = [
    Conv(2, 5, 3, 3, 7, 3, 2, 1, act=ACT_RELU, tr=True), Conv(2, 16, 8, 1, 1, 3, 2, 1, bias=False, tr=True),
    Conv(3, 128, 64, 3, 9, 3, 2, 1, tr=True, dtype=BF16, fwd=(1, 2)),                   # the paired phases
    Conv(3, 256, 128, 6, 10, 3, 2, 1, tr=True, dtype=BF16, fwd=(None, 4)),
]
CONVS = CONV_F32 + CONV_BF16 + CONV_T


def conv_operands(S):
    gen = _gen(S.B, S.cin, S.cout, S.H, S.W, S.k, S.s, int(S.tr), 3)
    w = torch.randn((S.cin, S.cout, S.k, S.k) if S.tr else (S.cout, S.cin, S.k, S.k), generator=gen) * (0.5 / (S.cin * S.k * S.k) ** 0.5)
    b = torch.randn(S.cout, generator=gen) * 0.3
    x = torch.randn(S.B, S.cin, S.H, S.W, generator=gen)
    return rnd(x, S.dtype), rnd(w, S.dtype), b, gen


def call_conv(S, x, w, b):
    if S.tr:
        return OPS.conv_transpose2d_fwd(x, w, b, S.act)
    return OPS.conv2d_fwd(x, w, b, S.s, S.p, L.PAD_REFLECT if S.reflect else L.PAD_ZERO, S.act)


def assert_reach(S, recording):
    """the first plan built is the forward call's: its recorder holds the forward launches, then the input gradient's"""
    reach = dict(S.reach)
    if not reach:
        return
    rec = recording.made[0]
    keys = [key_of(rec, c) for c in rec.calls]
    nf = len(keys) - 1 if S.tr else 1            # a transposed layer's input gradient is one strided launch, a regular forward one launch
    parts = {"fwd": keys[:nf], "dgrad": keys[nf:]}
    for name, (layout, n) in reach.items():
        got = parts[name]
        assert len(got) == n, f"{conv_id(S)}: {name} has {len(got)} launches, the case names {n}: {got}"
        assert layout is None or all(k["layout"] == layout for k in got), f"{conv_id(S)}: {name} did not reach layout {layout}: {got}"


def act_bwd_tol(gy64, y64, act, want):
    e = U * (gy64 * NR.act_grad_from_out64(y64, act)).abs()
    e = e + gy64.abs() * U * {ACT_NONE: 0, ACT_RELU: 0, ACT_LRELU: 0.2, ACT_TANH: 2 * (1 + y64 * y64)}[act] + U * want.abs()
    return e + U * (want.abs() + e)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def body_conv(device, S, recording=None, ref=None):
    """one convolution case: y, the activation's backward, dx, dw and db against float64; returns the figures"""
    ref = ref or Ref()
    dev = torch.device(device)
    x, w, b, gen = conv_operands(S)
    u_out = U_OUT[S.dtype]
    with compute_dtype(S.dtype):
        xd, wd = x.to(dev).clone().requires_grad_(True), w.to(dev).clone().requires_grad_(True)
        bd = b.to(dev).clone().requires_grad_(True) if S.bias else None
        y = call_conv(S, xd, wd, bd)
        assert y.dtype == torch.float32 and y.requires_grad
        gy = rnd(torch.randn(y.shape, generator=gen), S.dtype)
        grads = torch.autograd.grad(y, [xd, wd] + ([bd] if S.bias else []), gy.to(dev))
        gpre = OPS.act_bwd(y.detach(), gy.to(dev), S.act).cpu() if S.act != ACT_NONE else gy
    if recording is not None:
        assert_reach(S, recording)
    y_got = y.detach().cpu()
    dx, dw = grads[0].cpu(), grads[1].cpu()
    assert dx.shape == x.shape and dw.shape == w.shape and dx.dtype == dw.dtype == torch.float32
    k, s, p, tr = S.k, S.s, S.p, S.tr
    x64, w64, b64 = x.double(), w.double(), (b.double() if S.bias else None)
    wr = w64
    if ref.drop_tap:
        wr = w64.clone()
        wr[:, :, k - 1, 0] = 0.0
    reflect = S.reflect and not ref.zero_pad
    figs = {}
    # ---- forward
    t, A, K = conv_ref64("fwd", k, s, p, tr, reflect, wr, x=x64)
    if b64 is not None:
        t, A = t + b64.view(1, -1, 1, 1), A + b64.abs().view(1, -1, 1, 1)
    assert y_got.shape == t.shape, (y_got.shape, t.shape)
    tol_y, _ = R.elem_tol(t, A, K, S.act, None, u_out, S.bias)
    figs["y"] = ratio(y_got, R.act64(t, S.act), tol_y)
    # ---- the activation's backward, from the saved output (the header's statement)
    gy64, y64 = gy.double(), y_got.double()
    if S.act != ACT_NONE:
        basis = t if ref.act_from_pre else y64
        want_g = gy64 * NR.act_grad_from_out64(basis, S.act)
        figs["act'"] = ratio(gpre, want_g, act_bwd_tol(gy64, y64, S.act, gy64 * NR.act_grad_from_out64(y64, S.act)))
    gop = rnd(gpre, S.dtype).double()             # the operand the library stages for all three gradients
    # ---- input gradient
    if reflect:
        rp, Ap, Kd = conv_ref64("dgrad", k, s, p, tr, True, wr, dy=gop, x_hw=(S.H, S.W), padded_domain=True)
        tol_p = derived_bound(rp, Ap, Kd, u_out)
        want_dx = _nchw(NR.fold_full64(_nhwc(rp), p))
        n_r = _nchw(NR.fold_full64(torch.ones_like(_nhwc(rp)), p))
        T = _nchw(NR.fold_full64(_nhwc(tol_p), p)) + (n_r + 1) * U * _nchw(NR.fold_full64(_nhwc(rp.abs() + tol_p), p))
        tol_dx = T + u_out * (want_dx.abs() + T)
    else:
        want_dx, Ad, Kd = conv_ref64("dgrad", k, s, p, tr, False, wr, dy=gop, x_hw=(S.H, S.W))
        tol_dx = derived_bound(want_dx, Ad, Kd, u_out)
    if ref.last_row_out and s == 2 and not tr:
        want_dx = want_dx.clone()
        want_dx[:, :, 2 * (S.H // 2):, :] = 0.0
        want_dx[:, :, :, 2 * (S.W // 2):] = 0.0
    figs["dx"] = ratio(dx, want_dx, tol_dx)
    # ---- weight and bias gradient
    rw, Aw, Kw = conv_ref64("wgrad", k, s, p, tr, reflect, wr, x=x64, dy=gop)
    figs["dw"] = ratio(dw, rw, derived_bound(rw, Aw, Kw, 0.0))
    if S.bias:
        db = grads[2].cpu()
        figs["db"] = ratio(db, gop.sum((0, 2, 3)), derived_bound(gop.sum((0, 2, 3)), gop.abs().sum((0, 2, 3)), gop[:, 0].numel(), 0.0))
    group = "conv_transpose2d" if tr else "conv2d"
    report(dev.type, group, S.dtype, conv_id(S), figs)
    if type(ref) is Ref:
        _done[(dev.type, S)] = figs
    bad = {n: v for n, v in figs.items() if not v <= 1.0}
    assert not bad, f"{conv_id(S)}: error / bound {bad}"
    return figs


# ------------------------------------------------------------------------------------------------ instance norm
NORM_SHAPES = [(2, 5, 3, 7), (3, 64, 9, 9), (1, 256, 2, 3), (2, 8, 1, 1)]
NORMS = [(sh, act, res, dt) for sh in NORM_SHAPES for act in (ACT_NONE, ACT_RELU, ACT_LRELU) for res in (False, True) for dt in (F32, BF16)]


def norm_id(p):
    sh, act, res, dt = p
    return "x".join(map(str, sh)) + f"-act{act}-res{int(res)}-{NAME[dt]}"


def norm_operands(shape, dtype, seed=0):
    B, C, H, W = shape
    gen = _gen(B, C, H, W, seed, 17)
    x = torch.randn(shape, generator=gen) * (0.5 + torch.rand(1, C, 1, 1, generator=gen) * 2) + torch.randn(1, C, 1, 1, generator=gen)
    r = torch.randn(shape, generator=gen)
    g = torch.randn(shape, generator=gen) * 0.5
    return rnd(x, dtype), rnd(r, dtype), rnd(g, dtype)


def body_norm(device, shape, act, has_res, dtype, ref=None):
    ref = ref or Ref()
    dev = torch.device(device)
    B, C, H, W = shape
    x, r, g = norm_operands(shape, dtype)
    with compute_dtype(dtype):
        xd = x.to(dev).clone().requires_grad_(True)
        rd = r.to(dev).clone().requires_grad_(True) if has_res else None
        y, stats = OPS.instance_norm_fwd(xd, 1e-5, act, rd)
        grads = torch.autograd.grad(y, [xd] + ([rd] if has_res else []), g.to(dev))
    what = norm_id((shape, act, has_res, dtype))
    assert y.dtype == torch.float32 and stats.shape == (B * cpad(C) * 2,) and stats.dtype == torch.float32
    st = stats.detach().cpu().view(B, cpad(C), 2)[:, :C].double()
    v = _nhwc(x.double())
    figs = {}
    # ---- the returned statistics against float64 sums
    mean, var, rstd, tm, tv, lo, hi, well = N.stats_tol(v)
    assert H * W == 1 or bool(well.all()), f"{what}: the data is meant to be well conditioned"
    up, dn = hi - rstd, rstd - lo
    if ref.unbiased:
        rstd = 1.0 / torch.sqrt(var * (H * W) / max(H * W - 1, 1) + NR.EPS64)
    gm, gr = st[..., 0], st[..., 1]
    figs["mean"] = ratio(gm, mean, tm)
    figs["rstd"] = float(torch.where(gr >= rstd, (gr - rstd) / (up + 1e-300), (rstd - gr) / (dn + 1e-300)).max())
    # ---- y and dx given those statistics (the norm family's statement)
    u_out = U_OUT[dtype]
    r64 = _nhwc(r.double()) if has_res else None
    want = NR.apply64(v, gm, gr, act, r64)
    figs["y"] = ratio(_nhwc(y.detach().cpu()), want, N.apply_tol(v, gm, gr, act, r64, want, u_out))
    if H * W == 1:
        assert torch.equal(y.detach().cpu(), r if has_res else torch.zeros(shape)), f"{what}: one pixel must give exactly 0 (+ residual)"
    g64 = _nhwc(g.double())
    res = {"x64": v, "dtype": dtype, "st64": st, "shape": (B, H, W, C, 0), "g64": g64, "gview": N.Geo(B, H, W, C, 0, H, W), "a64": None}
    want_dx, tol_dx, _ = N.bwd_terms(res, act, N.Ref(), False)
    figs["dx"] = ratio(_nhwc(grads[0].cpu()), want_dx, tol_dx)
    if has_res:
        want_r = g * NR.act_grad_from_out64(y.detach().cpu().double() - r.double(), act).float() if ref.res_grad_masked else g
        assert torch.equal(grads[1].cpu(), want_r), f"{what}: d(residual) is not gy bit for bit"
    report(dev.type, "instance_norm", dtype, what, figs)
    if type(ref) is Ref:
        _done[(dev.type, (shape, act, has_res, dtype))] = figs
    bad = {n: f for n, f in figs.items() if not f <= 1.0}
    assert not bad, f"{what}: error / bound {bad}"
    return figs


# ------------------------------------------------------------------------------------------------ act_bwd
def body_act_bwd(device):
    """relu, lrelu and tanh from the OUTPUT y on 0.0, -0.0, +-1e-30, +-0.5 and 1.0 against the header's statement; a NaN in g stays a NaN"""
    dev = torch.device(device)
    yv = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 1.0], dtype=torch.float32)
    y = yv.view(1, 1, 1, 7).repeat(2, 3, 2, 1).contiguous()
    g = torch.randn(y.shape, generator=_gen(5)) + 2.0
    gn = g.clone()
    gn[0, 1, 0, 4], gn[1, 2, 1, 5], gn[0, 0, 1, 0] = float("nan"), float("nan"), float("nan")
    figs = {}
    for act in (ACT_RELU, ACT_LRELU, ACT_TANH):
        got = OPS.act_bwd(y.to(dev), g.to(dev), act).cpu()
        y64, g64 = y.double(), g.double()
        want = g64 * NR.act_grad_from_out64(y64, act)             # y > 0 ? 1 : 0 | y > 0 ? 1 : 0.2 | 1 - y^2
        figs[f"act{act}"] = ratio(got, want, act_bwd_tol(g64, y64, act, want))
        if act == ACT_RELU:
            assert torch.equal(got, (g * (y > 0)).float()), "act_bwd relu is g or 0 exactly"
        gotn = OPS.act_bwd(y.to(dev), gn.to(dev), act).cpu()
        assert bool(torch.isnan(gotn[torch.isnan(gn)]).all()), f"act_bwd act {act}: a NaN in g did not stay a NaN"
        assert torch.equal(gotn[~torch.isnan(gn)], got[~torch.isnan(gn)]), f"act_bwd act {act}: a NaN in g reached another element"
    report(dev.type, "act_bwd", F32, "7 values x 12", figs)
    _done[(dev.type, "act_bwd")] = figs
    assert max(figs.values()) <= 1.0, figs
    return figs


# ------------------------------------------------------------------------------------------------ pads (exact)
def body_pads(device):
    from tests.test_ops_library import pad_op_cases
    pad_op_cases(device)
    dev = torch.device(device)
    for (shape, pad), modes in ((((1, 1, 2, 2), 1), ("replicate", "reflect")), (((2, 3, 4, 6), 3), ("reflect",)), (((1, 8, 5, 3), 2), ("reflect",))):
        for mode in modes:          # reflect with pad = min(H, W) - 1: every interior pixel but the last is a pre-image
            name = "replication_pad2d" if mode == "replicate" else "reflection_pad2d"
            x = torch.randn(shape, generator=_gen(pad, 9)).to(dev).requires_grad_(True)
            y = getattr(OPS, name)(x, pad)
            assert torch.equal(y.detach().cpu(), F.pad(x.detach().cpu(), (pad,) * 4, mode=mode)), (name, shape, pad)
            wv = torch.randn(y.shape, generator=_gen(pad, 10))
            gx, = torch.autograd.grad(y, x, wv.to(dev))

            def fold(g64):          # the padding is linear: its gradient is the fold of the upstream gradient, whatever x
                z = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
                return torch.autograd.grad(F.pad(z, (pad,) * 4, mode=mode), z, g64)[0]
            # an fp32 sum of n pre-images: (n - 1) u sum|terms| (tests/norm_cases.py, FOLD); one pre-image: exact
            tol = (fold(torch.ones(y.shape, dtype=torch.float64)) - 1) * U * fold(wv.double().abs())
            assert ratio(gx, fold(wv.double()), tol) <= 1.0, (name, shape, pad)
    for shape, pad in (((1, 3, 4, 6), 4), ((1, 3, 6, 3), 3), ((1, 1, 1, 1), 1)):       # refused on the host, before any launch
        with pytest.raises((AssertionError, RuntimeError)):
            OPS.reflection_pad2d(torch.zeros(shape, device=dev), pad)


# ------------------------------------------------------------------------------------------------ BatchNorm2d
def body_batchnorm(device, momentum):
    """the drop-in BatchNorm2d against float64 nn.BatchNorm2d on (3, 5, 4, 6): two training steps, then eval"""
    dev = torch.device(device)
    shape = (3, 5, 4, 6)
    B, C, H, W = shape
    n = B * H * W
    gen = _gen(11, 0 if momentum is None else 1)
    mod, refm = L.BatchNorm2d(C, momentum=momentum).to(dev), nn.BatchNorm2d(C, momentum=momentum).double()
    wv, bv = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    with torch.no_grad():
        mod.weight.copy_(wv); mod.bias.copy_(bv); refm.weight.copy_(wv); refm.bias.copy_(bv)
    figs = {}
    tol_rm, tol_rv = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for step in range(2):
        x = torch.randn(shape, generator=gen) * (0.5 + torch.rand(1, C, 1, 1, generator=gen)) + torch.randn(1, C, 1, 1, generator=gen)
        gy = torch.randn(shape, generator=gen)
        xd = x.to(dev).clone().requires_grad_(True)
        y = mod(xd)
        dx, dwt, dbs = torch.autograd.grad(y, [xd, mod.weight, mod.bias], gy.to(dev))
        xr = x.double().requires_grad_(True)
        yr = refm(xr)
        dxr, dwr, dbr = torch.autograd.grad(yr, [xr, refm.weight, refm.bias], gy.double())
        # the batch as ONE instance (1, B*H, W, C) of the norm family's statement
        v = x.double().permute(1, 0, 2, 3).reshape(1, C, B * H, W).permute(0, 2, 3, 1).contiguous()
        g1 = (gy * wv.view(1, C, 1, 1)).double().permute(1, 0, 2, 3).reshape(1, C, B * H, W).permute(0, 2, 3, 1).contiguous()      # gy * w, rounded once in fp32
        gyv = gy.double().permute(1, 0, 2, 3).reshape(1, C, B * H, W).permute(0, 2, 3, 1).contiguous()
        mean, var, rstd, tm, tv, lo, hi, well = N.stats_tol(v)
        assert bool(well.all())
        bc = lambda t_: t_[:, None, None, :]
        dr = torch.maximum(hi - rstd, rstd - lo)
        d, c = dr / rstd, hi * tm
        xh = (v - bc(mean)) * bc(rstd)
        e_xh = N.apply_tol(v, mean, rstd, ACT_NONE, None, xh, U) + (v - bc(mean)).abs() * bc(dr) + bc(c)
        w64 = wv.double().view(1, 1, 1, C)
        back = lambda t_: t_[0].permute(2, 0, 1).reshape(C, B, H, W).permute(1, 0, 2, 3)        # (1, B*H, W, C) -> (B, C, H, W)
        tol_y = w64.abs() * e_xh + 2 * U * ((xh * w64).abs() + (xh * w64 + bv.double().view(1, 1, 1, C)).abs())
        figs[f"y{step}"] = ratio(y.detach(), yr.detach(), back(tol_y))
        res = {"x64": v, "dtype": F32, "st64": torch.stack([mean, rstd], -1), "shape": (1, B * H, W, C, 0), "g64": g1, "gview": N.Geo(1, B * H, W, C, 0, B * H, W), "a64": None}
        want_dx, tol_dx, _ = N.bwd_terms(res, ACT_NONE, N.Ref(), False)
        m1, m2 = g1.mean((1, 2)), (g1 * xh).mean((1, 2))
        prop = bc(rstd) * ((((1 + bc(d)) ** 3 - 1) * ((g1 - bc(m1)).abs() + (xh * bc(m2)).abs())) + bc(c) * (bc(m2.abs()) + xh.abs() * bc(m1.abs())) + bc(c * c * m1.abs()))
        # the product gy * w is itself rounded once in fp32 (the float64 module does not round it): u |g'| on every element and in both means
        tol_dx = tol_dx + prop + U * bc(rstd) * (g1.abs() + bc(g1.abs().mean((1, 2))) + xh.abs() * bc((g1 * xh).abs().mean((1, 2))))
        figs[f"dx{step}"] = ratio(dx, dxr, back(tol_dx))
        k = BOUND_C * math.sqrt(n) * U
        figs[f"dweight{step}"] = ratio(dwt, dwr, ((gyv.abs() * e_xh).sum((0, 1, 2)) + k * (gyv * xh).abs().sum((0, 1, 2)) + U * dwr.abs()))
        figs[f"dbias{step}"] = ratio(dbs, dbr, k * gyv.abs().sum((0, 1, 2)) + U * dbr.abs())
        # running statistics: the unbiased batch variance, momentum m (None: the cumulative average 1 / (step + 1))
        m = momentum if momentum is not None else 1.0 / (step + 1)
        tol_rm = (1 - m) * tol_rm + m * tm[0] + 4 * U * refm.running_mean.abs()
        # var from the stored rstd: 1 / rstd^2 - eps, the rstd interval mapped back (2 dr / rstd^3) on top of tol(var)
        tol_rv = (1 - m) * tol_rv + m * (n / (n - 1)) * (tv[0] + 2 * dr[0] / rstd[0] ** 3 + 8 * U * (var[0] + NR.EPS64)) + 4 * U * refm.running_var.abs()
        figs[f"running_mean{step}"] = ratio(mod.running_mean, refm.running_mean, tol_rm)
        figs[f"running_var{step}"] = ratio(mod.running_var, refm.running_var, tol_rv)
        assert int(mod.num_batches_tracked) == int(refm.num_batches_tracked) == step + 1
    mod.eval(); refm.eval()
    with torch.no_grad():
        ye, yer = mod(x.to(dev)), refm(x.double())
    sc = refm.weight.detach() / torch.sqrt(refm.running_var + refm.eps)
    tol_e = (x.double() - refm.running_mean.view(1, C, 1, 1)).abs() * (sc * (tol_rv / (2 * (refm.running_var + refm.eps)) + 4 * U)).view(1, C, 1, 1) \
        + (sc * tol_rm).view(1, C, 1, 1) + 4 * U * ((x.double() * sc.view(1, C, 1, 1)).abs() + (refm.running_mean * sc).abs().view(1, C, 1, 1) + refm.bias.detach().abs().view(1, C, 1, 1))
    figs["eval"] = ratio(ye, yer, tol_e)
    assert int(mod.num_batches_tracked) == 2
    report(dev.type, "batch_norm", F32, f"momentum {momentum}", figs)
    _done[(dev.type, "batch_norm", momentum)] = figs
    bad = {n_: f for n_, f in figs.items() if not f <= 1.0}
    assert not bad, f"BatchNorm2d momentum {momentum}: error / bound {bad}"
    return figs


# ------------------------------------------------------------------------------------------------ autograd plumbing (exact)
P_CONV = Conv(2, 8, 8, 6, 5, 3, 1, 1, act=ACT_LRELU)
P_CONVT = Conv(2, 8, 8, 3, 4, 3, 2, 1, act=ACT_RELU, tr=True)


def _forms(x32):
    """the same float32 values handed over in other forms: (name, tensor, dtype of the gradient)"""
    big = torch.zeros(x32.shape[0], x32.shape[1], x32.shape[2] * 2, x32.shape[3] + 3, dtype=torch.float32, device=x32.device)
    big[:, :, ::2, 2:-1] = x32
    return [("channels_last", x32.contiguous(memory_format=torch.channels_last), torch.float32), ("strided slice", big[:, :, ::2, 2:-1], torch.float32),
            ("bfloat16", x32.bfloat16(), torch.bfloat16), ("float64", x32.double(), torch.float64)]


def body_plumbing(device):
    dev = torch.device(device)
    # ---- convolutions: gradient subsets, input forms
    for S in (P_CONV, P_CONVT):
        x, w, b, gen = conv_operands(S)
        x = x.bfloat16().float()                                       # representable in every form below
        xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
        y = call_conv(S, xd, wd, bd)
        gy = torch.randn(y.shape, generator=gen).to(dev)
        full = torch.autograd.grad(y, [xd, wd, bd], gy)
        for i, name in enumerate(("x", "w", "bias")):
            leaves = [t.detach().clone().requires_grad_(i == j) for j, t in enumerate((xd, wd, bd))]
            y1 = call_conv(S, *leaves)
            assert torch.equal(y1, y), f"{conv_id(S)}: the forward depends on which input requires a gradient"
            g1, = torch.autograd.grad(y1, leaves[i], gy)
            assert torch.equal(g1, full[i]), f"{conv_id(S)}: the gradient for {name} alone differs from the one taken with the others"
        for name, xf, gdt in _forms(x.to(dev)):
            xf = xf.detach().requires_grad_(True)
            assert name in ("bfloat16", "float64") or not xf.is_contiguous()
            y1 = call_conv(S, xf, wd, bd)
            assert y1.dtype == torch.float32 and torch.equal(y1, y), f"{conv_id(S)}: x as {name}: another result"
            gx, gw = torch.autograd.grad(y1, [xf, wd], gy)
            assert gx.dtype == gdt and torch.equal(gx, full[0].to(gdt)) and torch.equal(gw, full[1]), f"{conv_id(S)}: x as {name}: another gradient"
    # ---- instance norm: gradient for x alone / the residual alone, input forms
    shape = (2, 8, 5, 4)
    x, r, g = (t.to(dev) for t in norm_operands(shape, BF16))
    xd, rd = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    y, st = OPS.instance_norm_fwd(xd, 1e-5, ACT_RELU, rd)
    full = torch.autograd.grad(y, [xd, rd], g)
    for i in range(2):
        leaves = [t.detach().clone().requires_grad_(i == j) for j, t in enumerate((xd, rd))]
        y1, st1 = OPS.instance_norm_fwd(leaves[0], 1e-5, ACT_RELU, leaves[1])
        g1, = torch.autograd.grad(y1, leaves[i], g)
        assert torch.equal(y1, y) and torch.equal(st1, st) and torch.equal(g1, full[i])
    for name, xf, gdt in _forms(x):
        xf = xf.detach().requires_grad_(True)
        y1, st1 = OPS.instance_norm_fwd(xf, 1e-5, ACT_RELU, rd)
        gx, = torch.autograd.grad(y1, xf, g)
        assert y1.dtype == torch.float32 and torch.equal(y1, y) and torch.equal(st1, st), f"instance_norm_fwd: x as {name}: another result"
        assert gx.dtype == gdt and torch.equal(gx, full[0].to(gdt)), f"instance_norm_fwd: x as {name}: another gradient"
    # ---- two layers of one geometry (one plan) and different weights in one graph: c(c(x, w1), w2) + c(x, w2), backward once, against the
    #      same chain walked by hand through the functional ops.  Nothing a backward needs may live in the plan's staging buffers.
    S = P_CONV
    x, w1, b1, gen = conv_operands(S)
    w2, b2 = torch.randn(w1.shape, generator=gen) * 0.2, torch.randn(b1.shape, generator=gen)
    x, w1, b1, w2, b2 = (t.to(dev).requires_grad_(True) for t in (x, w1, b1, w2, b2))
    c = lambda a, w_, b_: OPS.conv2d_fwd(a, w_, b_, S.s, S.p, L.PAD_ZERO, S.act)
    y1 = c(x, w1, b1)
    out = c(y1, w2, b2) + c(x, w2, b2)
    gy = torch.randn(out.shape, generator=gen).to(dev)
    gx, gw1, gb1, gw2, gb2 = torch.autograd.grad(out, [x, w1, b1, w2, b2], gy)
    with torch.no_grad():
        xs, shp, wsh = x.detach(), list(x.shape), list(w1.shape)
        y1h = c(xs, w1, b1)
        y2h, y3h = c(y1h, w2, b2), c(xs, w2, b2)
        assert torch.equal(out, y2h + y3h)
        ga, gb_ = OPS.act_bwd(y2h, gy, S.act), OPS.act_bwd(y3h, gy, S.act)
        d_y1 = OPS.act_bwd(y1h, OPS.conv2d_dgrad(ga, w2, shp, S.s, S.p, L.PAD_ZERO), S.act)
        hw2a, hb2a = OPS.conv2d_wgrad(y1h, ga, wsh, True, S.s, S.p, L.PAD_ZERO)
        hw2b, hb2b = OPS.conv2d_wgrad(xs, gb_, wsh, True, S.s, S.p, L.PAD_ZERO)
        hw1, hb1 = OPS.conv2d_wgrad(xs, d_y1, wsh, True, S.s, S.p, L.PAD_ZERO)
        hx = OPS.conv2d_dgrad(d_y1, w1, shp, S.s, S.p, L.PAD_ZERO) + OPS.conv2d_dgrad(gb_, w2, shp, S.s, S.p, L.PAD_ZERO)
    for name, a, h in (("dx", gx, hx), ("dw1", gw1, hw1), ("db1", gb1, hb1), ("dw2", gw2, hw2a + hw2b), ("db2", gb2, hb2a + hb2b)):
        assert torch.equal(a, h), f"two layers sharing a plan: {name} differs from the chain walked by hand"
    # ... and against float64 torch: fp32 mode, 72-term sums of O(1) values: far inside 1e-4 of the largest element, where a stale staging buffer is O(1)
    f64 = lambda t_: t_.detach().cpu().double().requires_grad_(True)
    X, W1, B1, W2, B2 = (f64(t_) for t_ in (x, w1, b1, w2, b2))
    cr = lambda a, w_, b_: F.leaky_relu(F.conv2d(a, w_, b_, stride=S.s, padding=S.p), 0.2)
    refs = torch.autograd.grad(cr(cr(X, W1, B1), W2, B2) + cr(X, W2, B2), [X, W1, B1, W2, B2], gy.cpu().double())
    for name, a, h in zip(("dx", "dw1", "db1", "dw2", "db2"), (gx, gw1, gb1, gw2, gb2), refs):
        assert float((a.cpu().double() - h).abs().max()) <= 1e-4 * float(h.abs().max()), f"two layers sharing a plan: {name} against float64 torch"


# ------------------------------------------------------------------------------------------------ registration (emulator only)
def opcheck_args():
    """(op name, args, utilities) for every op of the library"""
    import os
    from gan_variant_research_amd import cut as CUT
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cut_losses.npz"))
    t = lambda *s: torch.randn(*s, generator=_gen(*s))
    rq = lambda *s: t(*s).requires_grad_(True)
    aug = CUT.DiffAugment(["color", "translation", "cutout"])
    torch.manual_seed(0)
    prm = aug.to_params(aug.sample(2, 16, 16, None), 2, 16, 16)
    both = ("test_schema", "test_autograd_registration")
    ps = [t(4, 3), t(5)]
    z = lambda: [torch.zeros_like(p) for p in ps]
    return [
        ("conv2d_fwd", (rq(1, 4, 5, 7), rq(6, 4, 3, 3), rq(6), 2, 1, 0, ACT_LRELU), both),
        ("conv2d_fwd", (rq(1, 4, 5, 6), rq(6, 4, 3, 3), None, 1, 1, 1, ACT_NONE), both),
        ("conv2d_dgrad", (t(1, 6, 3, 4), t(6, 4, 3, 3), [1, 4, 5, 7], 2, 1, 0), both),
        ("conv2d_wgrad", (t(1, 4, 5, 7), t(1, 6, 3, 4), [6, 4, 3, 3], True, 2, 1, 0), both),
        ("conv_transpose2d_fwd", (rq(1, 4, 3, 5), rq(4, 6, 3, 3), rq(6), ACT_RELU), both),
        ("conv_transpose2d_dgrad", (t(1, 6, 6, 10), t(4, 6, 3, 3), [1, 4, 3, 5]), both),
        ("conv_transpose2d_wgrad", (t(1, 4, 3, 5), t(1, 6, 6, 10), [4, 6, 3, 3], False), both),
        ("instance_norm_fwd", (rq(2, 5, 3, 4), 1e-5, ACT_RELU, rq(2, 5, 3, 4)), both),
        ("instance_norm_bwd", (t(2, 5, 3, 4), torch.rand(2 * 8 * 2) + 0.5, t(2, 5, 3, 4), ACT_RELU), both),
        ("reflection_pad2d", (rq(1, 3, 4, 5), 2), both), ("reflection_pad2d_bwd", (t(1, 3, 8, 9), 2), both),
        ("replication_pad2d", (rq(1, 3, 4, 5), 2), both), ("replication_pad2d_bwd", (t(1, 3, 8, 9), 2), both),
        ("act_bwd", (t(1, 3, 4, 5), t(1, 3, 4, 5), ACT_TANH), both),
        ("patchnce_fwd", (torch.tensor(g["nce.a.src"]), torch.tensor(g["nce.a.tgt"]).requires_grad_(True), torch.tensor(g["nce.a.ids"]), 0.07), both),
        ("patchnce_bwd", (torch.tensor(g["nce.a.tgt"]), torch.tensor(2.0)), both),
        ("diffaugment_fwd", (rq(2, 3, 16, 16), prm), both), ("diffaugment_bwd", (t(2, 3, 16, 16), prm), both),
        ("palette_stats", (torch.rand(2, 3, 16, 16) * 2 - 1, 4), both),
        ("palette_prior_fwd", ((torch.rand(2, 3, 16, 16) * 2 - 1).requires_grad_(True), torch.rand(3, 2), 4), both),
        ("palette_prior_bwd", (t(2, 3, 16, 16), torch.tensor(2.0)), both),
        ("allreduce_bucket_", (torch.arange(8, dtype=torch.float32), ""), ("test_schema",)),
        ("fused_clip_adam_ema_", (ps, [t(4, 3), t(5)], z(), z(), [p.clone() for p in ps], torch.zeros(2, dtype=torch.int32), 2e-4, 0.5, 0.999, 1e-8, 10.0, 1.0, 0.999),
         ("test_schema",)),
    ]


# ------------------------------------------------------------------------------------------------ the assertions bite
REJECT_ON = {
    "TapDropped": [("conv", CONV_F32[1]), ("conv", CONV_F32[7]), ("conv", CONV_BF16[0]), ("conv", CONV_T[0])],
    "ZeroPaddingForReflect": [("conv", CONV_F32[6]), ("conv", CONV_BF16[0]), ("conv", CONV_BF16[5])],
    "ActDerivativeFromThePreActivation": [("conv", CONV_F32[7]), ("conv", CONV_BF16[3]), ("conv", CONV_BF16[4])],
    "UnbiasedVariance": [("norm", ((2, 5, 3, 7), ACT_NONE, False, F32)), ("norm", ((3, 64, 9, 9), ACT_RELU, True, BF16)), ("norm", ((1, 256, 2, 3), ACT_LRELU, False, F32))],
    "ResidualGradientMasked": [("norm", ((2, 5, 3, 7), ACT_RELU, True, F32)), ("norm", ((3, 64, 9, 9), ACT_LRELU, True, BF16))],
    "OddStridedGradientWithoutLastRow": [("conv", CONV_F32[1]), ("conv", CONV_F32[2]), ("conv", CONV_F32[4]), ("conv", CONV_BF16[6])],
}


def rejects(device, wrong, reset):
    """every case listed for `wrong` passes against the honest reference and fails against the wrong one"""
    failed = []
    for kind, case in REJECT_ON[wrong.__name__]:
        run = (lambda ref: body_conv(device, case, None, ref)) if kind == "conv" else (lambda ref: body_norm(device, *case, ref=ref))
        if (torch.device(device).type, case) not in _done:
            reset()
            run(None)
        _rejecting.append(wrong.__name__)
        try:
            reset()
            run(wrong())
        except AssertionError as e:
            failed.append((conv_id(case) if kind == "conv" else norm_id(case), str(e)[:100]))
        finally:
            _rejecting.clear()
    print(f"[oplib-family] {wrong.__name__} rejected on {failed}")
    assert len(failed) == len(REJECT_ON[wrong.__name__]), f"the assertions accept the wrong reference {wrong.__name__} on a case it was tried on: {failed}"


# ------------------------------------------------------------------------------------------------ the ratio report
BOUNDED_GROUPS = [("conv2d", F32), ("conv2d", BF16), ("conv_transpose2d", F32), ("conv_transpose2d", BF16), ("instance_norm", F32), ("instance_norm", BF16),
                  ("act_bwd", F32), ("batch_norm", F32)]


def summary(device, reset):
    """runs every bounded case that has no figure yet and reports the worst error / bound per group and dtype; a group below 0.01 is
    held by a bound that catches nothing and fails.  The exact groups (pads, plumbing, residual gradient) have no figure."""
    dev = torch.device(device).type
    todo = [(S, lambda S=S: body_conv(device, S)) for S in CONVS] + [(p, lambda p=p: body_norm(device, *p)) for p in NORMS]
    todo += [("act_bwd", lambda: body_act_bwd(device))] + [(("batch_norm", m), lambda m=m: body_batchnorm(device, m)) for m in (0.1, None)]
    for key, run in todo:
        if ((dev,) + key if isinstance(key, tuple) and key[0] == "batch_norm" else (dev, key)) in _done:
            continue
        reset()
        try:
            run()
        except AssertionError as e:       # each case is a test of its own: a miss fails there and is only listed here
            print(f"[oplib-family] SUMMARY MISS {str(e)[:200]}")
    for group, dt in BOUNDED_GROUPS:
        k = (dev, group, NAME[dt])
        assert k in _worst, f"no figure for {k}"
        print(f"[oplib-family] SUMMARY {dev} {group} {NAME[dt]}: worst error / bound = {_worst[k]:.3g}")
    idle = [k for k in ((dev, g_, NAME[dt]) for g_, dt in BOUNDED_GROUPS) if not 0.01 <= _worst[k] <= 1.0]
    assert not idle, f"groups outside [0.01, 1] of their bound: {[(k, _worst[k]) for k in idle]}"
    return {k: v for k, v in _worst.items() if k[0] == dev}
