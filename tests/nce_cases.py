"""TEST INFRASTRUCTURE: cases, derived bounds and assertions for the PatchNCE kernels of csrc/patchnce.hip, written against an op layer:
tests/test_nce_family_cpu.py runs them on the emulator (loss and gtgt), tests/test_nce_family_gpu.py on HipOps (the workspace
intermediates as well), with the same shapes and the same assertions.  The float64 statement is tests/nce_ref64.py.

Bounds (convention of tests/cases.py: BOUND_C, U_BF16, U_F32 = 2^-24 =: u; an fp32 sum of K terms errs by at most k(K) = BOUND_C sqrt(K) u
times the sum of the absolute terms).  Inputs are exact (the stored values).  None of the bounds is fitted to a result.

  NORMALISED ROWS.  ss = sum of C squares in fp32, all terms positive: relative error k(C) + u (the squares' own rounding); the square root
  halves it and is itself within 2u, so the stored norm is within  e_n = (k(C) + u) / 2 + 2u  (relative);  the division adds 2u:
        tol(tnorm) = e_n tnorm,        tol(Sn), tol(Tn) = e_r |.|,   e_r = e_n + 2u
  In the eps branch the divisor is the constant 1e-6f: e_r is then generous.

  LOGIT.  A dot product of C exact fp32 products (MFMA and fma both round only the accumulation): k(C) A, A = sum_c |t_c s_c| <= 1; the
  error of the two normalised rows enters as (2 e_r + e_r^2) A; then * (1/T): 1.f / T and the product, and T itself held as a float, 3u:
        tol(raw) = A (k(C) + 2 e_r + e_r^2) / T + 3u |raw|
  The clamp is 1-Lipschitz: tol(lg) = tol(raw) where |raw| < 50 and 0 where it is clamped.  CONDITION (asserted by the case builder):
  no raw logit lies within tol(raw) of +50 or -50 -- the mask is a branch, an entry at the boundary cannot be held to either side.

  LSE.  lse = mx + logf(sum_j expf(lg_j - mx)) is 1-Lipschitz in the max-norm of the row's logits: E_i = max_j tol(lg_ij).  expf and logf
  within 2 ulp (4u relative); the subtraction lg_j - mx rounds by u |lg_j - mx|, which enters exp relatively; a sum of P positive terms:
        tol(lse) = E_i + sum_j p_j (4u + u |lg_j - mx|) + k(P) + 4u |lse - mx| + u |lse|                     (p = softmax of the row)
  ROW LOSS.  A difference of two such quantities, so absolute:  tol(rowloss) = tol(lse) + tol(lg_ii) + u |rowloss|.
  LOSS.  Image mean: tol(per) = mean tol(rowloss) + k(P) mean|rowloss| + u |per|;  sum over B images in order, / B, * weight:
        tol(inc) = |weight| sum_b tol(per_b) / B + (k(B) + 3u) |inc|,      tol(loss) = tol(inc) + u |prior + inc|     (the += rounds once)

  dLOGITS (the kernels fold weight / (P B T) into them).  p = expf(lg - lse): exp has Lipschitz constant p <= 1, so
        tol(p) = p (tol(lg) + tol(lse) + u |lg - lse| + 4u),      tol(d) = sc (tol(p) + u |p - [i=j]|) + 5u |d|,   sc = |weight| / (P B T)
  (5u: weight * flag * (1/T) / (P * B) and the product); exactly 0 where the clamp is active and for a flag-0 image.
  dTn = sum over P terms:    tol(g) = tol(d) . |Sn| + (|d| . |Sn|) (e_r + k(P))
  PROJECTION AND DIVISION.  dot = <Tn, g>:  tol(dot) = sum_c (|Tn| tol(g) + e_r |Tn g|) + k(C) sum_c |Tn g|;
        tol(dX) = [tol(g) + |Tn| tol(dot) + (e_r + 2u) |Tn dot| + u (|g| + |Tn dot|)] / tnorm + (e_n + 2u) |dX|         (||x|| > eps)
        tol(dX) = tol(g) / eps + 2u |dX|                                                      (eps branch: the factor is 1e6 and the bound scales with it)
  CONDITION: no row norm of source or target lies within e_n of eps.
  SCATTER.  One lane adds the n duplicate rows in order, then the prior, then rounds once to the buffer's dtype (u_out):
        e = sum tol(dX) + n u (|prior| + sum |dX|),        tol(gtgt) = e + u_out (|want| + e) + eta
  UNDERFLOW.  The relative model above holds for normal fp32 numbers only.  With T = 0.01 a row whose diagonal sits at +50 has softmax
  values exp(-100) = 4e-44 elsewhere: d, its products with Sn and everything downstream are subnormal or flushed.  Every fp32 operation
  whose result lies below the smallest normal number eta = 2^-126 may lose all of it (flush to zero) -- an ABSOLUTE error of at most eta
  per operation, whatever the denormal mode: tol(Sn), tol(Tn) += eta;  tol(d) += 2 eta (expf, the scaling);  tol(g) += (P + 1) eta;
  tol(dot) += (C + 1) eta;  the numerator of dX += 3 eta (so 3 eta / tnorm, 1e6 times as much in the eps branch) and its quotient += eta.
  1e-38 is far below any gradient of substance (the smallest |dX| that matters to a bf16 or fp32 gtgt here is 1e-12).

All-equal ids make the rows of an image identical: the softmax is uniform, sum_j dlg_ij = 0 and every gradient row is exactly 0 in float64.
Those runs hold the leader's sum of 256 rows to that 0 and the loss to log P; duplicates with a gradient of substance are in the `dup`
runs (P = 240 and 255 positions on 256 pixels, pairs across the 64-position chunks of the scatter).

Images of a run whose float64 loss is not finite (the non-finite classes) are held to: flag 0, nothing added to the loss, dX rows exactly 0,
their part of gtgt bit for bit the prior.  Their other intermediates hold NaN in the reference and are not compared.
"""
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from tests import nce_ref64 as R
from tests.cases import BOUND_C, U_BF16, U_F32

U = U_F32
TDT = {BF16: torch.bfloat16, F32: torch.float32}
NAME = {BF16: "bf16", F32: "fp32"}
BITS = {BF16: torch.int16, F32: torch.int32}
U_OUT = {BF16: U_BF16, F32: U_F32}
SENT, WS_FILL, IN_HALO = 7.5, 3e5, 3e4       # exact in bf16 and fp32
ETA = 2.0 ** -126                            # the smallest normal fp32 number
GUARD = 256                                  # floats allocated past gan_patchnce_ws_floats
LOSS_PRIOR, WEIGHT = 3.25, 0.25
T_PLAIN, T_CLAMP = 0.07, 0.01

# documented constants of csrc/patchnce.hip
TI, SLAB, MAXP, MAXC, MFMA_MAXC, FIN_B = 16, 32, 256, 512, 256, 256


def k(n):
    return BOUND_C * math.sqrt(n) * U


def cdiv(a, b):
    return -(-a // b)


def t32(T):
    return float(np.float32(T))


# ------------------------------------------------------------------------------------------------ shapes and regimes
# (B, H, W, view C, halo, P, C) and the regime the case names
SHAPES = [
    ((2, 4, 4, 64, 1, 16, 64), dict(path="mfma", idle_waves=3, dead_steps=3, bwd_trips=1)),
    ((2, 7, 7, 192, 1, 48, 192), dict(path="mfma", nct=3, invalid_col_tiles=13, dead_steps=1)),
    ((2, 5, 13, 128, 0, 80, 128), dict(path="mfma", bwd_trips=2, last_trip_steps=1, nonsquare=True)),
    ((1, 16, 16, 256, 1, 256, 256), dict(path="mfma", nct=4, fwd_trips=4, bwd_trips=4, dead_steps=0)),
    ((2, 16, 16, 64, 1, 240, 64), dict(path="mfma", invalid_col_tiles=1, dead_steps=1, bwd_trips=4)),
    ((2, 6, 6, 128, 1, 32, 64), dict(path="mfma", view_wider=True)),
    ((2, 3, 3, 8, 1, 1, 8), dict(path="scalar", row_tiles=1, last_tile_rows=1)),
    ((2, 5, 5, 64, 1, 17, 64), dict(path="scalar", row_tiles=2, last_tile_rows=1, mfma_c=True)),
    ((2, 10, 10, 40, 0, 100, 40), dict(path="scalar", slab_tail=8, slabs=2)),
    ((2, 16, 16, 8, 3, 255, 8), dict(path="scalar", last_tile_rows=15, slab_tail=8)),
    ((1, 16, 16, 512, 1, 256, 512), dict(path="scalar", vals=8, ti_c=8192)),
    ((2, 8, 8, 320, 1, 64, 320), dict(path="scalar", mfma_p=True, c_mult64=True, vals=5)),
    ((257, 2, 2, 8, 0, 4, 8), dict(path="scalar", fin_trips=2, flag_pad=3)),
    ((5, 4, 4, 16, 1, 8, 16), dict(path="scalar", flag_pad=3)),
]
NF_SHAPES = [((3, 6, 6, 128, 1, 32, 64), dict(path="mfma", view_wider=True)), ((5, 4, 4, 16, 1, 8, 16), dict(path="scalar", flag_pad=3))]
REGIME = dict(SHAPES + NF_SHAPES)


def regime(shape):
    B, H, W, Cv, halo, P, C = shape
    mfma = C % 64 == 0 and C <= MFMA_MAXC and P % TI == 0 and P <= MAXP
    g = dict(path="mfma" if mfma else "scalar", row_tiles=cdiv(P, TI), last_tile_rows=P - TI * (cdiv(P, TI) - 1), fin_trips=cdiv(B, FIN_B),
             flag_pad=cdiv(B, 4) * 4 - B, view_wider=Cv > C, nonsquare=H != W, mfma_c=C % 64 == 0 and C <= MFMA_MAXC, mfma_p=P % TI == 0,
             c_mult64=C % 64 == 0, slabs=cdiv(C, SLAB), slab_tail=C % SLAB, vals=cdiv(C, 64), ti_c=TI * C)
    if mfma:
        g.update(idle_waves=4 - cdiv(P, 64), invalid_col_tiles=16 - P // TI, fwd_trips=C // 64, nct=C // 64, bwd_trips=cdiv(P, 64),
                 last_trip_steps=(P - 64 * (cdiv(P, 64) - 1)) // TI, dead_steps=4 * cdiv(P, 64) - P // TI)
    return g


def check_regime(shape):
    """the case is in the regime it names, from the documented constants of csrc/patchnce.hip and its entry checks"""
    B, H, W, Cv, halo, P, C = shape
    assert 1 <= P <= MAXP and 1 <= C <= MAXC and C <= Cv and TI * C <= 256 * 33
    g = regime(shape)
    for key, want in REGIME[shape].items():
        assert g[key] == want, f"{shape}: {key} = {g[key]}, the case names {want}"
    return g


# ------------------------------------------------------------------------------------------------ runs
# cls: corr | clamp | eps | big | nf_src_inf | nf_tgt_nan | nf_unsampled          ids: dup | perm | equal
Run = namedtuple("Run", "shape dtype cls ids")


def _runs():
    out = []
    for shape, _ in SHAPES:
        for dt in (BF16, F32):
            out += [Run(shape, dt, cls, "dup") for cls in ("corr", "clamp", "eps")]
    for shape in (SHAPES[3][0], SHAPES[10][0], SHAPES[4][0], SHAPES[9][0], SHAPES[8][0]):
        for dt in (BF16, F32):
            out += [Run(shape, dt, "corr", "perm"), Run(shape, dt, "corr", "equal")]
    for shape, _ in NF_SHAPES:
        for dt in (BF16, F32):
            out += [Run(shape, dt, cls, "dup") for cls in ("nf_src_inf", "nf_tgt_nan", "nf_unsampled")]
    for shape in (SHAPES[0][0], SHAPES[13][0]):
        for dt in (BF16, F32):
            out.append(Run(shape, dt, "big", "dup"))
    return out


RUNS = _runs()
BIG_SCALE = 2.0 ** 59          # rows of norm up to ~1e19 / 2: just inside sqrt(sum x^2) < FLT_MAX (||x|| < 1.8e19)


def run_id(r):
    return "x".join(map(str, r.shape)) + f"-{NAME[r.dtype]}-{r.cls}-{r.ids}"


def seed_of(r):
    cls = ["corr", "clamp", "eps", "big", "nf_src_inf", "nf_tgt_nan", "nf_unsampled"].index(r.cls)
    return sum(a * b for a, b in zip(r.shape, (3, 5, 7, 11, 13, 17, 19))) * 31 + cls * 7 + ["dup", "perm", "equal"].index(r.ids) + r.dtype * 1009


def make_ids(r, g):
    B, H, W, Cv, halo, P, C = r.shape
    HW = H * W
    if r.ids == "equal":
        return torch.full((P,), HW - 1, dtype=torch.int64)
    if r.ids == "perm":
        assert P <= HW
        ids = torch.randperm(HW, generator=g)[:P]
        for want, at in ((0, 0), (HW - 1, P - 1)):
            if P >= 2 and want not in ids.tolist():
                ids[at] = want
        assert len(set(ids.tolist())) == P
        return ids
    ids = torch.randint(0, HW, (P,), generator=g)
    if r.cls == "nf_unsampled":          # pixel HW // 2 stays unsampled
        ids[ids == HW // 2] = 1
    for m in range(1, 5):                # the positions the eps class rewrites sample distinct pixels
        if m < P - 1:
            ids[m] = m % (HW - 1)
    ids[0] = 0
    if P >= 2:
        ids[P - 1] = HW - 1
    for m in (64, 128, 192):             # pairs of duplicates straddling the 64-position chunks of the scatter's ballots
        if P > m:
            ids[m] = ids[m - 1]
    return ids


def make_data(r):
    """(src, tgt) interiors (B, H, W, view C) in the buffer's dtype, ids, temperature"""
    B, H, W, Cv, halo, P, C = r.shape
    g = torch.Generator().manual_seed(seed_of(r))
    ids = make_ids(r, g)
    ys, xs = ids // W, ids % W
    src = torch.randn(B, H, W, Cv, generator=g, dtype=torch.float64)
    tgt = src + 0.5 * torch.randn(B, H, W, Cv, generator=g, dtype=torch.float64)
    if (H, W, C) == (16, 16, 8) and halo == 3:          # the layer-0 shape: an image padded to 8 channels
        src[..., 3:C], tgt[..., 3:C] = 0.0, 0.0
    src[1::2] *= 2.0 ** 10                               # the normalisation is scale free
    tgt[1::2] *= 2.0 ** -5
    if r.cls == "big":
        src[0], tgt[0] = src[0] * BIG_SCALE, tgt[0] * BIG_SCALE
    src, tgt = src.to(TDT[r.dtype]), tgt.to(TDT[r.dtype])
    at = lambda m: (ys[m % P], xs[m % P])
    if r.cls == "clamp" and P >= 2:
        for m in (5, 6):
            tgt[:, at(m)[0], at(m)[1]] = -src[:, at(m)[0], at(m)[1]] * (3.0 if m == 5 else 1.0)       # cosine -1: raw = -1 / T
    if r.cls == "eps":
        tiny = lambda: (torch.randn(B, Cv, generator=g, dtype=torch.float64) * (1e-8 / math.sqrt(C))).to(TDT[r.dtype])
        src[:, at(1)[0], at(1)[1]] = 0
        src[:, at(2)[0], at(2)[1]] = tiny()
        tgt[:, at(3)[0], at(3)[1]] = 0
        tgt[:, at(4)[0], at(4)[1]] = tiny()
    if r.cls == "nf_src_inf":
        src[1, at(2)[0], at(2)[1], C // 2] = float("inf")
    if r.cls == "nf_tgt_nan":
        tgt[2, at(3)[0], at(3)[1], 1] = float("nan")
    if r.cls == "nf_unsampled":
        hw = (H * W) // 2
        assert hw not in ids.tolist()
        src[1, hw // W, hw % W, 0] = float("inf")
        tgt[1, hw // W, hw % W, 3] = float("inf")
    return src, tgt, ids, (T_CLAMP if r.cls == "clamp" else T_PLAIN)


# ------------------------------------------------------------------------------------------------ tolerances from the float64 reference
def tolerances(fw, bw, T, weight, prior_loss, live):
    """every tolerance of the module docstring, for the images `live` (an index tensor) of a true reference"""
    Sn, Tn, raw, lg, lse = (fw[n][live] for n in ("Sn", "Tn", "raw", "lg", "lse"))
    tnorm, rowloss, per = fw["tnorm"][live], fw["rowloss"][live], fw["per"][live]
    nB = fw["per"].numel()
    Bl, P, C = Sn.shape
    e_n = (k(C) + U) / 2 + 2 * U
    e_r = e_n + 2 * U
    t = dict(e_n=e_n, e_r=e_r, Sn=e_r * Sn.abs() + ETA, Tn=e_r * Tn.abs() + ETA, tnorm=e_n * tnorm)
    A = torch.bmm(Tn.abs(), Sn.abs().transpose(1, 2))
    t["raw"] = A * (k(C) + 2 * e_r + e_r * e_r) / T + 3 * U * raw.abs()
    clamped = raw.abs() > R.CLAMP
    t["lg"] = torch.where(clamped, torch.zeros_like(raw), t["raw"])
    E = t["lg"].max(2).values
    mx = lg.max(2, keepdim=True).values
    p = torch.exp(lg - lse.unsqueeze(2))
    t["lse"] = E + (p * (4 * U + U * (lg - mx).abs())).sum(2) + k(P) + 4 * U * (lse - mx.squeeze(2)).abs() + U * lse.abs()
    t["rowloss"] = t["lse"] + torch.diagonal(t["lg"], dim1=1, dim2=2) + U * rowloss.abs()
    t["per"] = t["rowloss"].mean(1) + k(P) * rowloss.abs().mean(1) + U * per.abs()
    inc = weight * per.sum() / nB
    t["inc"] = abs(weight) * t["per"].sum() / nB + (k(nB) + 3 * U) * abs(inc)
    t["loss"] = t["inc"] + U * abs(prior_loss + inc)
    dlg, dTn, dX = (v[live] for v in bw)
    d = dlg / T
    sc = abs(weight) / (P * nB * T)
    tp = p * (t["lg"] + t["lse"].unsqueeze(2) + U * (lg - lse.unsqueeze(2)).abs() + 4 * U)
    td = sc * (tp + U * (p - torch.eye(P, dtype=torch.float64)).abs()) + 5 * U * d.abs() + 2 * ETA
    td = torch.where(clamped, torch.zeros_like(td), td)
    tg = torch.bmm(td, Sn.abs()) + torch.bmm(d.abs(), Sn.abs()) * (e_r + k(P)) + (P + 1) * ETA
    dot = (Tn * dTn).sum(2, keepdim=True)
    tdot = (Tn.abs() * tg + e_r * (Tn * dTn).abs()).sum(2, keepdim=True) + k(C) * (Tn * dTn).abs().sum(2, keepdim=True) + (C + 1) * ETA
    nrm = tnorm.unsqueeze(2)
    normal = (tg + Tn.abs() * tdot + (e_r + 2 * U) * (Tn * dot).abs() + U * (dTn.abs() + (Tn * dot).abs()) + 3 * ETA) / nrm + (e_n + 2 * U) * dX.abs()
    t["dX"] = torch.where(nrm > R.EPS, normal, (tg + 3 * ETA) / nrm + 2 * U * dX.abs()) + ETA
    return t


def check_conditions(fw, s_norm, tol, live, what):
    """the conditions of the bounds, on the float64 reference, with no element excluded"""
    raw = fw["raw"][live]
    gap = ((raw.abs() - R.CLAMP).abs() - tol["raw"]).min()
    assert float(gap) > 0, f"{what}: a raw logit within its tolerance of the clamp boundary (choose another seed)"
    for name, n in (("target", fw["tnorm_true"][live]), ("source", s_norm[live])):
        assert bool(((n - R.EPS).abs() > tol["e_n"] * n + 1e-300).all()), f"{what}: a {name} row norm within its tolerance of eps"


# ------------------------------------------------------------------------------------------------ running a case
def sync(ctx):
    if ctx.device.type == "cuda":
        torch.cuda.synchronize()


def _view(ctx, B, H, W, Cv, halo, dtype, fill, interior=None):
    v = ctx.view(B, H, W, Cv, halo, dtype=dtype)
    v.t.fill_(fill)
    if interior is not None:
        v.nhwc()[..., :interior.shape[3]].copy_(interior.to(ctx.device))
    return v


def halo_mask(B, H, W, C, halo):
    m = torch.ones(B, H + 2 * halo, W + 2 * halo, C, dtype=torch.bool)
    m[:, halo:halo + H, halo:halo + W] = False
    return m


def run_case(ctx, r):
    shape, dtype = r.shape, r.dtype
    B, H, W, Cv, halo, P, C = shape
    check_regime(shape)
    ops = ctx.ops
    src, tgt, ids, T = make_data(r)
    g = torch.Generator().manual_seed(seed_of(r) + 1)
    prior = (torch.randn(B, H, W, C, generator=g) * 0.01).to(TDT[dtype])
    n_ws = ops.patchnce_ws_floats(B, P, C)
    assert n_ws == 3 * B * P * C + 3 * B * P + cdiv(B, 4) * 4 + 64

    def once():
        sv = _view(ctx, B, H, W, Cv, halo, dtype, IN_HALO, src)
        tv = _view(ctx, B, H, W, Cv, halo, dtype, IN_HALO, tgt)
        if r.cls == "nf_unsampled" and halo:
            sv.padded()[:, 0, :, :] = float("inf")
            tv.padded()[:, :, 0, :] = float("inf")
        gv = _view(ctx, B, H, W, Cv, halo, dtype, SENT, prior)
        iv = ctx.i32(ids.tolist())
        loss = ctx.f32(1, LOSS_PRIOR)
        ws = ctx.f32(n_ws + GUARD, WS_FILL)
        ops.patchnce_fwd(sv, tv, iv, P, C, T, WEIGHT, loss, ws)()
        ops.patchnce_bwd(tv, iv, P, C, T, WEIGHT, gv, ws)()
        sync(ctx)
        return dict(loss=loss.detach().cpu().clone(), ws=ws.detach().cpu().clone(), gtgt=gv.padded().detach().cpu().clone(),
                    src=sv.nhwc().detach().cpu().double(), tgt=tv.nhwc().detach().cpu().double())
    a, b = once(), once()
    what = run_id(r)
    assert torch.equal(a["loss"].view(torch.int32), b["loss"].view(torch.int32)), f"{what}: a repeated call gave another loss"
    assert torch.equal(a["gtgt"].view(BITS[dtype]), b["gtgt"].view(BITS[dtype])), f"{what}: a repeated call gave other bits in gtgt"
    if ops.is_hip:
        assert torch.equal(a["ws"].view(torch.int32), b["ws"].view(torch.int32)), f"{what}: a repeated call gave other bits in the workspace"
        assert bool((a["ws"][n_ws:] == WS_FILL).all()), f"{what}: floats past gan_patchnce_ws_floats were written"
    # what no reference has a say in: halos of gtgt and its channels >= C keep the sentinel
    hm = halo_mask(B, H, W, Cv, halo)
    assert bool((a["gtgt"][hm].float() == SENT).all()), f"{what}: the halo of gtgt was written"
    inner = a["gtgt"][:, halo:halo + H, halo:halo + W]
    assert bool((inner[..., C:].float() == SENT).all()), f"{what}: channels >= C of gtgt were written"
    res = dict(run=r, what=what, is_hip=ops.is_hip, T=t32(T), ids=ids, src64=a["src"], tgt64=a["tgt"], prior=prior, prior64=prior.double(),
               loss=float(a["loss"][0].double()), gtgt=inner[..., :C].clone(), n_ws=n_ws)
    if ops.is_hip:
        w, o = a["ws"], 0
        for name, n, shp in (("Sn", B * P * C, (B, P, C)), ("Tn", B * P * C, (B, P, C)), ("tnorm", B * P, (B, P)), ("lse", B * P, (B, P)),
                             ("rowloss", B * P, (B, P)), ("flag", cdiv(B, 4) * 4, None), ("dX", B * P * C, (B, P, C))):
            res["ws_" + name] = w[o:o + n].view(shp).double() if shp else w[o:o + B].double()
            o += n
        assert o + 64 == n_ws
    # the true reference, its tolerances and the conditions they rest on
    s, t = R.gather64(res["src64"], ids, C), R.gather64(res["tgt64"], ids, C)
    fw = R.forward64(s, t, res["T"])
    bw = R.backward64(fw, res["T"], WEIGHT)
    live = torch.nonzero(fw["flag"]).flatten()
    tol = tolerances(fw, bw, res["T"], WEIGHT, LOSS_PRIOR, live)
    check_conditions(fw, torch.sqrt((s * s).sum(2)), tol, live, what)
    res.update(fw=fw, bw=bw, live=live, tol=tol)
    return res


_results = {}


def result(make, r):
    ctx = make()
    key = (ctx.device.type, r)
    if key not in _results:
        _results[key] = run_case(ctx, r)
    return _results[key]


# ------------------------------------------------------------------------------------------------ assertions
_rejecting = []
_worst = {}


def ratio(got, ref, tol):
    """max |got - ref| / tol; a zero tolerance admits only an exact match"""
    r = (got.double() - ref).abs() / (tol + 1e-300)
    assert not bool(torch.isnan(r).any()), "NaN in a result or its reference"
    return float(r.max()) if r.numel() else 0.0


def report(what, q, r):
    if _rejecting:
        print(f"[nce-family] (against the wrong reference {_rejecting[0]}) {what} {q}: {r:.3g}")
    else:
        _worst[(what, q)] = r
        print(f"[nce-family] {what} {q}: error / bound = {r:.3g}")
    return r


def check_data_class(res):
    """the data class does what it names, on the float64 reference"""
    r, fw = res["run"], res["fw"]
    B, H, W, Cv, halo, P, C = r.shape
    raw = fw["raw"]
    if r.cls == "corr" or r.cls == "big":
        assert float(raw.abs().max()) < R.CLAMP and bool(fw["flag"].all())
    if r.cls == "clamp":
        hi, lo, mid = raw > R.CLAMP, raw < -R.CLAMP, raw.abs() < R.CLAMP
        assert bool(hi.any())
        if P >= 2:
            assert bool(lo.any())
            assert bool((hi.any(2) & mid.any(2)).any()) and bool((lo.any(2) & mid.any(2)).any()), "no row with clamped and unclamped entries"
    if r.cls == "eps":
        s = R.gather64(res["src64"], res["ids"], C)
        for n in (fw["tnorm_true"], torch.sqrt((s * s).sum(2))):
            assert bool((n == 0).any() or P < 6) and bool((n < R.EPS).any())
    if r.cls == "big":
        assert float(fw["tnorm_true"].max()) > 1e18
    if r.cls in ("nf_src_inf", "nf_tgt_nan"):
        dead = {"nf_src_inf": 1, "nf_tgt_nan": 2}[r.cls]
        assert fw["flag"].tolist() == [b != dead for b in range(B)]
    if r.cls == "nf_unsampled":
        assert bool(fw["flag"].all()) and not bool(torch.isfinite(res["src64"]).all())
    if r.ids == "dup":
        ids = res["ids"].tolist()
        assert P < 2 or (0 in ids and H * W - 1 in ids)
        assert all(ids[m] == ids[m - 1] for m in (64, 128, 192) if P > m)


def check(res, ref=None):
    """hold the results of a run to `ref` (the true statement by default) with the tolerances of the true one"""
    ref = ref or R.Ref()
    true = type(ref) is R.Ref
    r, what, T, ids, tol, live = res["run"], res["what"], res["T"], res["ids"], res["tol"], res["live"]
    B, H, W, Cv, halo, P, C = r.shape
    if true:
        fw, bw = res["fw"], res["bw"]
        check_data_class(res)
    else:
        fw = R.forward64(R.gather64(res["src64"], ids, C, ref), R.gather64(res["tgt64"], ids, C, ref), T, ref)
        bw = R.backward64(fw, T, WEIGHT, ref)
    flag = res["fw"]["flag"]
    dead = torch.nonzero(~flag).flatten()
    worst = {}
    # loss
    inc = float(R.loss64(fw, WEIGHT, ref))
    want = inc if ref.loss_overwrite else LOSS_PRIOR + inc
    worst["loss"] = ratio(torch.tensor(res["loss"]), torch.tensor(want, dtype=torch.float64), torch.tensor(float(tol["loss"])))
    # gtgt
    wantg, n, mag = R.scatter64(res["prior64"], bw[2], ids, C, fw["flag"], ref)
    _, n_true, mag_true = R.scatter64(res["prior64"], res["bw"][2], ids, C, flag)
    tsum = torch.zeros(B, H, W, C, dtype=torch.float64)
    tsum[live], _, _ = R.scatter64(torch.zeros(len(live), H, W, C, dtype=torch.float64), tol["dX"], ids, C, torch.ones(len(live), dtype=torch.bool))
    e = tsum + n_true.view(1, H, W, 1).double() * U * mag_true
    truth, _, _ = R.scatter64(res["prior64"], res["bw"][2], ids, C, flag)
    tolg = e + U_OUT[r.dtype] * (truth.abs() + e) + ETA
    worst["gtgt"] = ratio(res["gtgt"][live], wantg[live], tolg[live])
    if len(dead) and true:
        assert torch.equal(res["gtgt"][dead].view(BITS[r.dtype]), res["prior"][dead].view(BITS[r.dtype])), f"{what}: gtgt of a non-finite image lost its prior bits"
    if res["is_hip"]:
        for name in ("Sn", "Tn", "tnorm", "lse", "rowloss"):
            worst[name] = ratio(res["ws_" + name][live], fw[name][live][:, :, :C] if name in ("Sn", "Tn") else fw[name][live], tol[name])
        worst["dX"] = ratio(res["ws_dX"][live], bw[2][live, :, :C], tol["dX"])
        # THE SCATTER ITSELF: gtgt against the float64 sum of the rows the backward kernel left in the workspace (they are its summands bit for
        # bit), n rows and the prior added in order by one lane, one rounding to the buffer's dtype
        own, n_o, mag_o = R.scatter64(res["prior64"], res["ws_dX"], ids, C, flag, ref)
        e_o = n_o.view(1, H, W, 1).double() * U * mag_o
        worst["scatter"] = ratio(res["gtgt"], own, e_o + U_OUT[r.dtype] * (own.abs() + e_o) + ETA)
        if true:
            assert torch.equal(res["ws_flag"], flag.double()), f"{what}: flag {res['ws_flag'].tolist()} for {flag.tolist()}"
            assert bool((res["ws_dX"][dead] == 0).all()), f"{what}: dX rows of a non-finite image are not exactly zero"
    for q, v in worst.items():
        report(what, q, v)
    bad = {q: v for q, v in worst.items() if not v <= 1.0}
    assert not bad, f"{what}: outside the derived bound (error / bound): {bad}"


def body(make, r, ref=None):
    check(result(make, r), ref)


# ------------------------------------------------------------------------------------------------ wrong references
def _wrong(name, **kw):
    return type(name, (R.Ref,), kw)


def _find(shape, dtype, cls, ids="dup"):
    r = Run(shape, dtype, cls, ids)
    assert r in RUNS, r
    return r


# every wrong statement with the runs it is tried on (one MFMA, one scalar where both exist)
WRONG = [
    (_wrong("NoClampMask", no_mask=True), [_find(SHAPES[4][0], F32, "clamp"), _find(SHAPES[8][0], BF16, "clamp")]),
    (_wrong("Eps1e12", eps=1e-12), [_find(SHAPES[1][0], F32, "eps"), _find(SHAPES[7][0], BF16, "eps")]),
    (_wrong("DuplicatesOverwrite", dup_overwrite=True), [_find(SHAPES[4][0], BF16, "corr"), _find(SHAPES[9][0], F32, "corr")]),
    (_wrong("DivisionByPOnly", no_B=True), [_find(SHAPES[0][0], F32, "corr"), _find(SHAPES[13][0], BF16, "corr")]),
    (_wrong("NoTemperatureInGradient", no_invT_grad=True), [_find(SHAPES[1][0], BF16, "corr"), _find(SHAPES[8][0], F32, "corr")]),
    (_wrong("IdOverH", div_H=True), [_find(SHAPES[2][0], F32, "corr")]),
    (_wrong("NoProjection", no_projection=True), [_find(SHAPES[0][0], BF16, "corr"), _find(SHAPES[11][0], F32, "corr")]),
    (_wrong("NonFiniteCounted", count_nonfinite=True), [_find(NF_SHAPES[0][0], F32, "nf_src_inf"), _find(NF_SHAPES[1][0], BF16, "nf_tgt_nan")]),
    (_wrong("ViewChannels", view_channels=True), [_find(SHAPES[5][0], F32, "corr"), _find(NF_SHAPES[0][0], BF16, "nf_unsampled")]),
    (_wrong("LossOverwritten", loss_overwrite=True), [_find(SHAPES[0][0], F32, "corr"), _find(SHAPES[12][0], BF16, "corr")]),
]


def rejects(make, wrong, runs):
    """the kernels' results held to the wrong reference fail on every run listed for it"""
    failed = []
    _rejecting.append(wrong.__name__)
    try:
        for r in runs:
            res = result(make, r)
            try:
                check(res, wrong())
            except AssertionError as e:
                failed.append((run_id(r), str(e)[:100]))
    finally:
        _rejecting.clear()
    print(f"[nce-family] {wrong.__name__} rejected on {failed}")
    assert len(failed) == len(runs), f"the assertions accept the wrong reference {wrong.__name__} on a run it was tried on"


# ------------------------------------------------------------------------------------------------ refused arguments (the C ABI's checks)
def body_refused(make):
    """each returns its error and writes nothing: loss, workspace and gtgt keep their bits"""
    from gan_variant_research_amd._lib import GanError
    ctx = make()
    ops = ctx.ops
    B, H, W, Cv, halo = 2, 4, 4, 64, 1
    mk = lambda dtype=F32, H_=H, C_=Cv, fill=1.0: _view(ctx, B, H_, W, C_, halo, dtype, fill)
    src, tgt, gt = mk(), mk(), mk(fill=SENT)
    ids = ctx.i32([i % (H * W) for i in range(300)])
    loss, ws = ctx.f32(1, LOSS_PRIOR), ctx.f32(ops.patchnce_ws_floats(B, 256, 512) + GUARD, WS_FILL)
    narrow = _view(ctx, B, H, W, 32, halo, F32, SENT)
    wide_s, wide_t = _view(ctx, B, H, W, 520, halo, F32, 1.0), _view(ctx, B, H, W, 520, halo, F32, 1.0)
    calls = {
        "P=0": (lambda: ops.patchnce_fwd(src, tgt, ids, 0, 64, 0.07, 1.0, loss, ws), lambda: ops.patchnce_bwd(tgt, ids, 0, 64, 0.07, 1.0, gt, ws)),
        "P=257": (lambda: ops.patchnce_fwd(src, tgt, ids, 257, 64, 0.07, 1.0, loss, ws), lambda: ops.patchnce_bwd(tgt, ids, 257, 64, 0.07, 1.0, gt, ws)),
        "C=0": (lambda: ops.patchnce_fwd(src, tgt, ids, 16, 0, 0.07, 1.0, loss, ws), lambda: ops.patchnce_bwd(tgt, ids, 16, 0, 0.07, 1.0, gt, ws)),
        "C=520": (lambda: ops.patchnce_fwd(wide_s, wide_t, ids, 16, 520, 0.07, 1.0, loss, ws), lambda: ops.patchnce_bwd(wide_t, ids, 16, 520, 0.07, 1.0, wide_s, ws)),
        "C > view C": (lambda: ops.patchnce_fwd(src, tgt, ids, 16, 72, 0.07, 1.0, loss, ws), lambda: ops.patchnce_bwd(tgt, ids, 16, 72, 0.07, 1.0, gt, ws)),
        "C > gtgt channels": (None, lambda: ops.patchnce_bwd(tgt, ids, 16, 64, 0.07, 1.0, narrow, ws)),
        "shape mismatch": (lambda: ops.patchnce_fwd(mk(H_=5), tgt, ids, 16, 64, 0.07, 1.0, loss, ws), lambda: ops.patchnce_bwd(tgt, ids, 16, 64, 0.07, 1.0, mk(H_=5, fill=SENT), ws)),
        "dtype mismatch": (lambda: ops.patchnce_fwd(mk(BF16), tgt, ids, 16, 64, 0.07, 1.0, loss, ws), lambda: ops.patchnce_bwd(tgt, ids, 16, 64, 0.07, 1.0, mk(BF16, fill=SENT), ws)),
    }
    for name, pair in calls.items():
        for op in pair:
            if op is None:
                continue
            with pytest.raises(GanError, match="patchnce"):
                op()()
    sync(ctx)
    assert float(loss[0]) == LOSS_PRIOR and bool((ws == WS_FILL).all()), "a refused call wrote the loss or the workspace"
    assert bool((gt.t.float() == SENT).all()) and bool((narrow.t.float() == SENT).all()) and bool((wide_s.t == 1.0).all()), "a refused call wrote gtgt"
