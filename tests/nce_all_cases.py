"""TEST INFRASTRUCTURE: cases, derived bounds and assertions for PatchNCE with negatives from the whole minibatch (gan_patchnce_all_*,
csrc/patchnce.hip), written against an op layer: tests/test_nce_all_cpu.py runs them on tests/emulator_nce_all.py (loss and gtgt),
tests/test_nce_all_gpu.py on HipOps (the workspace intermediates as well), with the same shapes and the same assertions.  The float64
statement is tests/nce_all_ref64.py.

Bounds: those of tests/nce_cases.py (k(n) = BOUND_C sqrt(n) u, u = 2^-24, eta = 2^-126; read its docstring for the derivation of every
term) with the sums over the P source patches of an image taken over the K = S Q keys of the call, the positive at column self Q + i instead
of the diagonal, the divisor P B replaced by Q, and the image mean followed by the batch mean replaced by one mean over Q rows:

        tol(lse)  = E_i + sum_j p_j (4u + u |lg_j - mx|) + k(K) + 4u |lse - mx| + u |lse| + 5u (TRIPS + COMBINE)
        tol(call) = mean tol(rowloss) + k(Q) mean |rowloss| + u |call|;    tol(inc) = |weight| tol(call) + 3u |inc|
        tol(d)    = sc (tol(p) + u |p - [j = pos]|) + 5u |d| + 2 eta,   sc = |weight| / (Q T)
        tol(g)    = tol(d) . |Key| + (|d| . |Key|) (e_r + k(K)) + (K + 1) eta

THE RUNNING MAXIMUM.  The kernels never hold a row of logits: a lane keeps (m, s) = (maximum, sum of exp(. - m)) of the columns it has met
and rescales s by expf(m_old - m_new) on every key trip; the lanes' pairs are then merged the same way.  Term j therefore carries the
product exp(lg_j - m_1) exp(m_1 - m_2) ... exp(m_n - mx) instead of exp(lg_j - mx).  The maxima only grow, lg_j <= m_1 <= ... <= mx, so the
roundings of the subtractions add up to at most u (m_1 - lg_j) + u (m_2 - m_1) + ... = u |lg_j - mx|: the term the bound already has.  What
is new is one expf (4u) and one product (u) per rescale on the relative error of the sum, i.e. on the absolute error of lse:  5u per key
trip, TRIPS = ceil(K / KEY_TILE), and 5u per merge level, COMBINE = 8 (the scalar path merges 64 lanes in 6 levels and 4 waves in 2; the MFMA
path 16 lanes in 4 levels and 4 waves in 2).  The keys are not split over workgroups (SPLIT = 1): there is no further combine.
Foreign key segments are given normalised rows, exact as stored; they are bounded like the own rows (e_r), which only widens the bound by
the rounding of a row that has none.  None of the bounds is fitted to a result.

CONDITIONS (asserted by the case builder on the float64 reference, no element excluded; a case that violates one is a broken case): no raw
logit within tol(raw) of +-50; no row norm of source or target within e_n of eps.

A call whose float64 loss is not finite is held to: every flag entry 0, nothing added to the loss, every dX row exactly 0, gtgt bit for bit
its prior.  All-equal ids make all rows of an image identical; the `equal` runs also make the images identical (and the foreign segments
copies), so the softmax is uniform over the K keys: loss log K, every gradient row 0 in float64.
"""
import math
from collections import namedtuple

import pytest
import torch

from gan_variant_research_amd import BF16, F32
from tests import nce_all_ref64 as R
from tests import nce_cases as N0
from tests.nce_cases import (BITS, ETA, GUARD, IN_HALO, LOSS_PRIOR, NAME, SENT, TDT, U, U_OUT, WEIGHT, WS_FILL, cdiv, halo_mask, k, ratio, sync,
                             t32, _view)

# documented constants of the gan_patchnce_all_* kernels (include/mi355x_gan.h, csrc/patchnce.hip)
QUERY_TILE, KEY_TILE, K_CHUNK, SPLIT, MFMA_MAXC, MAXP, MAXC, COMBINE = 16, 256, 64, 1, 256, 256, 512, 8
KEY_SENT = 9.5e3          # between and behind the key segments of a run with foreign keys

# (B, H, W, view C, halo, P, C) and the regime the case names
SHAPES = [
    ((2, 4, 4, 64, 1, 16, 64), dict(path="mfma", Q=32, trips=1, key_tail=32, row_tiles=2)),
    ((3, 7, 7, 192, 1, 48, 192), dict(path="mfma", Q=144, trips=1, key_tail=144, k_chunks=3)),
    ((5, 5, 13, 128, 0, 80, 128), dict(path="mfma", Q=400, trips=2, key_tail=144, nonsquare=True)),
    ((4, 16, 16, 256, 1, 256, 256), dict(path="mfma", Q=1024, trips=4, key_tail=0, k_chunks=4)),
    ((2, 16, 16, 64, 1, 240, 64), dict(path="mfma", Q=480, trips=2, key_tail=224)),
    ((2, 6, 6, 128, 1, 32, 64), dict(path="mfma", Q=64, view_wider=True)),
    ((1, 3, 3, 8, 1, 1, 8), dict(path="scalar", Q=1, row_tiles=1, last_tile_rows=1)),
    ((2, 3, 3, 8, 1, 1, 8), dict(path="scalar", Q=2, last_tile_rows=2)),
    ((3, 5, 5, 64, 1, 17, 64), dict(path="scalar", Q=51, mfma_c=True, last_tile_rows=3)),
    ((2, 10, 10, 40, 0, 100, 40), dict(path="scalar", Q=200, mfma_q=False, mfma_c=False)),
    ((1, 16, 16, 512, 1, 256, 512), dict(path="scalar", Q=256, mfma_q=True, c_mult64=True, trips=1, key_tail=0)),
    ((257, 2, 2, 8, 0, 4, 8), dict(path="scalar", Q=1028, trips=5, key_tail=4, last_tile_rows=4)),
    ((2, 8, 8, 320, 1, 64, 320), dict(path="scalar", Q=128, mfma_q=True, c_mult64=True)),                  # C % 64 == 0 above the MFMA range
    ((1, 16, 16, 256, 1, 256, 256), dict(path="mfma", Q=256, trips=1, key_tail=0)),                        # B = 1: exactly one full key trip
    ((3, 6, 6, 128, 1, 32, 64), dict(path="mfma", Q=96)),                                                  # the non-finite classes (B = 3)
    ((5, 4, 4, 16, 1, 8, 16), dict(path="scalar", Q=40)),
]
REGIME = dict(SHAPES)


def regime(shape, segs=1):
    B, H, W, Cv, halo, P, C = shape
    Q = B * P
    K = Q * segs
    mfma = C % K_CHUNK == 0 and C <= MFMA_MAXC and Q % QUERY_TILE == 0
    return dict(path="mfma" if mfma else "scalar", Q=Q, K=K, trips=cdiv(K, KEY_TILE), key_tail=K % KEY_TILE, row_tiles=cdiv(Q, QUERY_TILE),
                last_tile_rows=Q - QUERY_TILE * (cdiv(Q, QUERY_TILE) - 1), k_chunks=C // K_CHUNK, view_wider=Cv > C, nonsquare=H != W,
                mfma_c=C % K_CHUNK == 0 and C <= MFMA_MAXC, mfma_q=Q % QUERY_TILE == 0, c_mult64=C % K_CHUNK == 0, split=SPLIT)


def check_regime(shape):
    """the case is in the regime it names, from the documented constants and the entry checks"""
    B, H, W, Cv, halo, P, C = shape
    assert 1 <= P <= MAXP and 1 <= C <= MAXC and C <= Cv
    g = regime(shape)
    for key, want in REGIME[shape].items():
        assert g[key] == want, f"{shape}: {key} = {g[key]}, the case names {want}"
    return g


# cls: corr | clamp | eps | big | nf_src_inf | nf_tgt_nan | nf_unsampled | nf_foreign          ids: dup | perm | equal
Run = namedtuple("Run", "shape dtype cls ids segs self_seg", defaults=(1, 0))
NF = (SHAPES[14][0], SHAPES[15][0])


def _runs():
    out = []
    for shape, _ in SHAPES[:14]:
        for dt in (BF16, F32):
            out.append(Run(shape, dt, "corr", "dup"))
    for i in (0, 1, 2, 5, 8, 9, 12):
        for dt in (BF16, F32):
            out += [Run(SHAPES[i][0], dt, "clamp", "dup"), Run(SHAPES[i][0], dt, "eps", "dup")]
    for i in (3, 4, 10):
        out += [Run(SHAPES[i][0], F32, "eps", "dup"), Run(SHAPES[i][0], BF16, "corr", "perm")]
    for i in (0, 2, 4, 9):
        out += [Run(SHAPES[i][0], BF16, "corr", "equal"), Run(SHAPES[i][0], F32, "corr", "equal")]
    for shape in NF:
        for dt in (BF16, F32):
            out += [Run(shape, dt, cls, "dup") for cls in ("nf_src_inf", "nf_tgt_nan", "nf_unsampled")]
    for dt in (BF16, F32):
        out += [Run(SHAPES[0][0], dt, "big", "dup"), Run(SHAPES[15][0], dt, "big", "dup")]
        # foreign key segments
        out += [Run(SHAPES[0][0], dt, "corr", "dup", 3, 1), Run(SHAPES[3][0], dt, "corr", "dup", 2, 1), Run(SHAPES[3][0], dt, "corr", "dup", 2, 0),
                Run(SHAPES[8][0], dt, "corr", "dup", 3, 2), Run(SHAPES[0][0], dt, "nf_foreign", "dup", 3, 1), Run(SHAPES[0][0], dt, "clamp", "dup", 3, 1)]
    out += [Run(SHAPES[0][0], F32, "corr", "equal", 3, 1), Run(SHAPES[6][0], F32, "corr", "dup", 3, 2)]
    return out


RUNS = _runs()


def run_id(r):
    return "x".join(map(str, r.shape)) + f"-{NAME[r.dtype]}-{r.cls}-{r.ids}" + (f"-S{r.segs}self{r.self_seg}" if r.segs > 1 else "")


def base_run(r):
    """the run of tests/nce_cases.py whose data builder makes this run's source and target"""
    return N0.Run(r.shape, r.dtype, "corr" if r.cls == "nf_foreign" else r.cls, r.ids)


def make_data(r):
    """(src, tgt) interiors in the buffer's dtype, ids, temperature, and the S - 1 foreign key segments (Q, C) fp32, normalised"""
    B, H, W, Cv, halo, P, C = r.shape
    src, tgt, ids, T = N0.make_data(base_run(r))
    if r.ids == "equal":                  # identical images as well: the softmax is uniform over all K keys
        src[:], tgt[:] = src[0:1].clone(), tgt[0:1].clone()
    g = torch.Generator().manual_seed(N0.seed_of(base_run(r)) + 77 + r.segs * 5 + r.self_seg)
    foreign = []
    for s in range(r.segs - 1):
        if r.ids == "equal":
            x = src.double()[:, ids // W, ids % W, :C].reshape(B * P, C)
        else:
            # correlated with the targets (the other ranks' photos are other photos, but hard negatives are what the term is for)
            x = 0.6 * tgt.double()[:, ids // W, ids % W, :C].reshape(B * P, C).roll(s + 1, 0) + torch.randn(B * P, C, generator=g, dtype=torch.float64)
        x = torch.where(torch.isfinite(x), x, torch.ones_like(x))
        n = torch.sqrt((x * x).sum(1, keepdim=True))
        foreign.append((x / torch.where(n > 0, n, torch.ones_like(n))).float())
    if r.cls == "nf_foreign":
        foreign[-1][B * P // 2, C // 3] = float("nan")
    return src, tgt, ids, T, foreign


# ------------------------------------------------------------------------------------------------ tolerances from the float64 reference
def tolerances(fw, bw, T, weight, prior_loss, trips):
    """every tolerance of the module docstring, for a call of a true reference whose flag is 1"""
    Tn, Key, raw, lg, lse, mx, pos = (fw[n] for n in ("Tn", "keys", "raw", "lg", "lse", "mx", "pos"))
    tnorm, rowloss, call = fw["tnorm"], fw["rowloss"], fw["call"]
    Q, Kn = raw.shape
    C = Tn.shape[1]
    rows = torch.arange(Q)
    e_n = (k(C) + U) / 2 + 2 * U
    e_r = e_n + 2 * U
    t = dict(e_n=e_n, e_r=e_r, Sn=e_r * fw["Sn"].abs() + ETA, Tn=e_r * Tn.abs() + ETA, tnorm=e_n * tnorm)
    A = Tn.abs() @ Key.abs().t()
    t["raw"] = A * (k(C) + 2 * e_r + e_r * e_r) / T + 3 * U * raw.abs()
    clamped = raw.abs() > R.CLAMP
    t["lg"] = torch.where(clamped, torch.zeros_like(raw), t["raw"])
    E = t["lg"].max(1).values
    p = torch.exp(lg - lse.unsqueeze(1))
    t["lse"] = E + (p * (4 * U + U * (lg - mx.unsqueeze(1)).abs())).sum(1) + k(Kn) + 4 * U * (lse - mx).abs() + U * lse.abs() + 5 * U * (trips + COMBINE)
    t["rowloss"] = t["lse"] + t["lg"][rows, pos] + U * rowloss.abs()
    t["call"] = t["rowloss"].mean() + k(Q) * rowloss.abs().mean() + U * call.abs()
    inc = weight * call
    t["inc"] = abs(weight) * t["call"] + 3 * U * abs(inc)
    t["loss"] = t["inc"] + U * abs(prior_loss + inc)
    dlg, dTn, dX = bw
    d = dlg / T
    sc = abs(weight) / (Q * T)
    onehot = torch.zeros_like(raw)
    onehot[rows, pos] = 1.0
    tp = p * (t["lg"] + t["lse"].unsqueeze(1) + U * (lg - lse.unsqueeze(1)).abs() + 4 * U)
    td = sc * (tp + U * (p - onehot).abs()) + 5 * U * d.abs() + 2 * ETA
    td = torch.where(clamped, torch.zeros_like(td), td)
    tg = td @ Key.abs() + (d.abs() @ Key.abs()) * (e_r + k(Kn)) + (Kn + 1) * ETA
    dot = (Tn * dTn).sum(1, keepdim=True)
    tdot = (Tn.abs() * tg + e_r * (Tn * dTn).abs()).sum(1, keepdim=True) + k(C) * (Tn * dTn).abs().sum(1, keepdim=True) + (C + 1) * ETA
    nrm = tnorm.unsqueeze(1)
    normal = (tg + Tn.abs() * tdot + (e_r + 2 * U) * (Tn * dot).abs() + U * (dTn.abs() + (Tn * dot).abs()) + 3 * ETA) / nrm + (e_n + 2 * U) * dX.abs()
    t["dX"] = torch.where(nrm > R.EPS, normal, (tg + 3 * ETA) / nrm + 2 * U * dX.abs()) + ETA
    return t


def check_conditions(fw, s_norm, tol, what):
    gap = ((fw["raw"].abs() - R.CLAMP).abs() - tol["raw"]).min()
    assert float(gap) > 0, f"{what}: a raw logit within its tolerance of the clamp boundary (choose another seed)"
    for name, n in (("target", fw["tnorm_true"]), ("source", s_norm)):
        assert bool(((n - R.EPS).abs() > tol["e_n"] * n + 1e-300).all()), f"{what}: a {name} row norm within its tolerance of eps"


# ------------------------------------------------------------------------------------------------ running a case
def key_buffer(ctx, r, foreign, ws):
    """(keys tensor, seg_stride): single segment -> the workspace's own Sn; else a buffer of S segments seg_stride > Q C apart with sentinels
    between and behind them, the own segment filled from the workspace after the gather"""
    B, H, W, Cv, halo, P, C = r.shape
    if r.segs == 1:
        return ws, 0
    stride = B * P * C + 24
    buf = ctx.f32(r.segs * stride, KEY_SENT)
    others = list(foreign)
    for s in range(r.segs):
        if s != r.self_seg:
            buf[s * stride:s * stride + B * P * C].copy_(others.pop(0).reshape(-1).to(ctx.device))
    return buf, stride


def run_case(ctx, r):
    shape, dtype = r.shape, r.dtype
    B, H, W, Cv, halo, P, C = shape
    Q = B * P
    check_regime(shape)
    ops = ctx.ops
    src, tgt, ids, T, foreign = make_data(r)
    g = torch.Generator().manual_seed(N0.seed_of(base_run(r)) + 1)
    prior = (torch.randn(B, H, W, C, generator=g) * 0.01).to(TDT[dtype])
    n_ws = ops.patchnce_all_ws_floats(B, P, C)
    assert n_ws == 3 * Q * C + 3 * Q + cdiv(B, 4) * 4 + 64 == ops.patchnce_ws_floats(B, P, C)

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
        keys, stride = key_buffer(ctx, r, foreign, ws)
        ops.patchnce_all_gather(sv, tv, iv, P, C, ws)()
        if r.segs > 1:                     # what the trainer's exchange does with the own rows
            sync(ctx)
            keys[r.self_seg * stride:r.self_seg * stride + Q * C].copy_(ws[:Q * C])
        ops.patchnce_all_fwd(tv, P, C, T, WEIGHT, keys, r.segs, stride, r.self_seg, loss, ws)()
        ops.patchnce_all_bwd(tv, iv, P, C, T, WEIGHT, keys, r.segs, stride, r.self_seg, gv, ws)()
        sync(ctx)
        out = dict(loss=loss.detach().cpu().clone(), ws=ws.detach().cpu().clone(), gtgt=gv.padded().detach().cpu().clone(),
                   src=sv.nhwc().detach().cpu().double(), tgt=tv.nhwc().detach().cpu().double())
        if r.segs > 1:
            kb = keys.detach().cpu().view(r.segs, stride)
            assert bool((kb[:, Q * C:] == KEY_SENT).all()), "the sentinels between the key segments were written"
            for s, f in zip([s for s in range(r.segs) if s != r.self_seg], foreign):
                assert torch.equal(kb[s, :Q * C].view(torch.int32), f.reshape(-1).view(torch.int32)), "a foreign key segment was written"
        return out
    a, b = once(), once()
    what = run_id(r)
    assert torch.equal(a["loss"].view(torch.int32), b["loss"].view(torch.int32)), f"{what}: a repeated call gave another loss"
    assert torch.equal(a["gtgt"].view(BITS[dtype]), b["gtgt"].view(BITS[dtype])), f"{what}: a repeated call gave other bits in gtgt"
    if ops.is_hip:
        assert torch.equal(a["ws"].view(torch.int32), b["ws"].view(torch.int32)), f"{what}: a repeated call gave other bits in the workspace"
    assert bool((a["ws"][n_ws:] == WS_FILL).all()), f"{what}: floats past gan_patchnce_all_ws_floats were written"
    hm = halo_mask(B, H, W, Cv, halo)
    assert bool((a["gtgt"][hm].float() == SENT).all()), f"{what}: the halo of gtgt was written"
    inner = a["gtgt"][:, halo:halo + H, halo:halo + W]
    assert bool((inner[..., C:].float() == SENT).all()), f"{what}: channels >= C of gtgt were written"
    res = dict(run=r, what=what, is_hip=ops.is_hip, T=t32(T), ids=ids, src64=a["src"], tgt64=a["tgt"], prior=prior, prior64=prior.double(),
               loss=float(a["loss"][0].double()), loss_bits=a["loss"].view(torch.int32).clone(), gtgt=inner[..., :C].clone(), n_ws=n_ws,
               foreign64=[f.double() for f in foreign])
    if ops.is_hip:
        w, o = a["ws"], 0
        for name, n, shp in (("Sn", Q * C, (Q, C)), ("Tn", Q * C, (Q, C)), ("tnorm", Q, (Q,)), ("lse", Q, (Q,)), ("rowloss", Q, (Q,)),
                             ("flag", cdiv(B, 4) * 4, None), ("dX", Q * C, (Q, C))):
            res["ws_" + name] = w[o:o + n].view(shp).double() if shp else w[o:o + B].double()
            o += n
        assert o + 64 == n_ws
    s, t = R.gather64(res["src64"], ids, C), R.gather64(res["tgt64"], ids, C)
    fw = R.forward64(s, t, res["T"], res["foreign64"], r.self_seg)
    bw = R.backward64(fw, res["T"], WEIGHT)
    res.update(fw=fw, bw=bw, tol=None)
    if fw["flag"]:
        tol = tolerances(fw, bw, res["T"], WEIGHT, LOSS_PRIOR, regime(shape, r.segs)["trips"])
        check_conditions(fw, torch.sqrt((s * s).sum(2)).reshape(-1), tol, what)
        res["tol"] = tol
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


def report(what, q, v):
    tag = f"(against the wrong reference {_rejecting[0]}) " if _rejecting else ""
    print(f"[nce-all] {tag}{what} {q}: error / bound = {v:.3g}")


def check_data_class(res):
    """the data class does what it names, on the float64 reference"""
    r, fw = res["run"], res["fw"]
    B, H, W, Cv, halo, P, C = r.shape
    raw = fw["raw"]
    if r.cls in ("corr", "big"):
        assert float(raw.abs().max()) < R.CLAMP and fw["flag"]
    if r.cls == "clamp":
        hi, lo, mid = raw > R.CLAMP, raw < -R.CLAMP, raw.abs() < R.CLAMP
        assert bool(hi.any()) and fw["flag"]
        if P >= 2:
            assert bool(lo.any())
            assert bool((hi.any(1) & mid.any(1)).any()) and bool((lo.any(1) & mid.any(1)).any()), "no row with clamped and unclamped entries"
    if r.cls == "eps":
        s = R.gather64(res["src64"], res["ids"], C)
        for n in (fw["tnorm_true"], torch.sqrt((s * s).sum(2))):
            assert bool((n == 0).any() or P < 6) and bool((n < R.EPS).any())
    if r.cls == "big":
        assert float(fw["tnorm_true"].max()) > 1e18
    if r.cls in ("nf_src_inf", "nf_tgt_nan", "nf_foreign"):
        assert not fw["flag"]
        if r.cls == "nf_tgt_nan":       # the per-image statement would have silenced one image only
            assert int(torch.isfinite(fw["per"]).sum()) == B - 1
    if r.cls == "nf_unsampled":
        assert fw["flag"] and not bool(torch.isfinite(res["src64"]).all())
    if r.ids == "equal":
        K = fw["raw"].shape[1]
        if r.segs == 1:
            assert abs(float(fw["call"]) - math.log(K)) < 1e-9 and float(res["bw"][2].abs().max()) < 1e-15
        else:                              # the foreign copies are fp32 roundings of the own rows: uniform to fp32 accuracy
            assert abs(float(fw["call"]) - math.log(K)) < 1e-5
    if r.segs > 1 and fw["flag"]:
        own = torch.zeros(raw.shape[1], dtype=torch.bool)
        own[r.self_seg * B * P:(r.self_seg + 1) * B * P] = True
        p = torch.exp(fw["lg"] - fw["lse"].unsqueeze(1))
        assert r.ids == "equal" or float(p[:, ~own].sum(1).max()) > 1e-3, "the foreign keys carry no weight: the case shows nothing"


def check(res, ref=None):
    """hold the results of a run to `ref` (the true statement by default) with the tolerances of the true one"""
    ref = ref or R.Ref()
    true = type(ref) is R.Ref
    r, what, T, ids, tol = res["run"], res["what"], res["T"], res["ids"], res["tol"]
    B, H, W, Cv, halo, P, C = r.shape
    Q = B * P
    if true:
        fw, bw = res["fw"], res["bw"]
        check_data_class(res)
    else:
        fw = R.forward64(R.gather64(res["src64"], ids, C), R.gather64(res["tgt64"], ids, C), T, res["foreign64"], r.self_seg, ref)
        bw = R.backward64(fw, T, WEIGHT, ref)
    live = res["fw"]["flag"]
    inc = float(R.loss64(fw, WEIGHT, ref))
    want = inc if ref.loss_overwrite else LOSS_PRIOR + inc
    worst = {}
    if not live:
        # the flag-0 call: exact statements, no tolerance
        worst["loss"] = 0.0 if res["loss"] == want else float("inf")
        wantg, _, _ = R.scatter64(res["prior64"], bw[2].view(B, P, -1), ids, C, fw["flag_b"])
        worst["gtgt"] = 0.0 if torch.equal(res["gtgt"].double(), wantg) else float("inf")
        if true:
            assert torch.equal(res["gtgt"].view(BITS[r.dtype]), res["prior"].view(BITS[r.dtype])), f"{what}: gtgt of a flag-0 call lost its prior bits"
            if res["is_hip"]:
                assert bool((res["ws_flag"] == 0).all()) and bool((res["ws_dX"] == 0).all()), f"{what}: flag or dX of a flag-0 call"
    else:
        worst["loss"] = ratio(torch.tensor(res["loss"]), torch.tensor(want, dtype=torch.float64), torch.tensor(float(tol["loss"])))
        ones = torch.ones(B, dtype=torch.bool)
        wantg, n, mag = R.scatter64(res["prior64"], bw[2].view(B, P, -1), ids, C, fw["flag_b"])
        truth, n_true, mag_true = R.scatter64(res["prior64"], res["bw"][2].view(B, P, C), ids, C, ones)
        tsum, _, _ = R.scatter64(torch.zeros(B, H, W, C, dtype=torch.float64), tol["dX"].view(B, P, C), ids, C, ones)
        e = tsum + n_true.view(1, H, W, 1).double() * U * mag_true
        tolg = e + U_OUT[r.dtype] * (truth.abs() + e) + ETA
        worst["gtgt"] = ratio(res["gtgt"], wantg, tolg)
        if res["is_hip"]:
            for name in ("Sn", "Tn", "tnorm", "lse", "rowloss"):
                worst[name] = ratio(res["ws_" + name], fw[name], tol[name])
            worst["dX"] = ratio(res["ws_dX"], bw[2], tol["dX"])
            own, n_o, mag_o = R.scatter64(res["prior64"], res["ws_dX"].view(B, P, C), ids, C, ones)
            e_o = n_o.view(1, H, W, 1).double() * U * mag_o
            worst["scatter"] = ratio(res["gtgt"], own, e_o + U_OUT[r.dtype] * (own.abs() + e_o) + ETA)
            if true:
                assert bool((res["ws_flag"] == 1).all()), f"{what}: flag {res['ws_flag'].tolist()}"
        if true and Q == 1 and r.segs == 1:
            assert res["loss"] == LOSS_PRIOR and bool((res["gtgt"].view(BITS[r.dtype]) == res["prior"].view(BITS[r.dtype])).all()), \
                f"{what}: Q = 1 adds exactly weight * 0 and a gradient of exactly 0"
    for q, v in worst.items():
        report(what, q, v)
    bad = {q: v for q, v in worst.items() if not v <= 1.0}
    assert not bad, f"{what}: outside the derived bound (error / bound): {bad}"


def body(make, r, ref=None):
    check(result(make, r), ref)


# ------------------------------------------------------------------------------------------------ wrong references
def _wrong(name, **kw):
    return type(name, (R.Ref,), kw)


def _find(i, dtype, cls, ids="dup", segs=1, self_seg=0):
    r = Run(SHAPES[i][0], dtype, cls, ids, segs, self_seg)
    assert r in RUNS, r
    return r


WRONG = [
    (_wrong("PositiveAtColumnI", pos_at_i=True), [_find(0, F32, "corr", segs=3, self_seg=1), _find(8, BF16, "corr", segs=3, self_seg=2)]),
    (_wrong("DivisionByP", div_P=True), [_find(0, F32, "corr"), _find(9, BF16, "corr")]),
    (_wrong("MeanPerImage", per_image=True), [_find(14, F32, "nf_tgt_nan"), _find(15, BF16, "nf_tgt_nan")]),
    (_wrong("OwnSegmentOnly", own_segment=True), [_find(3, F32, "corr", segs=2, self_seg=0), _find(8, BF16, "corr", segs=3, self_seg=2)]),
    (_wrong("NoClampMask", no_mask=True), [_find(2, F32, "clamp"), _find(9, BF16, "clamp")]),
    (_wrong("NoTemperatureInGradient", no_invT_grad=True), [_find(2, BF16, "corr"), _find(11, F32, "corr")]),
    (_wrong("LossOverwritten", loss_overwrite=True), [_find(0, F32, "corr"), _find(12, BF16, "corr")]),
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
    print(f"[nce-all] {wrong.__name__} rejected on {failed}")
    assert len(failed) == len(runs), f"the assertions accept the wrong reference {wrong.__name__} on a run it was tried on"


# ------------------------------------------------------------------------------------------------ equivalence with the per-image entry points
EQUIV = [Run(SHAPES[i][0], dt, "corr", "dup") for i in (10, 13) for dt in (BF16, F32)]


def body_equivalence(make, r):
    """B = 1, S = 1: loss and gtgt lie within the sum of both paths' bounds of gan_patchnce_fwd / bwd on the same data"""
    assert r.shape[0] == 1 and r.segs == 1 and r in RUNS
    new = result(make, r)
    old = N0.result(make, base_run(r)) if base_run(r) in N0.RUNS else N0.run_case(make(), base_run(r))
    B, H, W, Cv, halo, P, C = r.shape
    tl = float(new["tol"]["loss"]) + float(old["tol"]["loss"])
    assert abs(new["loss"] - old["loss"]) <= tl, (new["loss"], old["loss"], tl)
    ones = torch.ones(1, dtype=torch.bool)
    tn, _, _ = R.scatter64(torch.zeros(1, H, W, C, dtype=torch.float64), new["tol"]["dX"].view(1, P, C), new["ids"], C, ones)
    to, _, _ = R.scatter64(torch.zeros(1, H, W, C, dtype=torch.float64), old["tol"]["dX"], old["ids"], C, ones)
    truth, n, mag = R.scatter64(new["prior64"], new["bw"][2].view(1, P, C), new["ids"], C, ones)
    e = tn + to + 2 * n.view(1, H, W, 1).double() * U * mag
    allow = e + 2 * U_OUT[r.dtype] * (truth.abs() + e) + 2 * ETA
    q = ratio(new["gtgt"], old["gtgt"].double(), allow)
    print(f"[nce-all] {new['what']} against gan_patchnce_fwd/bwd: loss difference {abs(new['loss'] - old['loss']):.3g} (allowed {tl:.3g}), gtgt {q:.3g}")
    assert q <= 1.0


# ------------------------------------------------------------------------------------------------ refused arguments (the C ABI's checks)
def body_refused(make):
    """each returns its error and writes nothing: loss, workspace, keys and gtgt keep their bits"""
    from gan_variant_research_amd._lib import GanError
    ctx = make()
    ops = ctx.ops
    B, H, W, Cv, halo = 2, 4, 4, 64, 1
    mk = lambda dtype=F32, H_=H, C_=Cv, fill=1.0: _view(ctx, B, H_, W, C_, halo, dtype, fill)
    src, tgt, gt = mk(), mk(), mk(fill=SENT)
    ids = ctx.i32([i % (H * W) for i in range(300)])
    loss, ws = ctx.f32(1, LOSS_PRIOR), ctx.f32(ops.patchnce_all_ws_floats(B, 256, 512) + GUARD, WS_FILL)
    keys = ctx.f32(3 * B * 256 * 520, KEY_SENT)
    narrow = _view(ctx, B, H, W, 32, halo, F32, SENT)
    wide_s, wide_t = _view(ctx, B, H, W, 520, halo, F32, 1.0), _view(ctx, B, H, W, 520, halo, F32, 1.0)
    G = lambda s, t, P, C: (lambda: ops.patchnce_all_gather(s, t, ids, P, C, ws))
    Fw = lambda t, P, C, segs=1, stride=0, self_seg=0, kk=keys: (lambda: ops.patchnce_all_fwd(t, P, C, 0.07, 1.0, kk, segs, stride, self_seg, loss, ws))
    Bw = lambda t, P, C, g, segs=1, stride=0, self_seg=0, kk=keys: (lambda: ops.patchnce_all_bwd(t, ids, P, C, 0.07, 1.0, kk, segs, stride, self_seg, g, ws))
    calls = {
        "P=0": (G(src, tgt, 0, 64), Fw(tgt, 0, 64), Bw(tgt, 0, 64, gt)),
        "P=257": (G(src, tgt, 257, 64), Fw(tgt, 257, 64), Bw(tgt, 257, 64, gt)),
        "C=0": (G(src, tgt, 16, 0), Fw(tgt, 16, 0), Bw(tgt, 16, 0, gt)),
        "C=520": (G(wide_s, wide_t, 16, 520), Fw(wide_t, 16, 520), Bw(wide_t, 16, 520, wide_s)),
        "C > view C": (G(src, tgt, 16, 72), Fw(tgt, 16, 72), Bw(tgt, 16, 72, gt)),
        "C > gtgt channels": (Bw(tgt, 16, 64, narrow),),
        "shape mismatch": (G(mk(H_=5), tgt, 16, 64), Bw(tgt, 16, 64, mk(H_=5, fill=SENT))),
        "dtype mismatch": (G(mk(BF16), tgt, 16, 64), Bw(tgt, 16, 64, mk(BF16, fill=SENT))),
        "segs=0": (Fw(tgt, 16, 64, 0), Bw(tgt, 16, 64, gt, 0)),
        "self=segs": (Fw(tgt, 16, 64, 2, 4096, 2), Bw(tgt, 16, 64, gt, 2, 4096, 2)),
        "self<0": (Fw(tgt, 16, 64, 2, 4096, -1), Bw(tgt, 16, 64, gt, 2, 4096, -1)),
        "stride < Q C": (Fw(tgt, 16, 64, 2, B * 16 * 64 - 1, 0), Bw(tgt, 16, 64, gt, 2, B * 16 * 64 - 1, 0)),
    }
    for name, ops_ in calls.items():
        for op in ops_:
            with pytest.raises(GanError, match="patchnce"):
                op()()
    sync(ctx)
    assert float(loss[0]) == LOSS_PRIOR and bool((ws == WS_FILL).all()) and bool((keys == KEY_SENT).all()), "a refused call wrote the loss, the workspace or the keys"
    assert bool((gt.t.float() == SENT).all()) and bool((narrow.t.float() == SENT).all()) and bool((wide_s.t == 1.0).all()), "a refused call wrote gtgt"
