"""TEST INFRASTRUCTURE: cases, derived bounds and assertions for the spectral-norm kernels (csrc/spectral.hip: the single-matrix path
gan_spectral_norm_fwd / _bwd and the batched path gan_spectral_norm_batch_fwd / _bwd), written against an op layer:
tests/test_spectral_family_cpu.py runs them on the emulator, tests/test_spectral_family_gpu.py on HipOps, with the same shapes and the same
assertions.  The float64 statements are in tests/spectral_ref64.py.

Bounds (convention of tests/cases.py: BOUND_C, U_F32 = 2^-24 =: u, sqrt(K); tests/pointwise_cases.py: ks(K, D)); none is fitted to a result.
Every output is held to the statement evaluated AT WHAT THE KERNEL WROTE for the quantities before it, so conditioning does not leak from
one quantity into the next:  v against normalize(W^T u_in);  u against normalize(W v_written);  sigma against u_written . (W v_written);
dW against the formula at the written sigma and snapshots with the float64 <G, W>.

  DOT of K products in fp32: (u + ks(K, D)) sum|terms| -- each product rounds, and the sum errs by min(BOUND_C sqrt(K), 1.01 D) u
  sum|terms| for the D levels of the kernel's documented order.
  ORDERS (csrc/spectral.hip).  Batched: t_j over the <= 32 rows of a tile, then the row tiles in order; s_i over 4 products per lane, the
  wave butterfly (6), the column tiles in order; ||t||^2 per tile by the butterfly and 4 waves, then the tiles by a 1024-thread block
  (trips, 6, 16); ||s||^2 and sigma by that block; <G, W> per tile over its rows, 6, 4, then the tile partials (trips of 256, 6, 4).
  Single matrix: t_j over the h rows in order; s_i by a 256-thread block (trips, 6, 4); the norms and sigma by a 1024-thread block;
  <G, W_sn> by <= 256 blocks striding the matrix (trips, 6, 4), then one partial per thread, 6, 4.
  NORMALISE x (length K, elementwise error e_x) to x / max(||x||, eps):  the norm errs by ||e_x||_2 (triangle inequality) plus, relative,
  (2u + ks(K, D)) / 2 for the squares and their sum under the square root, 2u for sqrtf, and eta per square below 2^-125; the quotient
  by e_x / d + |x / d| e_d / d + u |x / d| (x 1.01 for the second order).  In the eps branch (||x|| < eps) the divisor is eps, exact.
  t = W^T u: DOT over h.  s = W v: DOT over w, one more u per term (the batched path multiplies W by t and divides the row sum by ||t||,
  the single-matrix path multiplies by the rounded v), one more u for that division.
  SIGMA = sum u_i s_i with the kernel's own fp32 s:  sum |u_i| e_s_i + DOT over h.
  dW: k = <G, W> / sigma: (DOT over h w) / |sigma| + u |k|; k u_i v_j: two products; the difference; the division; with accumulate one
  more rounding of prior + value.  W_sn = W / sigma: one rounding.
  Snapshots, untouched u and v (power_iter = 0), sentinels and repeated calls are compared bit for bit.
  RANGE.  The squares of t = W^T u and s = W v stay normal and their sums finite for 2^-63 <= |t_j| and ||t|| < 2^64 (the same for s);
  smaller elements only add eta each.  With the reference's eps = 1e-12 a W scaled by 1e-15 is in the eps branch: v = t / eps.
  NON-FINITE.  A NaN in W, u or G of one descriptor reaches that descriptor's outputs and no other descriptor's.
"""
import math
from collections import namedtuple

import pytest
import torch

from tests import spectral_ref64 as R
from tests.cases import U_F32
from tests.optim_cases import Family
from tests.pointwise_cases import cpu, ks, ratio, same_bits, sync

U = U_F32
ETA = 2.0 ** -126
SENT, WS_FILL, GUARD = 7.5, 3e5, 64
NAN = float("nan")
EPS = 1e-12
SN_RB, SN_CB = R.SN_RB, R.SN_CB

PAIRS = [(1, 1), (1, 255), (31, 256), (32, 257), (33, 300), (64, 1), (64, 255), (31, 300), (32, 1), (33, 256), (64, 257)]      # h x w thinned
ONE_TILE = [(1, 1), (32, 256), (1, 1), (5, 7), (32, 256)]
TABLES = {
    "t1": [(33, 300)],
    "t2": [(1030, 40), (1, 1)],
    "t3": [(1, 1), (512, 4352), (32, 1)],                      # the largest in the middle, between one-tile descriptors
    "t16": PAIRS + ONE_TILE[:4] + [(1, 8192)],                 # the largest (in tiles) last, after a run of one-tile descriptors
    "t17": [(1030, 40)] + ONE_TILE + PAIRS,                    # the largest first
    "d": [(33, 257)],
    "sq": [(40, 40)],
    "nf": [(33, 257), (31, 255), (32, 256)],
}
SINGLE = [(37, 45), (1, 1), (3, 1100), (1100, 3), (300, 300), (512, 1040)]
Case = namedtuple("Case", "name path shapes data gdata eps fwd_only")


def _cases():
    out = [Case(f"batch-{k}", "batch", tuple(TABLES[k]), "randn", "randn", EPS, False) for k in ("t1", "t2", "t3", "t16", "t17", "sq")]
    for data in ("rank1", "altsign", "scale1e15", "low-end", "high-end"):
        out.append(Case(f"batch-{data}", "batch", tuple(TABLES["d"]), data, "randn", 1e-30 if data == "low-end" else EPS, False))
    for data in ("zero", "scale1e-15"):
        out.append(Case(f"batch-{data}", "batch", tuple(TABLES["d"]), data, "randn", EPS, True))
    out += [Case("batch-G=Wsn", "batch", tuple(TABLES["d"]), "randn", "wsn", EPS, False), Case("batch-G-orthogonal", "batch", tuple(TABLES["d"]), "randn", "orth", EPS, False)]
    out += [Case(f"single-{h}x{w}", "single", ((h, w),), "randn", "randn", EPS, False) for h, w in SINGLE]
    out += [Case("single-rank1", "single", ((37, 45),), "rank1", "randn", EPS, False), Case("single-altsign", "single", ((37, 45),), "altsign", "orth", EPS, False)]
    for data in ("scale1e15", "low-end", "high-end"):          # the single-matrix kernels have their own normalisations: the same data
        out.append(Case(f"single-{data}", "single", (SINGLE[0],), data, "randn", 1e-30 if data == "low-end" else EPS, False))
    for data in ("zero", "scale1e-15"):
        out.append(Case(f"single-{data}", "single", (SINGLE[0],), data, "randn", EPS, True))
    out += [Case("single-G=Wsn", "single", (SINGLE[0],), "randn", "wsn", EPS, False), Case("single-G-orthogonal", "single", (SINGLE[0],), "randn", "orth", EPS, False)]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def case_id(c):
    return c.name


def tiles(h, w):
    return -(-h // SN_RB) * -(-w // SN_CB)


def check_regime(c):
    s = set(c.shapes)
    if c.name == "batch-t3":
        assert tiles(512, 4352) == 272 > 256 and 4352 > 1024 and (512, 4352) == c.shapes[1] and tiles(*c.shapes[0]) == tiles(*c.shapes[2]) == 1
    if c.name in ("batch-t2", "batch-t17"):
        assert (1030, 40) == c.shapes[0] and 1030 > 1024
    if c.name == "batch-t16":
        assert c.shapes[-1] == (1, 8192) and len(c.shapes) == 16 and max(tiles(*x) for x in c.shapes) == tiles(1, 8192)
        assert {h for h, _ in s} >= {1, 31, 32, 33, 64} and {w for _, w in s} >= {1, 255, 256, 257, 300}
    if c.name == "batch-t17":
        assert len(c.shapes) == 17 and max(tiles(*x) for x in c.shapes) == tiles(1030, 40)
    if c.path == "single":
        (h, w), = c.shapes
        n = h * w
        if (h, w) == (3, 1100) or (h, w) == (1100, 3):
            assert max(h, w) > 1024
        if (h, w) == (300, 300):
            assert -(-n // 256) > 256
        if (h, w) == (512, 1040):
            assert -(-n // 256) > 2048


def seed_of(c):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(c.name)) % (2 ** 31)


# ------------------------------------------------------------------------------------------------ data
def make_data(c):
    """per matrix: dict W, u, v, G, dW0 as fp32 CPU tensors"""
    g = torch.Generator().manual_seed(seed_of(c))
    out = []
    for h, w in c.shapes:
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        W = 0.05 * rn(h, w)
        u = torch.nn.functional.normalize(rn(h), dim=0)
        v = torch.nn.functional.normalize(rn(w), dim=0)
        if c.data == "rank1":
            a, b = torch.nn.functional.normalize(rn(h), dim=0), torch.nn.functional.normalize(rn(w), dim=0)
            W = 0.7 * torch.outer(a, b)
        if c.data == "altsign":          # rows alternate in sign under a positive u: the dots cancel, the bound is carried by sum|terms|
            W = W.abs() * (1 - 2 * (torch.arange(h) % 2)).double().view(h, 1)
            u = torch.nn.functional.normalize(u.abs() + 0.1, dim=0)
        if c.data == "zero":
            W = torch.zeros(h, w, dtype=torch.float64)
        if c.data == "scale1e15":
            W = W * 1e15
        if c.data == "scale1e-15":
            W = W * 1e-15
        if c.data == "low-end":           # the median |t_j| is 2^-62: most squares are just normal
            W = W * (2.0 ** -62 / float((W.t() @ u).abs().median()))
        if c.data == "high-end":          # ||t||^2 = 2^125: three powers of two below the overflow of the sum
            W = W * (2.0 ** 62.5 / float((W.t() @ u).norm()))
        W, u, v = W.float(), u.float(), v.float()
        G = rn(h, w)
        if c.gdata in ("wsn", "orth"):
            W64 = W.double()
            if c.gdata == "wsn":
                G = W64 / float(torch.linalg.matrix_norm(W64, 2))
            else:
                G = G - W64 * float((G * W64).sum() / (W64 * W64).sum().clamp_min(1e-300))
        out.append(dict(W=W, u=u, v=v, G=G.float(), dW0=rn(h, w).float()))
    return out


def guarded(ctx, t):
    """a device copy of t with GUARD sentinels behind it -> (buffer, view of the copy)"""
    n = t.numel()
    buf = ctx.f32(n + GUARD, SENT)
    buf[:n] = t.reshape(-1).to(ctx.device)
    return buf, buf[:n].view(t.shape)


def guards_intact(bufs, fill=SENT):
    return all(bool((b[-GUARD:] == fill).all()) for b in bufs)


def run_batch(ctx, c, data=None, ws_fill=WS_FILL):
    ops = ctx.ops
    data = data or make_data(c)
    es, bufs, wsb = [], [], []
    for d in data:
        h, w = d["W"].shape
        e = {}
        for k, t in (("W", d["W"]), ("u", d["u"]), ("v", d["v"]), ("sigma", torch.full((1,), SENT)), ("u_snap", torch.full((h,), SENT)),
                     ("v_snap", torch.full((w,), SENT)), ("G", d["G"]), ("dW", torch.full((h, w), SENT))):
            b, e[k] = guarded(ctx, t)
            bufs.append(b)
        n = ops.spectral_norm_batch_ws_floats(h, w)
        ws = ctx.f32(n + GUARD, ws_fill)
        wsb.append(ws)
        e["ws"] = ws[:n]
        es.append(e)
    f1, f0 = ops.spectral_norm_batch_fwd(es, True, c.eps), ops.spectral_norm_batch_fwd(es, False, c.eps)
    b0, b1 = ops.spectral_norm_batch_bwd(es, False), ops.spectral_norm_batch_bwd(es, True)
    grab = lambda keys: [{k: cpu(e[k]) for k in keys} for e in es]
    res = dict(data=data, is_hip=ops.is_hip)
    f1()
    sync(ctx)
    res["fwd"] = grab(("u", "v", "sigma", "u_snap", "v_snap"))
    if not c.fwd_only:
        b0()
        sync(ctx)
        res["dW"] = grab(("dW",))
        for e, d in zip(es, data):
            e["dW"].copy_(d["dW0"])
        b1()
        sync(ctx)
        res["dW_acc"] = grab(("dW",))
    f0()
    sync(ctx)
    res["fwd0"] = grab(("u", "v", "sigma", "u_snap", "v_snap"))
    for e, d in zip(es, data):          # the same calls from the first state repeat their bits
        e["u"].copy_(d["u"])
        e["v"].copy_(d["v"])
    f1()
    if not c.fwd_only:
        b0()
    sync(ctx)
    again = grab(("u", "v", "sigma", "u_snap", "v_snap") + (() if c.fwd_only else ("dW",)))
    for a, f, dw in zip(again, res["fwd"], res.get("dW", [{}] * len(es))):
        assert all(same_bits(a[k], f[k]) for k in f) and (c.fwd_only or same_bits(a["dW"], dw["dW"])), f"{c.name}: a repeated call gave other bits"
    assert guards_intact(bufs), f"{c.name}: a sentinel behind W, u, v, sigma, a snapshot, G or dW was written"
    assert all(same_bits(cpu(e["W"]), d["W"]) and same_bits(cpu(e["G"]), d["G"]) for e, d in zip(es, data)), f"{c.name}: W or G was written"
    if ops.is_hip:
        assert guards_intact(wsb, ws_fill), f"{c.name}: workspace floats past gan_spectral_norm_batch_ws_floats were written"
    return res


def run_single(ctx, c, data=None):
    ops = ctx.ops
    d, = data or make_data(c)
    h, w = d["W"].shape
    e, bufs = {}, []
    for k, t in (("W", d["W"]), ("u", d["u"]), ("v", d["v"]), ("sigma", torch.full((1,), SENT)), ("Wsn", torch.full((h, w), SENT)), ("G", d["G"]),
                 ("dW", torch.full((h, w), SENT))):
        b, e[k] = guarded(ctx, t)
        bufs.append(b)
    n = ops.spectral_norm_ws_floats(h, w)
    wsbuf = ctx.f32(n + GUARD, WS_FILL)
    ws = wsbuf[:n]
    f1, f0 = (ops.spectral_norm_fwd(e["W"], e["u"], e["v"], pi, c.eps, e["sigma"], e["Wsn"], ws) for pi in (True, False))
    bw = ops.spectral_norm_bwd(e["G"], e["Wsn"], e["u"], e["v"], e["sigma"], e["dW"], ws)
    grab = lambda keys: [{k: cpu(e[k]) for k in keys}]
    res = dict(data=[d], is_hip=ops.is_hip)
    f1()
    if not c.fwd_only:
        bw()
    sync(ctx)
    res["fwd"], res["dW"] = grab(("u", "v", "sigma", "Wsn")), grab(("dW",))
    f0()
    sync(ctx)
    res["fwd0"] = grab(("u", "v", "sigma", "Wsn"))
    e["u"].copy_(d["u"])
    e["v"].copy_(d["v"])
    f1()
    if not c.fwd_only:
        bw()
    sync(ctx)
    again = grab(("u", "v", "sigma", "Wsn", "dW"))[0]
    assert all(same_bits(again[k], res["fwd"][0][k]) for k in res["fwd"][0]) and same_bits(again["dW"], res["dW"][0]["dW"]), f"{c.name}: a repeated call gave other bits"
    assert guards_intact(bufs) and (not ops.is_hip or guards_intact([wsbuf], WS_FILL)), f"{c.name}: a sentinel behind an output or the workspace was written"
    assert same_bits(cpu(e["W"]), d["W"]) and same_bits(cpu(e["G"]), d["G"]), f"{c.name}: W or G was written"
    return res


# ------------------------------------------------------------------------------------------------ bounds
def depths(batch, h, w):
    """levels of each fp32 sum in the kernels' documented orders (module docstring: ORDERS)"""
    cd = lambda a, b: -(-a // b)
    if batch:
        R_, Cb = cd(h, SN_RB), cd(w, SN_CB)
        return dict(t=min(h, SN_RB) + R_, s=4 + 6 + Cb, tt=6 + 4 + cd(Cb, 1024) + 6 + 16, ss=cd(h, 1024) + 6 + 16, sigma=cd(h, 1024) + 6 + 16,
                    gw=min(h, SN_RB) + 6 + 4 + cd(R_ * Cb, 256) + 6 + 4)
    n = h * w
    return dict(t=h, s=cd(w, 256) + 6 + 4, tt=cd(w, 1024) + 6 + 16, ss=cd(h, 1024) + 6 + 16, sigma=cd(h, 1024) + 6 + 16,
                gw=cd(n, min(cd(n, 256), 256) * 256) + 6 + 4 + 1 + 6 + 4)


def dot_tol(absterms, K, depth, extra=0.0):
    return (U * (1.0 + extra) + ks(K, depth)) * absterms


def normalise_tol(x, e_x, eps, depth):
    """(module docstring: NORMALISE) -> elementwise bound on x / max(||x||, eps)"""
    K = x.numel()
    d = float(x.norm())
    sub = int((x * x < 2.0 ** -125).sum())
    e_d = float(e_x.norm()) + d * ((2 * U + ks(K, depth)) / 2 + 2 * U) + min(sub * ETA / max(d, 1e-300), math.sqrt(sub * ETA))
    assert abs(d - eps) > e_d, "the norm is too close to eps to say which branch is taken"
    if d < eps:
        return 1.01 * (e_x / eps + U * (x / eps).abs())
    y = x / d
    return 1.01 * (e_x / d + y.abs() * e_d / d + U * y.abs())


FAMILY = Family("spectral-family", {p + q for p, qs in (("b.", ("v", "u", "sigma", "sigma0", "dW", "dW_acc")), ("s.", ("v", "u", "sigma", "sigma0", "Wsn", "dW")))
                                    for q in qs})
report, worst_table = FAMILY.report, FAMILY.worst_table


def check_case(c, res, ref):
    worst = {}
    batch = c.path == "batch"
    for i, d in enumerate(res["data"]):
        h, w = d["W"].shape
        what = f"{c.name} [{i}] {h}x{w}"
        W, u0, v0, G = (d[k].double() for k in ("W", "u", "v", "G"))
        f, f0 = res["fwd"][i], res["fwd0"][i]
        uw, vw, sg = f["u"].double(), f["v"].double(), float(f["sigma"])
        A, D = W.abs(), depths(batch, h, w)
        # v against normalize(W^T u_in)
        t = W.t() @ u0
        tol_v = normalise_tol(t, dot_tol(A.t() @ u0.abs(), h, D["t"]), c.eps, D["tt"])
        worst["v"] = max(worst.get("v", 0.0), ratio(f["v"], R.v64(W, u0, v0, c.eps, ref), tol_v))
        # u against normalize(W v_written)
        s = W @ vw
        e_s = dot_tol(A @ vw.abs(), w, D["s"], extra=1.0) + U * s.abs() if batch else dot_tol(A @ vw.abs(), w, D["s"])
        worst["u"] = max(worst.get("u", 0.0), ratio(f["u"], R.u64(W, vw, c.eps, ref), normalise_tol(s, e_s, c.eps, D["ss"])))
        # sigma against u_written . (W v_written), after the power iteration and without one
        for name, ff, u_in in (("sigma", f, u0), ("sigma0", f0, uw)):
            tol_s = float((uw.abs() * e_s).sum()) + float(dot_tol((uw * s).abs().sum(), h, D["sigma"])) + ETA
            worst[name] = max(worst.get(name, 0.0), ratio(ff["sigma"][0], R.sigma64(W, u_in, uw, vw, ref), tol_s))
        assert same_bits(f0["u"], f["u"]) and same_bits(f0["v"], f["v"]), f"{what}: u or v was written without a power iteration"
        if batch:
            for ff, ub, vb in ((f, d["u"], d["v"]), (f0, f["u"], f["v"])):
                assert same_bits(ff["u_snap"], R.snap64(ub, ff["u"], ref)) and same_bits(ff["v_snap"], R.snap64(vb, ff["v"], ref)), \
                    f"{what}: the snapshots are not the u, v the statement snapshots"
        else:
            wsn = W / sg
            worst["Wsn"] = max(worst.get("Wsn", 0.0), ratio(f["Wsn"], wsn, U * wsn.abs() + ETA))
            assert same_bits(f0["Wsn"], f["Wsn"]) or abs(float(f0["sigma"]) - sg) > 0, f"{what}: W_sn changed at the same sigma"
        if ref is R.Ref:
            if c.data == "rank1":          # sigma is known in closed form: a ||a_0|| ||b_0|| = 0.7
                assert abs(R.sigma64(W, u0, R.u64(W, R.v64(W, u0, v0, c.eps), c.eps), R.v64(W, u0, v0, c.eps)) - 0.7) < 1e-6
                assert abs(sg - 0.7) < 1e-5, f"{what}: sigma of the rank-one matrix is {sg}"
            if c.data == "zero":
                assert sg == 0.0 and not bool(f["u"].any()) and not bool(f["v"].any()), f"{what}: the eps branch of an all-zero W"
                assert batch or bool(torch.isnan(f["Wsn"]).all()), f"{what}: W_sn of an all-zero W is 0 / 0"
            if c.data == "scale1e-15":
                assert float(t.norm()) < c.eps and float(f["v"].double().norm()) < 0.5, f"{what}: not in the eps branch"
        if c.fwd_only:
            continue
        # dW against the formula at the written sigma and (u, v) with the float64 <G, W>
        Wd = W if batch else f["Wsn"].double()
        gw = R.gw64(G, Wd, ref)
        e_gw = float(dot_tol((G * Wd).abs().sum(), h * w, D["gw"]))
        k_true = R.gw64(G, Wd) / sg if batch else R.gw64(G, Wd)
        k = gw / sg if batch else gw
        e_k = e_gw / abs(sg) + U * abs(k_true) if batch else e_gw
        outer = torch.outer(uw, vw)
        term = k_true * outer
        e_val = e_k * outer.abs() + 2 * U * term.abs() + 2 * ETA
        diff = G - term
        e_val = (e_val + U * diff.abs()) / abs(sg) + U * (diff / sg).abs() + ETA
        worst["dW"] = max(worst.get("dW", 0.0), ratio(res["dW"][i]["dW"], R.dW64(G, k, uw, vw, sg, None, ref), 1.01 * e_val))
        if batch:
            prior = d["dW0"].double()
            want = R.dW64(G, k, uw, vw, sg, prior, ref)
            worst["dW_acc"] = max(worst.get("dW_acc", 0.0), ratio(res["dW_acc"][i]["dW"], want, 1.01 * e_val + U * (prior + diff / sg).abs()))
    for q, r in worst.items():
        report(c, ("b." if batch else "s.") + q, q, r, res["is_hip"])
    bad = {q: v for q, v in worst.items() if not v <= 1.0}
    assert not bad, f"{c.name}: outside the derived bound (error / bound): {bad}"


_results = {}
KEEP = 1 << 20          # results of larger tables are not cached (no wrong reference is tried on them)


def result(make, c):
    ctx = make()
    key = (ctx.device.type, c)
    if key in _results:
        return _results[key]
    check_regime(c)
    res = (run_batch if c.path == "batch" else run_single)(ctx, c)
    if sum(h * w for h, w in c.shapes) < KEEP:
        _results[key] = res
    return res


def body(make, c, ref=None):
    check_case(c, result(make, c), ref or R.Ref)


# ------------------------------------------------------------------------------------------------ wrong references
def _wrong(name, **kw):
    return type(name, (R.Ref,), kw)


WRONG = [
    (_wrong("UNormalisedBeforeV", u_before_v=True), ["batch-t1", "single-37x45"]),
    (_wrong("SigmaFromOldU", sigma_old_u=True), ["batch-t1", "single-300x300"]),
    (_wrong("GradientWithoutDivSigma", no_div_sigma=True), ["batch-t16", "single-37x45"]),
    (_wrong("ProjectionWithUVSwapped", swap_uv=True), ["batch-sq"]),
    (_wrong("DotWithoutLastTile", drop_last_tile=True), ["batch-t1", "batch-t2"]),
    (_wrong("DotWithoutLastRowTile", drop_last_row_tile=True), ["batch-t1", "batch-t2"]),
    (_wrong("AccumulateOverwrites", acc_overwrites=True), ["batch-t1", "batch-t17"]),
    (_wrong("VUnnormalised", v_unnormalised=True), ["batch-t1", "single-3x1100"]),
    (_wrong("EpsAddedNotMax", eps_added=True), ["batch-scale1e-15"]),
    (_wrong("SnapshotsOneIterationStale", stale_snap=True), ["batch-t1", "batch-sq"]),
]


def rejects(make, wrong, names):
    FAMILY.rejects(wrong, [BY_NAME[n] for n in names], lambda c: result(make, c), check_case)


# ------------------------------------------------------------------------------------------------ the non-finite contract
def body_nonfinite(make, where):
    """a NaN in W, u or G of the middle descriptor of three reaches that descriptor's outputs and no other's"""
    ctx = make()
    c = Case("batch-nf-" + where, "batch", tuple(TABLES["nf"]), "randn", "randn", EPS, False)
    clean = run_batch(ctx, c)
    data = make_data(c)
    data[1][where].view(-1)[5] = NAN
    got = run_batch(ctx, c, data)
    for i in (0, 2):
        for part in ("fwd", "dW", "dW_acc", "fwd0"):
            assert all(same_bits(got[part][i][k], clean[part][i][k]) for k in clean[part][i]), f"NaN in {where}: descriptor {i} changed ({part})"
    f = got["fwd"][1]
    if where == "G":
        assert all(same_bits(f[k], clean["fwd"][1][k]) for k in f), "a NaN in G changed the forward"
    else:
        assert all(bool(torch.isnan(f[k]).all()) for k in ("u", "v", "sigma", "u_snap", "v_snap")), f"NaN in {where}: u, v, sigma of its descriptor are not all NaN"
    assert bool(torch.isnan(got["dW"][1]["dW"]).all()) and bool(torch.isnan(got["dW_acc"][1]["dW"]).all()), f"NaN in {where}: dW of its descriptor is not all NaN"


def body_nonfinite_single(make, where):
    """the single-matrix path (include/mi355x_gan.h, gan_spectral_norm_fwd / _bwd).  With a power iteration a NaN in W or u makes every
    element of u, v, sigma and W_sn NaN, a NaN in G leaves the forward alone, and dW is all NaN in each case.  Without one, u and v keep
    their bits, and a NaN in W, u or v makes sigma and every element of W_sn NaN."""
    ctx = make()
    ops = ctx.ops
    c = Case("single-nf-" + where, "single", (SINGLE[0],), "randn", "randn", EPS, False)
    h, w = SINGLE[0]
    if where in ("W", "u", "G"):
        clean = run_single(ctx, c)
        d, = make_data(c)
        d[where].view(-1)[5] = NAN
        got = run_single(ctx, c, [d])
        f = got["fwd"][0]
        if where == "G":
            assert all(same_bits(f[k], clean["fwd"][0][k]) for k in f), "a NaN in G changed the forward"
        else:
            assert all(bool(torch.isnan(f[k]).all()) for k in ("u", "v", "sigma", "Wsn")), f"NaN in {where}: u, v, sigma, W_sn are not all NaN"
        assert bool(torch.isnan(got["dW"][0]["dW"]).all()), f"NaN in {where}: dW is not all NaN"
    if where in ("W", "u", "v"):          # without a power iteration
        d, = make_data(c)
        d[where].view(-1)[5] = NAN
        e, bufs = {}, []
        for k, t in (("W", d["W"]), ("u", d["u"]), ("v", d["v"]), ("sigma", torch.full((1,), SENT)), ("Wsn", torch.full((h, w), SENT))):
            b, e[k] = guarded(ctx, t)
            bufs.append(b)
        n = ops.spectral_norm_ws_floats(h, w)
        wsbuf = ctx.f32(n + GUARD, WS_FILL)
        ops.spectral_norm_fwd(e["W"], e["u"], e["v"], False, c.eps, e["sigma"], e["Wsn"], wsbuf[:n])()
        sync(ctx)
        assert all(same_bits(cpu(e[k]), d[k]) for k in ("W", "u", "v")), f"NaN in {where}, no power iteration: W, u or v was written"
        assert bool(torch.isnan(cpu(e["sigma"])).all()) and bool(torch.isnan(cpu(e["Wsn"])).all()), f"NaN in {where}, no power iteration: sigma or W_sn is not all NaN"
        assert guards_intact(bufs) and (not ops.is_hip or guards_intact([wsbuf], WS_FILL)), f"NaN in {where}: a sentinel was written"


# ------------------------------------------------------------------------------------------------ refused arguments (the C ABI's checks)
def body_refused(make):
    import ctypes as C
    from gan_variant_research_amd._lib import GanError
    ctx = make()
    ops = ctx.ops
    assert ops.is_hip
    h, w = 5, 7
    bufs = {k: ctx.f32(n, SENT) for k, n in (("W", h * w), ("u", h), ("v", w), ("sigma", 1), ("Wsn", h * w), ("G", h * w), ("dW", h * w),
                                              ("ws", ops.spectral_norm_ws_floats(h, w)), ("table", 64))}
    p = lambda k, null: ops._p(None if k == null else bufs[k])

    def fwd(null=None, h_=h, w_=w):
        return ops._call("gan_spectral_norm_fwd", p("W", null), h_, w_, p("u", null), p("v", null), 1, C.c_float(EPS), p("sigma", null), p("Wsn", null),
                         p("ws", null), ops._s())

    def bwd(null=None, h_=h, w_=w):
        return ops._call("gan_spectral_norm_bwd", p("G", null), p("Wsn", null), p("u", null), p("v", null), p("sigma", null), h_, w_, p("dW", null),
                         p("ws", null), ops._s())
    calls = {f"fwd {k} NULL": (lambda k=k: fwd(k)) for k in ("W", "u", "v", "sigma", "Wsn", "ws")}
    calls.update({f"bwd {k} NULL": (lambda k=k: bwd(k)) for k in ("G", "Wsn", "u", "v", "sigma", "dW", "ws")})
    calls.update({"fwd h 0": lambda: fwd(h_=0), "fwd w -1": lambda: fwd(w_=-1), "bwd h 0": lambda: bwd(h_=0), "bwd w 0": lambda: bwd(w_=0)})
    for name, args in (("descs NULL", (ops._p(None), 1, 1)), ("n 0", (ops._p(bufs["table"]), 0, 1)), ("total_blocks 0", (ops._p(bufs["table"]), 1, 0))):
        calls[f"batch_fwd {name}"] = lambda a=args: ops._call("gan_spectral_norm_batch_fwd", a[0], a[1], a[2], 1, C.c_float(EPS), ops._s())
        calls[f"batch_bwd {name}"] = lambda a=args: ops._call("gan_spectral_norm_batch_bwd", a[0], a[1], a[2], 0, ops._s())
    for name, call in calls.items():
        with pytest.raises(GanError):
            call()()
        sync(ctx)
        assert all(bool((b == SENT).all()) for b in bufs.values()), f"{name}: a refused call wrote a buffer"
    assert ops.spectral_norm_batch_ws_floats(0, 5) == 0 and ops.spectral_norm_batch_ws_floats(5, -1) == 0
