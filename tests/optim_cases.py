"""TEST INFRASTRUCTURE: cases, derived bounds and assertions for the optimiser kernels (csrc/optim.hip: gan_adam_step, gan_scaler_update)
and the fp32 helpers of csrc/util.hip (gan_fill_f32, gan_axpy_f32), written against an op layer: tests/test_optim_family_cpu.py runs them
on the emulator, tests/test_optim_family_gpu.py on HipOps, with the same tables and the same assertions.  The float64 statements are in
tests/optim_ref64.py.

Bounds (convention of tests/cases.py: BOUND_C, U_F32 = 2^-24 =: u, sqrt(K); eta = 2^-126 where a product may underflow); none of them is
fitted to a result.  Inputs are the stored fp32 values and the floats the C ABI receives.

  NORM.  norm_out[0] = sqrtf(S), S the fp32 sum of K squares (g * gs)^2, gs = fl(grad_scale * *inv_scale).  A term errs by 5u of itself
  (the scale product, the scaled gradient -- twice, it is squared -- and the square) + 2 eta; the sum by ks(K, D) S, with the documented
  order of adam_sumsq_kernel and adam_apply_kernel: a thread's <= 64 trips, the wave butterfly (6), the block's 4 waves, then
  ceil(nchunks / 256) trips over the partials, 6, 4 (tests/pointwise_cases.py: SUM).  The square root halves the relative error
  (|sqrt(S') - sqrt(S)| = |S' - S| / (sqrt(S') + sqrt(S))) and rounds itself: sqrtf 1 ulp = 2u (HIP's documented accuracy).
  COEFFICIENT.  norm_out[1] is held to the float64 coefficient AT THE NORM THE KERNEL WROTE: the sum and the division round, 2u (x 1.01).
  norm_out[2] is exact: 1 where the written norm is not finite.
  ELEMENTS.  m, v, p and ema are held to the float64 step taken from the state before the call WITH THE COEFFICIENT THE KERNEL WROTE.
  `E` carries a float64 value with a bound on the error of its fp32 evaluation and replays adam_apply_kernel operation by operation:
  every +, -, * adds u of its own result to the propagated errors of its operands (a product also eta); a division the same (IEEE
  division, as the library is compiled); sqrtf 2u of its result on top of min(e / sqrt(x), sqrt(e)) for an operand error e (the second
  form carries x = 0: v = 0 and g = 0 give 0 / eps); bc1 = (float)(1 - b1^t) and sqrt(bc2) are float64 values rounded once (u);
  lr / bc1 is an fp32 division.  Both arms of at::lerp are replayed as written, chosen as the kernel chooses (fp32 1 - beta1 < 0.5).
  An fma in place of a product and a sum only removes a rounding.  Several steps are chained from the kernel's own state, so nothing
  compounds.  Step counters, skipped tensors (g == NULL), sentinels and a repeated call are compared bit for bit.
  NON-FINITE.  Where the float64 value is NaN the result must be NaN; where it is +-Inf the result must be the same Inf, except for m,
  where it must be non-finite (the second arm of at::lerp, g - (g - m) beta1, turns an Inf gradient into Inf - Inf; torch does the
  same); elsewhere it must be finite and inside the bound.
  RANGE.  The squares stay normal in fp32 for 2^-63 <= |g gs| < 2^64 / sqrt(K) (the upper end keeps their sum finite too); below, the
  bound is carried by eta; above, the norm is Inf and the non-finite contract applies.
  SCALER.  scale * factor rounds once, 1 / scale once more.  FILL is exact.  AXPY: y + a x with or without contraction: u (|a x| + |y'|).
"""
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

from gan_variant_research_amd.runtime import ADAM_CHUNK
from tests import optim_ref64 as R
from tests.cases import U_F32
from tests.pointwise_cases import Fl, cpu, ks, same_bits, sync, t32
from tests.pointwise_cases import ratio as strict_ratio

U = U_F32
ETA = 2.0 ** -126
SENT, WS_FILL = 7.5, 3e5
GUARD = 64
NAN, INF = float("nan"), float("inf")
BUMP_BLOCK, PARTIAL_THREADS, GRID_CAP = 64, 256, 2048 * 256       # documented constants of csrc/optim.hip and csrc/util.hip


class E(Fl):
    """Fl (tests/pointwise_cases.py: +, -, *) with the division, the square root and a value rounded once (module docstring: ELEMENTS)"""

    @staticmethod
    def rounded(v):
        """a float64 value rounded once to fp32"""
        v = torch.tensor(float(v), dtype=torch.float64)
        return E(v, U * v.abs())

    def __truediv__(self, o):
        o = self.of(o)
        v = self.v / o.v
        low = (o.v.abs() - o.e).clamp_min(1e-300)
        return E(v, (self.e + v.abs() * o.e) / low + U * v.abs() + ETA)

    def sqrt(self):
        v = torch.sqrt(self.v)
        return E(v, torch.minimum(self.e / v.clamp_min(1e-300), torch.sqrt(self.e)) + 2 * U * v)


# ------------------------------------------------------------------------------------------------ cases
DEFAULT = dict(lr=2e-4, lr_dev=None, b1=0.5, b2=0.999, eps=1e-8, max_norm=10.0, grad_scale=1.0, inv_scale=None, ema=True, ema_decay=0.999,
               step0=0, skip=0, gkind="randn", gmag=1.0, nsteps=1, nf=None, aligned=True, builder="own")
TABLES = {      # (numel, live)
    "sizes": [(1, 1), (3, 1), (16383, 1), (16384, 1), (16385, 1), (2 * 16384 + 1, 1)],
    "ones300": [(1, int(i % 3 != 0)) for i in range(300)],
    "skipmid": [(5000, 1), (16385, 0), (7, 1)],
    "small": [(40, 1), (5, 0), (3, 1), (1, 1)],
}
N_SMALL = 44          # live elements of "small"
Case = namedtuple("Case", "name table opt")


def _case(name, table, **kw):
    assert set(kw) <= set(DEFAULT), kw
    return Case(name, table, tuple(sorted(kw.items())))


def opt_of(c):
    return {**DEFAULT, **dict(c.opt)}


def _cases():
    out = [_case("sizes", "sizes", step0="ramp"), _case("sizes-unaligned", "sizes", aligned=False, step0="ramp"),
           _case("sizes-3steps", "sizes", nsteps=3, step0="ramp", max_norm=1.0),
           _case("ones300", "ones300", step0="ramp"), _case("skipmid", "skipmid", max_norm=1.0),
           _case("fusedadam-builder", "sizes", builder="fused_adam", lr_dev=2e-4), _case("fusedadam-builder-skip", "skipmid", builder="fused_adam", lr_dev=2e-4),
           _case("launch-builder", "sizes", builder="launch")]
    for b1 in (0.0, 0.4, 0.5, 0.9):
        for b2 in (0.9, 0.999):
            out.append(_case(f"b1={b1}-b2={b2}", "small", b1=b1, b2=b2, step0=3))
    out += [_case(f"step0={s}", "small", step0=s, b1=0.9) for s in (0, 1, 999, 10 ** 6)]
    out += [_case("eps=1e-3", "small", eps=1e-3), _case("eps=1e-8", "small", eps=1e-8, step0=5),
            _case("no-ema", "small", ema=False), _case("ema-decay-0", "small", ema_decay=0.0), _case("ema-decay-0.999", "small", ema_decay=0.999, step0=2),
            _case("no-clip", "small", max_norm=0.0), _case("no-clip-negative", "small", max_norm=-1.0),
            _case("clip-hard", "small", max_norm=0.01), _case("clip-tiny-norm", "small", max_norm=1e-5, gmag=1e-5 / math.sqrt(N_SMALL)),
            _case("gradscaler", "small", grad_scale=0.5, inv_scale=0.3, skip=1), _case("lr-dev", "small", lr_dev=1e-3, lr=2e-4),
            _case("zero-g-zero-v", "small", gkind="zero")]
    for mn in (0.0, 1.0):       # the range of the squares (module docstring: RANGE): outside below, just inside both ends, and 1e18
        out += [_case(f"g=1e-20-clip{mn}", "small", gkind="mag", gmag=1e-20, max_norm=mn),
                _case(f"g-low-end-clip{mn}", "small", gkind="mag", gmag=2.4 * 2.0 ** -63, max_norm=mn),
                _case(f"g=1e18-clip{mn}", "small", gkind="mag", gmag=1e18, max_norm=mn),
                _case(f"g-high-end-clip{mn}", "small", gkind="mag", gmag=0.9 * 2.0 ** 64 / math.sqrt(N_SMALL), max_norm=mn)]
    for nf in ("nan", "pinf", "ninf"):
        for skip in (0, 1):
            for mn in (10.0, 0.0):
                out.append(_case(f"{nf}-skip{skip}-clip{mn}", "small", nf=nf, skip=skip, max_norm=mn))
        out.append(_case(f"{nf}-in-skipped-tensor", "small", nf=nf + "-unread"))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def case_id(c):
    return c.name


def chunks_of(sizes):
    ct, co = [], []
    for i, n in enumerate(sizes):
        for off in range(0, n, ADAM_CHUNK):
            ct.append(i)
            co.append(off)
    return ct, co


def check_cover(sizes, ct, co):
    """every element of every tensor lies in exactly one chunk"""
    seen = [np.zeros(n, dtype=np.int32) for n in sizes]
    for i, off in zip(ct, co):
        assert 0 <= i < len(sizes) and 0 <= off < sizes[i], (i, off)
        seen[i][off:min(off + ADAM_CHUNK, sizes[i])] += 1
    assert all(bool((s == 1).all()) for s in seen), "the chunk table does not cover every element exactly once"


def check_regime(c):
    """the table reaches the edge it is listed for, from the kernels' documented constants"""
    tb = TABLES[c.table]
    ct, co = chunks_of([n for n, _ in tb])
    if c.table == "sizes":
        assert [n for n, _ in tb] == [1, 3, ADAM_CHUNK - 1, ADAM_CHUNK, ADAM_CHUNK + 1, 2 * ADAM_CHUNK + 1] and len(ct) == 9
    if c.table == "ones300":
        assert len(ct) > PARTIAL_THREADS and -(-len(tb) // BUMP_BLOCK) == 5
        dead = [k for k, i in enumerate(ct) if not tb[i][1]]
        assert any(k < PARTIAL_THREADS for k in dead) and any(k >= PARTIAL_THREADS for k in dead)
    if c.table == "skipmid":
        assert not tb[1][1] and tb[1][0] == ADAM_CHUNK + 1 and tb[0][1] and tb[2][1] and ct == [0, 1, 1, 2]
    if c.table == "small":
        assert sum(n for n, live in tb if live) == N_SMALL


def seed_of(c):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(c.name)) % (2 ** 31)


# ------------------------------------------------------------------------------------------------ data
def make_state(c):
    """per tensor: dict p, g (None: skipped), m, v, ema (or None) as fp32 CPU tensors and step (int)"""
    o = opt_of(c)
    tb = TABLES[c.table]
    g = torch.Generator().manual_seed(seed_of(c))
    out = []
    for i, (n, live) in enumerate(tb):
        rn = lambda s=1.0: (torch.randn(n, generator=g, dtype=torch.float64) * s).float()
        t = dict(p=rn(), m=rn(0.1), v=rn(0.1) ** 2, ema=rn() if o["ema"] else None, g=None,
                 step=(i % 7 if o["step0"] == "ramp" else int(o["step0"])))
        grad = rn(o["gmag"])
        if o["gkind"] == "mag":
            sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
            grad = (sign * o["gmag"] * (0.5 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64))).float()
            t["m"], t["v"] = (t["m"].double() * o["gmag"]).float(), (t["v"].double() * o["gmag"] ** 2).float()
        if o["gkind"] == "zero" and i == 0:
            grad, t["m"], t["v"] = torch.zeros(n), torch.zeros(n), torch.zeros(n)
        if live:
            t["g"] = grad
        out.append(t)
    nf = o["nf"]
    if nf:
        bad = {"nan": NAN, "pinf": INF, "ninf": -INF}[nf.split("-")[0]]
        if nf.endswith("unread"):
            dead = next(t for t in out if t["g"] is None)
            dead["p"][1], dead["m"][2], dead["v"][0] = bad, bad, abs(bad)
        else:
            out[2]["g"][1] = bad
    return out


class Layout:
    """flat p, g, m, v, ema buffers with a sentinel gap before, between and after the slices (aligned: every slice starts at a multiple of
    4 floats, as cut.FusedAdam places them; unaligned: odd starts)"""

    def __init__(self, ctx, sizes, aligned, with_ema):
        offs, at = [], 4 if aligned else 3
        for n in sizes:
            offs.append(at)
            at += n + (((-n) % 4) + 4 if aligned else 1 + n % 2)
        self.offs, self.sizes, self.total = offs, sizes, at + 4
        assert all(o % 4 == 0 for o in offs) if aligned else any(o % 4 for o in offs)
        names = ("p", "g", "m", "v") + (("ema",) if with_ema else ())
        self.flat = {k: torch.full((self.total,), SENT, dtype=torch.float32, device=ctx.device) for k in names}
        self.steps = torch.zeros(len(sizes), dtype=torch.int32, device=ctx.device)
        self.gap = torch.ones(self.total, dtype=torch.bool)
        for o_, n in zip(offs, sizes):
            self.gap[o_:o_ + n] = False

    def slice(self, k, i):
        return self.flat[k][self.offs[i]:self.offs[i] + self.sizes[i]]

    def load(self, state):
        for i, t in enumerate(state):
            for k in self.flat:
                if t.get(k) is not None:
                    self.slice(k, i).copy_(t[k])
            self.steps[i] = t["step"]

    def entries(self, state):
        return [dict(p=self.slice("p", i), g=self.slice("g", i) if t["g"] is not None else None, m=self.slice("m", i), v=self.slice("v", i),
                     ema=self.slice("ema", i) if "ema" in self.flat else None, step=self.steps[i:i + 1]) for i, t in enumerate(state)]

    def read(self, state):
        out = []
        steps = self.steps.cpu()
        for i, t in enumerate(state):
            d = {k: cpu(self.slice(k, i)) for k in self.flat}
            d.setdefault("ema", None)
            d["g"] = d["g"] if t["g"] is not None else None
            d["step"] = int(steps[i])
            out.append(d)
        return out

    def gaps_intact(self):
        return all(bool((f.cpu()[self.gap] == SENT).all()) for f in self.flat.values())


def _snapshot(lay):
    return {k: f.clone() for k, f in lay.flat.items()}, lay.steps.clone()


def _restore(lay, snap):
    for k, f in snap[0].items():
        lay.flat[k].copy_(f)
    lay.steps.copy_(snap[1])


def run_adam(ctx, c):
    """-> dict: per step (before, after, norm_out) with the tensors as make_state lists, and what was compared bit for bit on the way"""
    o = opt_of(c)
    ops = ctx.ops
    state = make_state(c)
    sizes = [t["p"].numel() for t in state]
    dev = ctx.device
    lr_dev = torch.tensor([o["lr_dev"]], dtype=torch.float32, device=dev) if o["lr_dev"] is not None else None
    inv = torch.tensor([o["inv_scale"]], dtype=torch.float32, device=dev) if o["inv_scale"] is not None else None
    res = dict(steps=[], is_hip=ops.is_hip)
    if o["builder"] == "own":
        lay = Layout(ctx, sizes, o["aligned"], o["ema"])
        lay.load(state)
        ct, co = chunks_of(sizes)
        check_cover(sizes, ct, co)
        nch = len(ct)
        norm, ws = ctx.f32(3 + GUARD, SENT), ctx.f32(nch + GUARD, WS_FILL)
        table = ops.make_adam_table(lay.entries(state))
        op = ops.adam_step(table, len(sizes), torch.tensor(ct, dtype=torch.int32, device=dev), torch.tensor(co, dtype=torch.int64, device=dev), nch,
                           o["lr"], o["b1"], o["b2"], o["eps"], o["max_norm"], o["grad_scale"], o["ema_decay"], norm, ws, lr_dev=lr_dev, inv_scale=inv,
                           skip_nonfinite=bool(o["skip"]))
        for s in range(o["nsteps"]):
            before, snap = lay.read(state), _snapshot(lay)
            op()
            sync(ctx)
            after, n1, w1 = lay.read(state), cpu(norm), cpu(ws)
            assert lay.gaps_intact(), f"{c.name}: a sentinel between the tensor slices was written"
            assert bool((n1[3:] == SENT).all()), f"{c.name}: norm_out past [0 .. 3) was written"
            if res["is_hip"]:
                assert bool((w1[nch:] == WS_FILL).all()), f"{c.name}: workspace floats past ws[0 .. nchunks) were written"
            mid = _snapshot(lay)
            _restore(lay, snap)            # the same call on the restored state repeats its bits
            norm.fill_(SENT)
            op()
            sync(ctx)
            again = _snapshot(lay)
            assert all(same_bits(cpu(again[0][k]), cpu(mid[0][k])) for k in lay.flat) and torch.equal(again[1], mid[1]) and same_bits(cpu(norm), n1), \
                f"{c.name}: a repeated call gave other bits"
            res["steps"].append((before, after, n1[:3]))
    elif o["builder"] == "fused_adam":
        from gan_variant_research_amd.cut import FusedAdam
        names = [f"t{i}" for i in range(len(sizes))]
        opt = FusedAdam(ctx, names, [torch.Size([n]) for n in sizes], {n: t["p"] for n, t in zip(names, state)}, lr=o["lr_dev"], betas=(o["b1"], o["b2"]),
                        eps=o["eps"], ema_decay=o["ema_decay"] if o["ema"] else None)
        check_cover(sizes, opt.chunk_tensor.tolist(), opt.chunk_off.tolist())
        assert all(int(a) % 4 == 0 for a in opt.offsets), "FusedAdam's slices are 16-byte aligned"
        sl = lambda f, i: f[int(opt.offsets[i]):int(opt.offsets[i]) + sizes[i]]
        flats = dict(p=opt.flat_p, g=opt.flat_g, m=opt.flat_m, v=opt.flat_v, ema=opt.flat_ema)
        gap = torch.ones(opt.flat_p.numel(), dtype=torch.bool)
        for i, t in enumerate(state):
            gap[int(opt.offsets[i]):int(opt.offsets[i]) + sizes[i]] = False
        for k, f in flats.items():
            if f is not None:
                f[gap.to(dev)] = SENT
                for i, t in enumerate(state):
                    sl(f, i).copy_(t[k] if t[k] is not None else torch.zeros(sizes[i]))
        opt.steps.copy_(torch.tensor([t["step"] for t in state], dtype=torch.int32))
        read = lambda: [dict(p=cpu(sl(opt.flat_p, i)), g=cpu(sl(opt.flat_g, i)) if t["g"] is not None else None, m=cpu(sl(opt.flat_m, i)),
                             v=cpu(sl(opt.flat_v, i)), ema=cpu(sl(opt.flat_ema, i)) if o["ema"] else None, step=int(opt.steps[i])) for i, t in enumerate(state)]
        before = read()
        opt.step_op(o["max_norm"], o["grad_scale"], skip=[n for n, t in zip(names, state) if t["g"] is None])()
        sync(ctx)
        assert all(bool((f.cpu()[gap] == SENT).all()) for f in flats.values() if f is not None), f"{c.name}: the padding between FusedAdam's slices was written"
        res["steps"].append((before, read(), cpu(opt.norm_out)[:3]))
    else:
        from gan_variant_research_amd import training as T
        assert all(t["g"] is not None for t in state) and o["builder"] == "launch"
        d = lambda k: [t[k].clone().to(dev) for t in state]
        ps, gs_, ms, vs, es = d("p"), d("g"), d("m"), d("v"), d("ema")
        steps = torch.tensor([t["step"] for t in state], dtype=torch.int32, device=dev)
        T._FUSED_PLANS.clear()
        n0, f0 = T.fused_adam_launch(ps, gs_, ms, vs, es, steps, o["lr"], o["b1"], o["b2"], o["eps"], o["max_norm"], o["grad_scale"], o["ema_decay"])
        sync(ctx)
        (pl,) = T._FUSED_PLANS.values()
        check_cover(sizes, pl["ct"].tolist(), pl["co"].tolist())
        after = [dict(p=cpu(ps[i]), g=t["g"], m=cpu(ms[i]), v=cpu(vs[i]), ema=cpu(es[i]), step=int(steps[i])) for i, t in enumerate(state)]
        n1 = cpu(pl["norm"])[:3]
        assert float(n0) == float(n1[0]) and float(f0) == float(n1[2])
        T._FUSED_PLANS.clear()
        res["steps"].append((state, after, n1))
    return res


# ------------------------------------------------------------------------------------------------ bounds
def norm_bound(S, K, nchunks, kterms=5.05):
    """(module docstring: NORM) bound on |norm_out[0] - sqrt(S)| for the float64 sum S of K squares"""
    depth = min(K, ADAM_CHUNK // 256) + 6 + 4 + -(-nchunks // PARTIAL_THREADS) + 6 + 4
    es = (kterms * U + ks(max(K, 1), depth)) * S + 2 * K * ETA
    root = math.sqrt(S)
    return es / max(root + math.sqrt(max(S - es, 0.0)), 1e-300) + 2 * U * root if S > 0 else math.sqrt(es)


def replay(t, o, coef, rate):
    """adam_apply_kernel on one live tensor, operation by operation -> E of (p, m, v, ema): only the error bounds are used"""
    f = lambda x: t32(x)
    d = lambda k: E(t[k].double())
    gsc = E(f(o["grad_scale"])) * f(o["inv_scale"]) if o["inv_scale"] is not None else E(f(o["grad_scale"]))
    gs = gsc * coef
    b1, b2, dec = f(o["b1"]), f(o["b2"]), f(o["ema_decay"])
    w1, w2, we = 1.0 - E(b1), 1.0 - E(b2), 1.0 - E(dec)
    gi, mi, vi = d("g") * gs, d("m"), d("v")
    if float(np.float32(1.0) - np.float32(b1)) < 0.5:
        mi = mi + w1 * (gi - mi)
    else:
        mi = gi - (gi - mi) * (1.0 - w1)
    vi = vi * b2 + (w2 * gi) * gi
    step = t["step"] + 1
    bc1, bc2s = E.rounded(1.0 - b1 ** step), E.rounded(math.sqrt(1.0 - b2 ** step))
    denom = vi.sqrt() / bc2s + f(o["eps"])
    pi = d("p") - (E(rate) / bc1) * (mi / denom)
    ema = we * pi + E(dec) * d("ema") if t["ema"] is not None else None
    return pi, mi, vi, ema


def ratio(got, ref, tol, lerp_inf=False):
    """max |got - ref| / tol (module docstring: NON-FINITE).  The rule of tests/pointwise_cases.py -- NaN for NaN, the same Inf for an Inf --
    except for m (lerp_inf), where any non-finite value stands for an Inf."""
    if not lerp_inf:
        return strict_ratio(got, ref, tol)
    got = got.double()
    ref = torch.as_tensor(ref, dtype=torch.float64).expand_as(got)
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(got)
    fin = torch.isfinite(ref)
    if bool((torch.isnan(ref) & ~torch.isnan(got)).any()) or bool((~fin & torch.isfinite(got)).any()) or bool((fin & ~torch.isfinite(got)).any()):
        return INF
    r = ((got - ref).abs() / (tol + 1e-300))[fin]
    assert not bool(torch.isnan(r).any()), "NaN in a tolerance"
    return float(r.max()) if r.numel() else 0.0


class Family:
    """the bookkeeping every family keeps: the worst error / bound per group and op layer, and the wrong references (shared with
    tests/spectral_cases.py)"""

    def __init__(self, tag, groups):
        self.tag, self.groups, self.worst, self.rejecting = tag, set(groups), {}, []

    def report(self, c, group, q, r, hip):
        if self.rejecting:
            print(f"[{self.tag}] (against the wrong reference {self.rejecting[0]}) {c.name} {q}: {r:.3g}")
        else:
            self.worst[(hip, group)] = max(self.worst.get((hip, group), 0.0), r)
            print(f"[{self.tag}] {c.name} {q}: error / bound = {r:.3g}")
        return r

    def worst_table(self, hip):
        """the worst error / bound per group of what ran on the kernels (hip) or on the emulator; every group has to be there, so the
        idle-bound check cannot pass on a table that the cases never filled or that the other op layer filled"""
        worst = {g: r for (h, g), r in sorted(self.worst.items()) if h == hip}
        for group, r in worst.items():
            print(f"[{self.tag}] WORST {group}: error / bound = {r:.3g}")
        assert set(worst) == self.groups, f"groups without a figure: {sorted(self.groups - set(worst))}; unknown: {sorted(set(worst) - self.groups)}"
        return worst

    def rejects(self, wrong, cases, result, check):
        """the results held to the wrong reference fail on every case listed for it"""
        failed = []
        self.rejecting.append(wrong.__name__)
        try:
            for c in cases:
                res = result(c)
                try:
                    check(c, res, wrong)
                except AssertionError as e:
                    failed.append((c.name, str(e)[:100]))
        finally:
            self.rejecting.clear()
        print(f"[{self.tag}] {wrong.__name__} rejected on {failed}")
        assert len(failed) == len(cases), f"the assertions accept the wrong reference {wrong.__name__} on a case it was tried on"


FAMILY = Family("optim-family", {"norm", "coef", "p", "m", "v", "ema", "scaler", "axpy"})
report, worst_table = FAMILY.report, FAMILY.worst_table


def check_adam(c, res, ref):
    o = opt_of(c)
    f = t32
    worst = {}
    for s, (before, after, norm) in enumerate(res["steps"]):
        what = f"{c.name} step {s}"
        b64 = [{k: (v.double() if torch.is_tensor(v) else v) for k, v in t.items()} for t in before]
        inv = f(o["inv_scale"]) if o["inv_scale"] is not None else None
        gs = f(o["grad_scale"]) * (inv if inv is not None else 1.0)
        rate_true = f(o["lr_dev"]) if o["lr_dev"] is not None else f(o["lr"])
        wrote_norm, wrote_coef, wrote_found = (float(x) for x in norm)
        args = (f(o["lr"]), f(o["b1"]), f(o["b2"]), f(o["eps"]), f(o["max_norm"]), f(o["grad_scale"]), inv, f(o["ema_decay"]), bool(o["skip"]))
        lrd = f(o["lr_dev"]) if o["lr_dev"] is not None else None
        # the norm, against the statement's own; the coefficient and found_inf at the norm the kernel wrote
        want_norm, _, _, _ = R.step64(b64, *args, lr_dev=lrd, ref=ref)
        sizes = [t["p"].numel() for t in before]
        K = sum(t["g"].numel() for t in before if t["g"] is not None)
        tol_n = norm_bound(R.sumsq64(b64, gs), K, len(chunks_of(sizes)[0]))
        worst[f"norm/{s}"] = ratio(torch.tensor(wrote_norm), want_norm, tol_n)
        want_coef = R.coef64(wrote_norm, f(o["max_norm"]), ref)
        worst[f"coef/{s}"] = ratio(torch.tensor(wrote_coef), want_coef, 2.02 * U * abs(want_coef) if math.isfinite(want_coef) else 0.0)
        assert wrote_found == float(R.found_inf64(wrote_norm)), f"{what}: norm_out[2] = {wrote_found} at the norm {wrote_norm}"
        # the elements and the counters, with the coefficient the kernel wrote
        _, _, _, want = R.step64(b64, *args, lr_dev=lrd, coef=wrote_coef, ref=ref)
        skipped_all = bool(o["skip"]) and wrote_found == 1.0
        for i, (tb, ta, tw) in enumerate(zip(before, after, want)):
            assert ta["step"] == tw["step"], f"{what}: step counter of tensor {i} is {ta['step']}, the statement gives {tw['step']}"
            if tb["g"] is None or skipped_all:
                keys = [k for k in ("p", "m", "v", "ema") if tb[k] is not None]
                assert all(same_bits(ta[k], tb[k]) for k in keys), f"{what}: tensor {i} takes no step and was written"
                continue
            assert same_bits(ta["g"], tb["g"]), f"{what}: the gradient of tensor {i} was written"
            t64 = dict(b64[i])
            pi, mi, vi, ema = replay(t64, o, wrote_coef, rate_true)
            for k, e in (("p", pi), ("m", mi), ("v", vi), ("ema", ema)):
                if e is not None:
                    q = f"{k}/{s}"
                    worst[q] = max(worst.get(q, 0.0), ratio(ta[k], tw[k], e.e, lerp_inf=(k == "m")))
        if ref is R.Ref:
            check_contract(c, o, before, after, wrote_norm, wrote_coef, wrote_found, what)
    for q, r in worst.items():
        report(c, q.split("/")[0], q, r, res["is_hip"])
    bad = {q: v for q, v in worst.items() if not v <= 1.0}
    assert not bad, f"{c.name}: outside the derived bound (error / bound): {bad}"


def check_contract(c, o, before, after, norm, coef, found, what):
    """the non-finite and range contracts of include/mi355x_gan.h, stated on the results themselves"""
    nf = o["nf"]
    live = [i for i, t in enumerate(before) if t["g"] is not None]
    if nf is None or nf.endswith("unread"):
        assert found == 0.0 and math.isfinite(norm), what
        assert all(bool(torch.isfinite(after[i][k]).all()) for i in live for k in ("p", "m", "v")), f"{what}: a live tensor went non-finite"
        return
    assert found == 1.0 and not math.isfinite(norm) and math.isnan(norm) == (nf == "nan"), f"{what}: norm_out[0] = {norm}"
    if o["skip"]:
        return                                  # check_adam has compared every tensor and counter bit for bit
    clip = o["max_norm"] > 0
    assert (math.isnan(coef) if (clip and nf == "nan") else coef == (0.0 if clip else 1.0)), f"{what}: the coefficient is {coef}"
    for i in live:
        bad = ~torch.isfinite(before[i]["g"])
        for k in ("p", "m", "v"):
            if clip and nf == "nan":
                assert bool(torch.isnan(after[i][k]).all()), f"{what}: {k} of tensor {i} is not all NaN under a NaN coefficient"
            else:               # an Inf under clipping: Inf * 0 = NaN there, a zero gradient everywhere else; without clipping only the element
                assert torch.equal(~torch.isfinite(after[i][k]), bad), f"{what}: {k} of tensor {i} is non-finite elsewhere than at the non-finite gradient"
                if clip:
                    assert bool(torch.isnan(after[i][k][bad]).all()), what


_results = {}


def result(make, c):
    ctx = make()
    key = (ctx.device.type, c)
    if key not in _results:
        check_regime(c)
        _results[key] = run_adam(ctx, c)
    return _results[key]


def body(make, c, ref=None):
    check_adam(c, result(make, c), ref or R.Ref)


# ------------------------------------------------------------------------------------------------ wrong references
def _wrong(name, **kw):
    return type(name, (R.Ref,), kw)


WRONG = [
    (_wrong("NormWithoutLastChunk", drop_last_chunk=True), ["skipmid", "ones300"]),
    (_wrong("NormWithoutTensorTails", drop_tail=True), ["sizes", "skipmid"]),
    (_wrong("BiasCorrectionAtStep", bc_offset=0), ["step0=1", "b1=0.9-b2=0.999"]),
    (_wrong("EpsInsideSqrt", eps_inside_sqrt=True), ["eps=1e-3", "sizes"]),
    (_wrong("EmaFromOldP", ema_old_p=True), ["ema-decay-0", "sizes"]),
    (_wrong("CoefficientWithout1e-6", clip_eps=0.0), ["clip-tiny-norm"]),
    (_wrong("GradScaleAfterClipOnly", scale_after_clip_only=True), ["gradscaler"]),
    (_wrong("VFromUnclippedGradient", v_unclipped=True), ["clip-hard", "skipmid"]),
    (_wrong("SkippedCounterBumped", bump_skipped=True), ["ones300", "skipmid"]),
    (_wrong("LrFromArgument", lr_from_arg=True), ["lr-dev"]),
]


def rejects(make, wrong, names):
    FAMILY.rejects(wrong, [BY_NAME[n] for n in names], lambda c: result(make, c), check_adam)


# ------------------------------------------------------------------------------------------------ gan_scaler_update
SCALER_SEQS = {      # (found_inf per call, interval, growth, backoff, first scale)
    "clean-clean-overflow-clean": ([0, 0, 1, 0], 2, 2.0, 0.5, 1024.0),
    "interval-1": ([0, 0, 1, 0], 1, 2.0, 0.5, 3.0),
    "odd-factors": ([0, 1, 0, 0, 0], 2, 1.7, 0.3, 0.7),
    "tiny-scale-backoff": ([1, 1, 0], 2, 2.0, 0.3, 3e-38),          # the scale goes subnormal and 1 / scale overflows: Inf, as 1.f / x gives
}


def body_scaler(make, name):
    ctx = make()
    ops = ctx.ops
    found_seq, interval, growth, backoff, s0 = SCALER_SEQS[name]
    buf = ctx.f32(4 + GUARD, SENT)          # scale, inv_scale, found_inf, and sentinels
    tracker = torch.tensor([0, 77], dtype=torch.int32, device=ctx.device)
    buf[0], buf[1] = s0, SENT
    op = ops.scaler_update(buf[0:1], buf[1:2], tracker[0:1], buf[2:3], growth, backoff, interval)
    scale, trk, worst = t32(s0), 0, 0.0
    c = Case("scaler-" + name, None, ())
    for fi in found_seq:
        buf[2] = float(fi)
        op()
        sync(ctx)
        got = cpu(buf)
        want_s, _, trk = R.scaler_update64(scale, trk, fi, t32(growth), t32(backoff), interval)
        r = ratio(got[0], want_s, U * abs(want_s) + 2.0 ** -150)
        scale = float(got[0])                                        # the next call starts from the scale the kernel wrote
        want_inv = 1.0 / scale if scale != 0 else INF
        want_inv = want_inv if abs(want_inv) <= R.F32_MAX * (1 + U / 2) else math.copysign(INF, want_inv)
        r = max(r, ratio(got[1], want_inv, U * abs(want_inv) + 2.0 ** -150 if math.isfinite(want_inv) else 0.0))
        worst = max(worst, r)
        assert int(tracker[0]) == trk and int(tracker[1]) == 77, f"{name}: growth tracker {tracker.tolist()}, the statement gives {trk}"
        assert float(got[2]) == float(fi) and bool((got[3:] == SENT).all()), f"{name}: found_inf or a sentinel was written"
    report(c, "scaler", "scale, inv_scale", worst, ops.is_hip)
    assert worst <= 1.0, f"{name}: error / bound = {worst}"


# ------------------------------------------------------------------------------------------------ gan_fill_f32, gan_axpy_f32
HELPER_N = [0, 1, 255, 256, 257, 2048 * 256 + 1]
FILL_VALUES = [1.25, -0.0, NAN, INF, -INF, 1e-45]


def _fill_op(ops, buf, n, val):
    """fill of buf[0:n).  An empty torch view has a null data pointer, which the C ABI refuses whatever n is (body_refused), so n = 0 goes
    to the entry point with the buffer's own pointer: a valid pointer and nothing to write."""
    if n == 0 and ops.is_hip:
        import ctypes as C
        return ops._call("gan_fill_f32", ops._p(buf), C.c_int64(0), C.c_float(val), ops._s())
    return ops.fill(buf[:n], val)


def _axpy_op(ops, ybuf, xbuf, n, a):
    if n == 0 and ops.is_hip:
        import ctypes as C
        return ops._call("gan_axpy_f32", ops._p(ybuf), ops._p(xbuf), C.c_float(a), C.c_int64(0), ops._s())
    return ops.axpy(ybuf[:n], xbuf[:n], a)


def body_fill_axpy(make, n):
    ctx = make()
    ops = ctx.ops
    assert n != HELPER_N[-1] or -(-n // GRID_CAP) == 2           # the second trip of the capped grid
    c = Case(f"helpers-n{n}", None, ())
    for val in FILL_VALUES if n <= 257 else FILL_VALUES[:2]:
        buf = ctx.f32(n + GUARD, SENT)
        _fill_op(ops, buf, n, val)()
        sync(ctx)
        got = cpu(buf)
        assert same_bits(got[:n], torch.full((n,), val, dtype=torch.float32)), f"fill n={n} value {val}: not the value's bits"
        assert bool((got[n:] == SENT).all()), f"fill n={n}: wrote past n"
    g = torch.Generator().manual_seed(n + 1)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a = 0.7
    ybuf = ctx.f32(n + GUARD, SENT)
    ybuf[:n] = y.to(ctx.device)
    xd = ctx.f32(n + GUARD, SENT)
    xd[:n] = x.to(ctx.device)
    _axpy_op(ops, ybuf, xd, n, a)()
    sync(ctx)
    got = cpu(ybuf)
    assert bool((got[n:] == SENT).all()) and same_bits(cpu(xd)[:n], x) and bool((cpu(xd)[n:] == SENT).all()), f"axpy n={n}: wrote past n or into x"
    ax = t32(a) * x.double()
    want = y.double() + ax
    r = ratio(got[:n], want, U * (ax.abs() + want.abs()) + ETA)
    report(c, "axpy", "y", r, ops.is_hip)
    assert r <= 1.0, f"axpy n={n}: error / bound = {r}"
    ybuf2 = ctx.f32(n + GUARD, SENT)
    ybuf2[:n] = y.to(ctx.device)
    _axpy_op(ops, ybuf2, xd, n, a)()
    sync(ctx)
    assert same_bits(cpu(ybuf2), got), f"axpy n={n}: a repeated call gave other bits"


# ------------------------------------------------------------------------------------------------ refused arguments (the C ABI's checks)
def body_refused(make):
    """each returns its error and launches nothing (HipOps only: the checks are the C ABI's)"""
    import ctypes as C
    from gan_variant_research_amd._lib import GanError
    ctx = make()
    ops = ctx.ops
    assert ops.is_hip
    dev = ctx.device
    c = BY_NAME["b1=0.5-b2=0.999"]
    state = make_state(c)
    sizes = [t["p"].numel() for t in state]
    lay = Layout(ctx, sizes, True, True)
    lay.load(state)
    snap = _snapshot(lay)
    ct, co = chunks_of(sizes)
    ctd, cod = torch.tensor(ct, dtype=torch.int32, device=dev), torch.tensor(co, dtype=torch.int64, device=dev)
    norm, ws = ctx.f32(3 + GUARD, SENT), ctx.f32(len(ct) + GUARD, WS_FILL)
    table = ops.make_adam_table(lay.entries(state))
    good = dict(table=table, ntensors=len(sizes), ct=ctd, co=cod, nchunks=len(ct), norm=norm, ws=ws)

    def adam(**bad):
        a = {**good, **bad}
        fl = C.c_float
        return ops._call("gan_adam_step", ops._p(a["table"]), a["ntensors"], ops._p(a["ct"]), ops._p(a["co"]), a["nchunks"], fl(2e-4), fl(0.5), fl(0.999),
                         fl(1e-8), fl(10.0), fl(1.0), fl(0.999), ops._p(None), ops._p(None), 0, ops._p(a["norm"]), ops._p(a["ws"]), ops._s())
    sc = ctx.f32(3 + GUARD, SENT)
    trk = torch.tensor([5], dtype=torch.int32, device=dev)
    fbuf = ctx.f32(16, SENT)

    def scaler(growth=2.0, backoff=0.5, interval=2, **null):
        p = lambda k, t: ops._p(None if k in null else t)
        return ops._call("gan_scaler_update", p("scale", sc[0:1]), p("inv", sc[1:2]), p("tracker", trk), p("found", sc[2:3]), C.c_float(growth),
                         C.c_float(backoff), int(interval), ops._s())
    calls = {
        "adam table NULL": lambda: adam(table=None), "adam chunk_tensor NULL": lambda: adam(ct=None), "adam chunk_off NULL": lambda: adam(co=None),
        "adam norm_out NULL": lambda: adam(norm=None), "adam ws NULL": lambda: adam(ws=None), "adam ntensors 0": lambda: adam(ntensors=0),
        "adam nchunks 0": lambda: adam(nchunks=0), "adam nchunks -1": lambda: adam(nchunks=-1),
        "scaler growth < 1": lambda: scaler(growth=0.5), "scaler backoff 0": lambda: scaler(backoff=0.0), "scaler backoff > 1": lambda: scaler(backoff=1.5),
        "scaler interval 0": lambda: scaler(interval=0), "scaler scale NULL": lambda: scaler(scale=None), "scaler found_inf NULL": lambda: scaler(found=None),
        "fill NULL": lambda: ops._call("gan_fill_f32", ops._p(None), C.c_int64(4), C.c_float(1.0), ops._s()),
        "fill n < 0": lambda: ops._call("gan_fill_f32", ops._p(fbuf), C.c_int64(-1), C.c_float(1.0), ops._s()),
        "axpy y NULL": lambda: ops._call("gan_axpy_f32", ops._p(None), ops._p(fbuf), C.c_float(1.0), C.c_int64(4), ops._s()),
        "axpy x NULL": lambda: ops._call("gan_axpy_f32", ops._p(fbuf), ops._p(None), C.c_float(1.0), C.c_int64(4), ops._s()),
        "axpy n < 0": lambda: ops._call("gan_axpy_f32", ops._p(fbuf), ops._p(fbuf), C.c_float(1.0), C.c_int64(-4), ops._s()),
    }
    for name, call in calls.items():
        with pytest.raises(GanError):
            call()()
        sync(ctx)
        now = _snapshot(lay)
        assert all(same_bits(cpu(now[0][k]), cpu(snap[0][k])) for k in lay.flat) and torch.equal(now[1], snap[1]), f"{name}: a refused call wrote a tensor"
        assert bool((norm == SENT).all()) and bool((ws == WS_FILL).all()), f"{name}: a refused call wrote norm_out or the workspace"
        assert bool((sc == SENT).all()) and int(trk) == 5 and bool((fbuf == SENT).all()), f"{name}: a refused call wrote its output"
