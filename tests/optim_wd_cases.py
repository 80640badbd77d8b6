"""TEST INFRASTRUCTURE: cases, derived bounds and assertions for gan_adam_step_wd (csrc/optim.hip: the decaying instantiations of
adam_apply_kernel), written against an op layer: tests/test_optim_wd_cpu.py runs them on tests/emulator_optim_wd.py, tests/test_optim_wd_gpu.py
on HipOps, with the same tables and assertions.  The float64 statement is tests/optim_wd_ref64.py.  Tables, layout, E and the norm bound are
those of tests/optim_cases.py, whose conventions (u = 2^-24, eta = 2^-126, NORM, COEFFICIENT, ELEMENTS, NON-FINITE) hold here unchanged:

  NORM / COEFFICIENT.  norm_out[0 .. 2] are held to exactly the statements of tests/optim_cases.py: the norm of the scaled gradients alone.
  A decay that reached the norm would move it by about wd |p| / |g| relative, thousands of times the bound.
  ELEMENTS.  `replay_wd` extends the operation-by-operation replay of adam_apply_kernel by the new operations, none fitted:
    L2:         g_eff = g gs + wd p_old: one product (u of itself + eta) and one sum (u) in front of the chain; m, v, p then propagate the
                error of g_eff exactly as they propagate that of g gs.  An fma in their place only removes a rounding.
    decoupled:  keep = 1 - rate wd: one product, one difference; p' = p_old keep: one product; p = p' - step_size (m / denom): the final
                subtraction as before, now with the error of p' among its operands.
  Skipped tensors (g == NULL), a step skipped for a non-finite norm, step counters, sentinels and a repeated call are compared bit for bit --
  against the STATEMENT's value, so a statement that decays where the kernel must not is rejected.
"""
import math

import numpy as np
import pytest
import torch

from tests import optim_cases as P
from tests import optim_ref64 as R
from tests import optim_wd_ref64 as W
from tests.optim_cases import E, ETA, GUARD, SENT, U, WS_FILL, Case, Layout, check_cover, chunks_of
from tests.pointwise_cases import cpu, same_bits, sync, t32

DEFAULT = {**P.DEFAULT, "wd": 0.1, "decoupled": False, "pzero": False, "all_live": False}
TABLES = P.TABLES
MODES = (("l2", False), ("dec", True))


def _case(name, table, **kw):
    assert set(kw) <= set(DEFAULT), kw
    return Case(name, table, tuple(sorted(kw.items())))


def opt_of(c):
    return {**DEFAULT, **dict(c.opt)}


def _cases():
    out = []
    for tag, dec in MODES:
        k = dict(decoupled=dec)
        out += [_case(f"{tag}-sizes", "sizes", step0="ramp", **k), _case(f"{tag}-sizes-unaligned", "sizes", aligned=False, step0="ramp", wd=1e-4, **k),
                _case(f"{tag}-sizes-3steps", "sizes", nsteps=3, step0="ramp", max_norm=1.0, **k), _case(f"{tag}-skipmid", "skipmid", max_norm=1.0, **k)]
        for wd in (0.1, 1e-4):
            out += [_case(f"{tag}-wd{wd}-clip-hard", "small", wd=wd, max_norm=0.01, **k), _case(f"{tag}-wd{wd}-no-clip", "small", wd=wd, max_norm=0.0, step0=3, **k)]
        out += [_case(f"{tag}-gradscaler", "small", grad_scale=0.5, inv_scale=0.3, skip=1, **k), _case(f"{tag}-lr-dev", "small", lr_dev=1e-2, lr=2e-4, **k),
                _case(f"{tag}-lr-dev-ema0", "small", lr_dev=1e-2, lr=2e-4, ema_decay=0.0, step0=3, **k), _case(f"{tag}-no-ema", "small", ema=False, **k),
                _case(f"{tag}-step0=3-3steps", "small", step0=3, nsteps=3, **k), _case(f"{tag}-zero-g", "small", gkind="zero", pzero=True, lr_dev=1e-2, **k)]
        for nf in ("nan", "pinf", "ninf"):
            for skip in (0, 1):
                for mn in (10.0, 0.0):
                    out.append(_case(f"{tag}-{nf}-skip{skip}-clip{mn}", "small", nf=nf, skip=skip, max_norm=mn, **k))
            out.append(_case(f"{tag}-{nf}-in-skipped-tensor", "small", nf=nf + "-unread", **k))
        for b, kw in (("fused_adam", dict(lr_dev=2e-4)), ("launch", dict(all_live=True)), ("hipadam", dict(lr_dev=2e-4))):
            out += [_case(f"{tag}-{b}-sizes", "sizes", builder=b, **kw, **k),
                    _case(f"{tag}-{b}-skipmid", "skipmid", builder=b, max_norm=1.0, **{**kw, **(dict(ema=False) if b == "hipadam" else {})}, **k)]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
case_id = P.case_id


def make_state(c):
    """optim_cases.make_state; `pzero`: every third parameter of the first tensor is exactly 0; `all_live`: every tensor has its gradient
    (training.fused_adam_launch takes a gradient per tensor)"""
    o = opt_of(c)
    state = P.make_state(Case(c.name, c.table, tuple((k, v) for k, v in c.opt if k in P.DEFAULT)))
    if o["pzero"]:
        state[0]["p"][::3] = 0.0
        assert not bool(state[0]["g"].any()) and bool((state[0]["p"] == 0).any()) and bool((state[0]["p"] != 0).any())
    if o["all_live"]:
        g = torch.Generator().manual_seed(P.seed_of(c) + 1)
        for t in state:
            if t["g"] is None:
                t["g"] = torch.randn(t["p"].numel(), generator=g)
    return state


def _wd_args(o):
    return float(o["wd"]), bool(o["decoupled"])


def run_adam(ctx, c):
    """-> dict: per step (before, after, norm_out), as optim_cases.run_adam, through the builder the case names"""
    o = opt_of(c)
    ops = ctx.ops
    state = make_state(c)
    sizes = [t["p"].numel() for t in state]
    dev = ctx.device
    lr_dev = torch.tensor([o["lr_dev"]], dtype=torch.float32, device=dev) if o["lr_dev"] is not None else None
    inv = torch.tensor([o["inv_scale"]], dtype=torch.float32, device=dev) if o["inv_scale"] is not None else None
    wd, dec = _wd_args(o)
    res = dict(steps=[], is_hip=ops.is_hip)
    if o["builder"] == "own":
        lay = Layout(ctx, sizes, o["aligned"], o["ema"])
        lay.load(state)
        ct, co = chunks_of(sizes)
        check_cover(sizes, ct, co)
        nch = len(ct)
        norm, ws = ctx.f32(3 + GUARD, SENT), ctx.f32(nch + GUARD, WS_FILL)
        table = ops.make_adam_table(lay.entries(state))
        op = ops.adam_step_wd(table, len(sizes), torch.tensor(ct, dtype=torch.int32, device=dev), torch.tensor(co, dtype=torch.int64, device=dev), nch,
                              o["lr"], o["b1"], o["b2"], o["eps"], o["max_norm"], o["grad_scale"], o["ema_decay"], norm, ws, wd, dec, lr_dev=lr_dev,
                              inv_scale=inv, skip_nonfinite=bool(o["skip"]))
        for s in range(o["nsteps"]):
            before, snap = lay.read(state), P._snapshot(lay)
            op()
            sync(ctx)
            after, n1, w1 = lay.read(state), cpu(norm), cpu(ws)
            assert lay.gaps_intact(), f"{c.name}: a sentinel between the tensor slices was written"
            assert bool((n1[3:] == SENT).all()), f"{c.name}: norm_out past [0 .. 3) was written"
            if res["is_hip"]:
                assert bool((w1[nch:] == WS_FILL).all()), f"{c.name}: workspace floats past ws[0 .. nchunks) were written"
            mid = P._snapshot(lay)
            P._restore(lay, snap)            # the same call on the restored state repeats its bits
            norm.fill_(SENT)
            op()
            sync(ctx)
            again = P._snapshot(lay)
            assert all(same_bits(cpu(again[0][k]), cpu(mid[0][k])) for k in lay.flat) and torch.equal(again[1], mid[1]) and same_bits(cpu(norm), n1), \
                f"{c.name}: a repeated call gave other bits"
            res["steps"].append((before, after, n1[:3]))
    elif o["builder"] == "fused_adam":
        from gan_variant_research_amd.cut import FusedAdam
        names = [f"t{i}" for i in range(len(sizes))]
        opt = FusedAdam(ctx, names, [torch.Size([n]) for n in sizes], {n: t["p"] for n, t in zip(names, state)}, lr=o["lr_dev"], betas=(o["b1"], o["b2"]),
                        eps=o["eps"], weight_decay=wd, ema_decay=o["ema_decay"] if o["ema"] else None, decoupled=dec)
        check_cover(sizes, opt.chunk_tensor.tolist(), opt.chunk_off.tolist())
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
    elif o["builder"] == "launch":
        from gan_variant_research_amd import training as T
        assert all(t["g"] is not None for t in state)
        d = lambda k: [t[k].clone().to(dev) for t in state]
        ps, gs_, ms, vs, es = d("p"), d("g"), d("m"), d("v"), d("ema")
        steps = torch.tensor([t["step"] for t in state], dtype=torch.int32, device=dev)
        T._FUSED_PLANS.clear()
        n0, f0 = T.fused_adam_launch(ps, gs_, ms, vs, es, steps, o["lr"], o["b1"], o["b2"], o["eps"], o["max_norm"], o["grad_scale"], o["ema_decay"],
                                     weight_decay=wd, decoupled=dec)
        sync(ctx)
        (pl,) = T._FUSED_PLANS.values()
        check_cover(sizes, pl["ct"].tolist(), pl["co"].tolist())
        after = [dict(p=cpu(ps[i]), g=t["g"], m=cpu(ms[i]), v=cpu(vs[i]), ema=cpu(es[i]), step=int(steps[i])) for i, t in enumerate(state)]
        n1 = cpu(pl["norm"])[:3]
        assert float(n0) == float(n1[0]) and float(f0) == float(n1[2])
        T._FUSED_PLANS.clear()
        res["steps"].append((state, after, n1))
    else:
        from gan_variant_research_amd import training as T
        assert o["builder"] == "hipadam" and o["grad_scale"] == 1.0 and inv is None
        params = [torch.nn.Parameter(t["p"].clone().to(dev)) for t in state]
        opt = T.HipAdam(params, lr=o["lr_dev"], betas=(o["b1"], o["b2"]), eps=o["eps"], weight_decay=wd, decoupled_weight_decay=dec)
        shadow = [t["ema"].clone().to(dev) for t in state] if o["ema"] else None
        if shadow is not None:
            opt.attach_ema({id(p): s for p, s in zip(params, shadow)}, o["ema_decay"])
        for p, t in zip(params, state):
            opt.state[p] = {"exp_avg": t["m"].clone().to(dev), "exp_avg_sq": t["v"].clone().to(dev),
                            "step": torch.tensor([t["step"]], dtype=torch.int32, device=dev)}
            p.grad = t["g"].clone().to(dev) if t["g"] is not None else None
        opt.step(max_grad_norm=o["max_norm"] if o["max_norm"] > 0 else None)
        sync(ctx)
        after = [dict(p=cpu(p.data), g=t["g"], m=cpu(opt.state[p]["exp_avg"]), v=cpu(opt.state[p]["exp_avg_sq"]),
                      ema=cpu(shadow[i]) if shadow is not None else None, step=int(opt.state[p]["step"])) for i, (p, t) in enumerate(zip(params, state))]
        res["steps"].append((state, after, cpu(opt.last_grad_norm)[:3]))
    return res


# ------------------------------------------------------------------------------------------------ bounds
def replay_wd(t, o, coef, rate):
    """adam_apply_kernel<WD_L2 / WD_DECOUPLED> on one live tensor, operation by operation (optim_cases.replay plus the module docstring's
    new operations) -> E of (p, m, v, ema): only the error bounds are used"""
    f = lambda x: t32(x)
    d = lambda k: E(t[k].double())
    gsc = E(f(o["grad_scale"])) * f(o["inv_scale"]) if o["inv_scale"] is not None else E(f(o["grad_scale"]))
    gs = gsc * coef
    b1, b2, dec, wd = f(o["b1"]), f(o["b2"]), f(o["ema_decay"]), f(o["wd"])
    w1, w2, we = 1.0 - E(b1), 1.0 - E(b2), 1.0 - E(dec)
    gi, mi, vi, p0 = d("g") * gs, d("m"), d("v"), d("p")
    if o["decoupled"]:
        p0 = p0 * (1.0 - E(rate) * wd)
    else:
        gi = gi + E(wd) * p0
    if float(np.float32(1.0) - np.float32(b1)) < 0.5:
        mi = mi + w1 * (gi - mi)
    else:
        mi = gi - (gi - mi) * (1.0 - w1)
    vi = vi * b2 + (w2 * gi) * gi
    step = t["step"] + 1
    bc1, bc2s = E.rounded(1.0 - b1 ** step), E.rounded(math.sqrt(1.0 - b2 ** step))
    denom = vi.sqrt() / bc2s + f(o["eps"])
    pi = p0 - (E(rate) / bc1) * (mi / denom)
    ema = we * pi + E(dec) * d("ema") if t["ema"] is not None else None
    return pi, mi, vi, ema


FAMILY = P.Family("optim-wd", {"norm", "coef"} | {f"{tag}-{k}" for tag, _ in MODES for k in ("p", "m", "v", "ema")})
report, worst_table = FAMILY.report, FAMILY.worst_table


def check_adam(c, res, ref):
    o = opt_of(c)
    f = t32
    wd, dec = f(o["wd"]), bool(o["decoupled"])
    tag = "dec" if dec else "l2"
    worst = {}
    for s, (before, after, norm) in enumerate(res["steps"]):
        what = f"{c.name} step {s}"
        b64 = [{k: (v.double() if torch.is_tensor(v) else v) for k, v in t.items()} for t in before]
        inv = f(o["inv_scale"]) if o["inv_scale"] is not None else None
        gs = f(o["grad_scale"]) * (inv if inv is not None else 1.0)
        rate_true = f(o["lr_dev"]) if o["lr_dev"] is not None else f(o["lr"])
        wrote_norm, wrote_coef, wrote_found = (float(x) for x in norm)
        lr_arg = f(o["lr"]) if o["builder"] in ("own", "launch") else rate_true          # FusedAdam and HipAdam pass the rate both ways
        args = (lr_arg, f(o["b1"]), f(o["b2"]), f(o["eps"]), f(o["max_norm"]), f(o["grad_scale"]), inv, f(o["ema_decay"]), bool(o["skip"]), wd, dec)
        lrd = f(o["lr_dev"]) if o["lr_dev"] is not None else None
        want_norm, _, _, _ = W.step64_wd(b64, *args, lr_dev=lrd, ref=ref)
        sizes = [t["p"].numel() for t in before]
        K = sum(t["g"].numel() for t in before if t["g"] is not None)
        tol_n = P.norm_bound(R.sumsq64(b64, gs), K, len(chunks_of(sizes)[0]))
        worst[f"norm/{s}"] = P.ratio(torch.tensor(wrote_norm), want_norm, tol_n)
        want_coef = R.coef64(wrote_norm, f(o["max_norm"]), ref)
        worst[f"coef/{s}"] = P.ratio(torch.tensor(wrote_coef), want_coef, 2.02 * U * abs(want_coef) if math.isfinite(want_coef) else 0.0)
        assert wrote_found == float(R.found_inf64(wrote_norm)), f"{what}: norm_out[2] = {wrote_found} at the norm {wrote_norm}"
        check_elements(o, what, s, before, after, args, lrd, wrote_coef, bool(o["skip"]) and wrote_found == 1.0, rate_true, worst, ref)
        if ref is W.WdRef:
            P.check_contract(c, o, before, after, wrote_norm, wrote_coef, wrote_found, what)
            check_zero_gradient(c, o, before, after, what)
    for q, r in worst.items():
        report(c, q.split("/")[0], q, r, res["is_hip"])
    bad = {q: v for q, v in worst.items() if not v <= 1.0}
    assert not bad, f"{c.name}: outside the derived bound (error / bound): {bad}"


def check_elements(o, what, s, before, after, args, lrd, wrote_coef, skipped_all, rate_true, worst, ref=W.WdRef):
    """m, v, p, ema and the counters of every tensor against the float64 step from `before` with the coefficient the kernel wrote; the
    tensors may be any subset of the elements (the update is elementwise once the coefficient is known)"""
    tag = "dec" if o["decoupled"] else "l2"
    b64 = [{k: (v.double() if torch.is_tensor(v) else v) for k, v in t.items()} for t in before]
    _, _, _, want = W.step64_wd(b64, *args, lr_dev=lrd, coef=wrote_coef, ref=ref)
    for i, (tb, ta, tw) in enumerate(zip(before, after, want)):
        step_want = tb["step"] if skipped_all else tw["step"]           # (a subset of the gradients cannot tell whether the step was skipped)
        assert ta["step"] == step_want, f"{what}: step counter of tensor {i} is {ta['step']}, the statement gives {step_want}"
        if tb["g"] is None or skipped_all:      # the statement leaves such a tensor as it was: bit for bit what the statement holds
            keys = [k for k in ("p", "m", "v", "ema") if tb[k] is not None]
            assert all(same_bits(ta[k], tb[k]) for k in keys), f"{what}: tensor {i} takes no step and was written"
            assert all(bool(((ta[k].double() == tw[k]) | (torch.isnan(ta[k]) & torch.isnan(tw[k]))).all()) for k in keys), \
                f"{what}: tensor {i} takes no step; the statement changes it"
            continue
        assert same_bits(ta["g"], tb["g"]), f"{what}: the gradient of tensor {i} was written"
        pi, mi, vi, ema = replay_wd(dict(b64[i]), o, wrote_coef, rate_true)
        for k, e in (("p", pi), ("m", mi), ("v", vi), ("ema", ema)):
            if e is not None:
                q = f"{tag}-{k}/{s}"
                worst[q] = max(worst.get(q, 0.0), P.ratio(ta[k], tw[k], e.e, lerp_inf=(k == "m")))


def check_zero_gradient(c, o, before, after, what):
    """an exactly-zero gradient (with zero moments): L2 takes an Adam step on wd p, decoupled only shrinks, and p == 0 stays 0"""
    if not o["pzero"]:
        return
    p0, p1 = before[0]["p"].double(), after[0]["p"].double()
    z = p0 == 0
    assert bool((p1[z] == 0).all()), f"{what}: a zero parameter with a zero gradient moved"
    assert bool(((p0 - p1)[~z].sign() == p0[~z].sign()).all()), f"{what}: the decay did not move p towards 0"
    if o["decoupled"]:
        assert bool((p1[~z].abs() < p0[~z].abs()).all()) and bool((p1[~z].sign() == p0[~z].sign()).all()), f"{what}: the decay did not shrink p"
        assert not bool(after[0]["m"].any()) and not bool(after[0]["v"].any()), f"{what}: decoupled decay reached m or v"
    else:
        assert bool((after[0]["m"][~z] != 0).all()) and bool((after[0]["v"][~z] != 0).all()), f"{what}: L2 decay did not reach m and v"


_results = {}


def result(make, c):
    ctx = make()
    key = (ctx.device.type, c)
    if key not in _results:
        P.check_regime(c)
        _results[key] = run_adam(ctx, c)
    return _results[key]


def body(make, c, ref=None):
    check_adam(c, result(make, c), ref or W.WdRef)


# ------------------------------------------------------------------------------------------------ wrong references
def _wrong(name, **kw):
    return type(name, (W.WdRef,), kw)


WRONG = [
    (_wrong("DecayInsideTheNorm", wd_in_norm=True), ["l2-sizes", "dec-skipmid", "l2-wd0.1-no-clip"]),
    (_wrong("DecayBeforeTheClip", wd_before_clip=True), ["l2-wd0.1-clip-hard", "l2-skipmid"]),
    (_wrong("DecayOnSkippedTensors", wd_on_skipped=True), ["l2-skipmid", "dec-skipmid", "dec-fused_adam-skipmid", "l2-hipadam-skipmid"]),
    (_wrong("DecayOnASkippedNonFiniteStep", wd_on_nonfinite_skip=True), ["dec-nan-skip1-clip10.0", "l2-pinf-skip1-clip0.0"]),
    (_wrong("OtherMode", swap_mode=True), ["l2-sizes", "dec-sizes", "l2-fused_adam-sizes", "dec-launch-sizes", "dec-hipadam-sizes"]),
    (_wrong("DecoupledFactorAfterTheUpdate", decoupled_after=True), ["dec-lr-dev", "dec-lr-dev-ema0"]),
    (_wrong("DecoupledFactorFromLrArgument", decoupled_lr_from_arg=True), ["dec-lr-dev", "dec-zero-g"]),
    (_wrong("VFromUndecayedGradient", v_undecayed=True), ["l2-sizes", "l2-wd0.1-no-clip"]),
    (_wrong("EmaFromUndecayedP", ema_undecayed_p=True), ["dec-lr-dev-ema0", "l2-lr-dev-ema0"]),
]


def rejects(make, wrong, names):
    FAMILY.rejects(wrong, [BY_NAME[n] for n in names], lambda c: result(make, c), check_adam)


# ------------------------------------------------------------------------------------------------ weight_decay = 0 is gan_adam_step
def body_zero_decay_is_adam_step(make, decoupled):
    """the new entry with weight_decay = 0 against the old entry on the same state, two chained steps: p, m, v, ema, steps, norm_out bit for bit"""
    ctx = make()
    ops = ctx.ops
    c = P.BY_NAME["sizes-3steps"]
    o = P.opt_of(c)
    outs = []
    for new in (False, True):
        state = P.make_state(c)
        sizes = [t["p"].numel() for t in state]
        lay = Layout(ctx, sizes, True, True)
        lay.load(state)
        ct, co = chunks_of(sizes)
        norm, ws = ctx.f32(3 + GUARD, SENT), ctx.f32(len(ct) + GUARD, WS_FILL)
        a = (ops.make_adam_table(lay.entries(state)), len(sizes), torch.tensor(ct, dtype=torch.int32, device=ctx.device),
             torch.tensor(co, dtype=torch.int64, device=ctx.device), len(ct), o["lr"], o["b1"], o["b2"], o["eps"], o["max_norm"], o["grad_scale"],
             o["ema_decay"], norm, ws)
        op = ops.adam_step_wd(*a, 0.0, decoupled) if new else ops.adam_step(*a)
        trail = []
        for _ in range(2):
            op()
            sync(ctx)
            trail.append(({k: cpu(v) for k, v in lay.flat.items()}, lay.steps.cpu().clone(), cpu(norm)))
        outs.append(trail)
    for (fa, sa, na), (fb, sb, nb) in zip(*outs):
        assert all(same_bits(fa[k], fb[k]) for k in fa) and torch.equal(sa, sb) and same_bits(na, nb), \
            "gan_adam_step_wd(weight_decay = 0) and gan_adam_step differ"


# ------------------------------------------------------------------------------------------------ refused arguments
REFUSED = {"weight_decay < 0": (-0.1, 0, "weight_decay"), "weight_decay NaN": (float("nan"), 1, "weight_decay"),
           "decoupled 2": (0.1, 2, "decoupled"), "decoupled -1": (0.1, -1, "decoupled"), "decoupled 2 without decay": (0.0, 2, "decoupled")}


def body_refused(make):
    """each returns -1 with its message and launches nothing (HipOps only: the checks are the C ABI's)"""
    import ctypes as C
    from gan_variant_research_amd._lib import GanError
    ctx = make()
    ops = ctx.ops
    assert ops.is_hip
    dev = ctx.device
    c = BY_NAME["l2-wd0.1-no-clip"]
    state = make_state(c)
    sizes = [t["p"].numel() for t in state]
    lay = Layout(ctx, sizes, True, True)
    lay.load(state)
    snap = P._snapshot(lay)
    ct, co = chunks_of(sizes)
    ctd, cod = torch.tensor(ct, dtype=torch.int32, device=dev), torch.tensor(co, dtype=torch.int64, device=dev)
    norm, ws = ctx.f32(3 + GUARD, SENT), ctx.f32(len(ct) + GUARD, WS_FILL)
    table = ops.make_adam_table(lay.entries(state))

    def call(wd, dec, table=table):
        fl = C.c_float
        return ops._call("gan_adam_step_wd", ops._p(table), len(sizes), ops._p(ctd), ops._p(cod), len(ct), fl(2e-4), fl(0.5), fl(0.999), fl(1e-8), fl(10.0),
                         fl(1.0), fl(0.999), ops._p(None), ops._p(None), 0, fl(wd), int(dec), ops._p(norm), ops._p(ws), ops._s())
    calls = {name: (lambda v=v: call(v[0], v[1])) for name, v in REFUSED.items()}
    calls["table NULL"] = lambda: call(0.1, 0, table=None)
    for name, mk in calls.items():
        with pytest.raises(GanError) as ei:
            mk()()
        word = REFUSED[name][2] if name in REFUSED else "bad arguments"
        assert word in str(ei.value), f"{name}: the message is {ei.value}"
        sync(ctx)
        now = P._snapshot(lay)
        assert all(same_bits(cpu(now[0][k]), cpu(snap[0][k])) for k in lay.flat) and torch.equal(now[1], snap[1]), f"{name}: a refused call wrote a tensor"
        assert bool((norm == SENT).all()) and bool((ws == WS_FILL).all()), f"{name}: a refused call wrote norm_out or the workspace"
