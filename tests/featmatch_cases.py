"""TEST INFRASTRUCTURE: cases, bounds and assertions for the feature-matching term (csrc/featmatch.hip, nets.DPass hooks, cut.CutTrainer with
loss_weights.featmatch, cut.MultiscaleDiscriminator.get_intermediate_features, losses.feature_matching_loss), written against an op layer:
tests/test_featmatch_cpu.py runs the bodies on tests/emulator_featmatch.py, tests/test_featmatch_gpu.py on HipOps, with the same shapes and
the same assertions.  The float64 statement is tests/featmatch_ref64.py.

Bounds (none fitted to a result).  A loss of the kernel: the header's derived bound, tests/featmatch_ref64.loss_bound with the header's chain
length L, and no other.  A gradient of the kernel: bit-identical to the header's fp32 statement.  The trainer's term end to end against
float64 torch: the project's fp32 parity margin, 1e-3 relative (README, "Parity").  Inputs are bf16-representable, so fp32 and bf16 views and
the float64 statement read the same numbers."""
import math

import numpy as np
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd import cut as C
from gan_variant_research_amd._lib import ACT_LRELU, ACT_NONE, GanError
from gan_variant_research_amd.runtime import View
from tests import cases
from tests import featmatch_ref64 as R
from tests import palette_cases as PC

TDT = {BF16: torch.bfloat16, F32: torch.float32}
NAME = {BF16: "bf16", F32: "fp32"}
SENT = 7.5                                    # exact in bf16 and fp32
LOSS_SCALE, GRAD_SCALE, PREFILL = 0.25, 0.7, 1.5
# (B, H, W, view C, real C, halo f, halo r, halo g)
SHAPES = [(1, 1, 1, 8, 8, 0, 0, 0), (2, 3, 5, 8, 3, 1, 1, 2), (3, 31, 31, 64, 64, 1, 1, 2), (1, 2, 2, 512, 512, 1, 1, 1), (2, 16, 16, 128, 128, 1, 0, 1),
          (1, 31, 31, 512, 512, 1, 1, 2)]
SHAPE_ID = lambda s: "B%d_%dx%d_C%d_r%d_h%d%d%d" % s
MEASURED = []                                 # (label, error, allowance) of every loss check, for profiles/featmatch_accuracy.txt

sync, same_bits = PC.sync, PC.same_bits


def make_view(x, Cv, dtype, halo, device, fill):
    """(B,H,W,Cr) -> a view of Cv channels whose halo pixels and pad channels hold `fill`"""
    B, H, W, Cr = x.shape
    full = torch.full((B, H + 2 * halo, W + 2 * halo, Cv), fill, dtype=torch.float32)
    full[:, halo:halo + H, halo:halo + W, :Cr] = x
    return View(full.to(TDT[dtype]).reshape(-1).to(device), B, H, W, Cv, halo, dtype)


_REF = {}


def reference(shape):
    """f, r (B,H,W,Cr) fp32 holding bf16-representable values, with planted elements (f == r; f == 0 exactly with r on either side; f == r == 0),
    and the float64 sum: computed once per shape, shared, never modified"""
    if shape not in _REF:
        B, H, W, Cv, Cr, *_ = shape
        g = torch.Generator().manual_seed(7 + 13 * H + 5 * Cr + B)
        f = torch.randn(B, H, W, Cr, generator=g).bfloat16().float()
        r = torch.randn(B, H, W, Cr, generator=g).bfloat16().float()
        ff, rf = f.view(-1), r.view(-1)
        n = ff.numel()
        idx = torch.randperm(n, generator=g)
        k = max(1, n // 16)
        rf[idx[:k]] = ff[idx[:k]]                              # f == r: gradient 0
        ff[idx[k:2 * k]] = 0.0                                 # f == 0 exactly: factor 0.2 under LRELU, r random on either side
        if n >= 4:
            ff[idx[2 * k]] = 0.0
            rf[idx[2 * k]] = 0.0                               # both zero
        _REF[shape] = dict(f=f, r=r, S=float((f.double() - r.double()).abs().sum()), n=n)
    return _REF[shape]


def _pattern(B, H, W, Cr, unit):
    b, h, w, c = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), torch.arange(Cr), indexing="ij")
    return (((b * 5 + h * 7 + w * 3 + c * 2) % 5) - 2).float() * unit


def _ws(ops, fv, device):
    return torch.zeros(ops.featmatch_ws_floats(fv), dtype=torch.float32, device=device)


def body_family(ops, device, shape, dtype):
    """one shape of the issue's table: loss against float64 within the header's bound (and really accumulated), gradient bit-identical to the
    header's fp32 statement for accumulate 0 / 1 x act NONE / LRELU, halos and pad channels of g untouched, NaN in the halos and pad channels
    of f and r without effect, g = NULL, repeated bits"""
    B, H, W, Cv, Cr, hf, hr, hg = shape
    ref = reference(shape)
    f, r, n = ref["f"], ref["r"], ref["n"]
    label = f"{SHAPE_ID(shape)} {NAME[dtype]}"
    L = R.chain(B, H, W, Cr, dtype == F32)
    term = LOSS_SCALE * ref["S"] / n
    assert int((f == r).sum()) >= 1 and int((f == 0).sum()) >= 1, "the planted elements are missing"
    # the same data twice: halos and pad channels full of NaN (they must never be read), and holding 0.25
    views = [(make_view(f, Cv, dtype, hf, device, fill), make_view(r, Cv + (8 if Cr < Cv else 0), dtype, hr, device, fill)) for fill in (float("nan"), 0.25)]
    fv, rv = views[0]
    ws = _ws(ops, fv, device)
    # ---- loss: two calls onto a prefilled slot, no gradient view
    slot = torch.full((4,), SENT, dtype=torch.float32, device=device)
    slot[1] = PREFILL
    op = ops.featmatch(fv, rv, Cr, LOSS_SCALE, slot[1:2], GRAD_SCALE, ACT_NONE, None, 0, ws)
    got = []
    for _ in range(2):
        op()
        sync(device)
        got.append(float(slot[1]))
    assert float(slot[0]) == SENT and float(slot[2]) == SENT, f"{label}: a write beside the slot"
    for k, v in enumerate(got):
        want = PREFILL + (k + 1) * term
        err, tol = abs(v - want), (k + 1) * R.loss_bound(L, term, v)
        MEASURED.append((f"{label} call {k + 1}", err, tol))
        print(f"[featmatch] {label} call {k + 1}: slot {v:.9g} statement {want:.9g} error {err:.3g} (allowed {tol:.3g}, chain {L})")
        assert err <= tol, f"{label}: loss error {err:.3g} outside the header's bound {tol:.3g}"
    assert got[1] > got[0] > PREFILL or ref["S"] == 0
    # ---- gradient: bit for bit the header's statement
    inv = float(np.float32(GRAD_SCALE) / np.float32(n))
    unit = 2.0 ** math.floor(math.log2(inv))
    pat = _pattern(B, H, W, Cr, unit).to(TDT[dtype]).float()
    for act in (ACT_NONE, ACT_LRELU):
        for acc in (0, 1):
            outs = []
            for vi, (fv_, rv_) in enumerate(views):
                gv = make_view(pat, Cv, dtype, hg, device, SENT)
                before = gv.padded().clone()
                slot2 = torch.full((1,), PREFILL, dtype=torch.float32, device=device)
                op = ops.featmatch(fv_, rv_, Cr, LOSS_SCALE, slot2, GRAD_SCALE, act, gv, acc, ws)
                op()
                sync(device)
                want = R.grad32(f, r, GRAD_SCALE, act, pat if acc else None).to(TDT[dtype])
                assert same_bits(gv.nhwc()[..., :Cr].cpu(), want), f"{label} act={act} accumulate={acc}: the gradient differs from the header's fp32 statement"
                after = gv.padded().clone()
                keep = torch.ones(after.shape, dtype=torch.bool)
                keep[:, hg:hg + H, hg:hg + W, :Cr] = False
                assert same_bits(after.cpu()[keep], before.cpu()[keep]), f"{label}: a halo or pad channel of g was written"
                assert float(slot2) == got[0], f"{label}: the loss with a gradient view differs from the loss without"
                outs.append((after.cpu(), float(slot2)))
                if acc == 0 and vi == 0:      # determinism: the same launch into the same content repeats its bits
                    op()
                    sync(device)
                    assert same_bits(gv.padded().cpu(), after.cpu()), f"{label}: a repeated call differs"
            assert same_bits(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1], f"{label}: NaN in halos / pad channels of f, r changed a result"
            if acc:
                assert int((want.float() != pat).sum()) > 0, "accumulate = 1 changed nothing: the case shows nothing"


def body_nan_element(ops, device, dtype=BF16):
    """one NaN element (in f, then in r) poisons the loss and no other element's gradient"""
    shape = SHAPES[2]
    B, H, W, Cv, Cr, hf, hr, hg = shape
    ref = reference(shape)
    clean = None
    for which in (None, "f", "r"):
        f, r = ref["f"].clone(), ref["r"].clone()
        if which is not None:
            (f if which == "f" else r)[1, 17, 5, 9] = float("nan")
        fv, rv = make_view(f, Cv, dtype, hf, device, 0.0), make_view(r, Cv, dtype, hr, device, 0.0)
        gv = make_view(torch.zeros(B, H, W, Cr), Cv, dtype, hg, device, 0.0)
        slot = torch.zeros(1, dtype=torch.float32, device=device)
        ops.featmatch(fv, rv, Cr, 1.0, slot, 1.0, ACT_LRELU, gv, 0, _ws(ops, fv, device))()
        sync(device)
        g = gv.nhwc().cpu().clone()
        if which is None:
            clean = g
            assert math.isfinite(float(slot))
            continue
        assert math.isnan(float(slot)), which
        g[1, 17, 5, 9], c2 = 0, clean.clone()
        c2[1, 17, 5, 9] = 0
        assert same_bits(g, c2), f"NaN in {which}: another element's gradient changed"


def body_refusals(ops, device):
    """mismatched geometry, dtype, C or act: the project's error, and nothing is written"""
    v = lambda B=2, H=4, W=4, Cv=8, dt=F32, halo=1: make_view(torch.zeros(B, H, W, min(Cv, 8)), Cv, dt, halo, device, 0.0)
    f = v()
    ws = torch.zeros(64, dtype=torch.float32, device=device)
    slot = torch.full((1,), SENT, dtype=torch.float32, device=device)
    bad = [dict(r=v(B=1)), dict(r=v(H=3)), dict(r=v(W=5)), dict(r=v(dt=BF16)), dict(g=v(B=1)), dict(g=v(H=5)), dict(g=v(dt=BF16)), dict(Cr=0), dict(Cr=9),
           dict(Cr=16, g=v(Cv=8), r=v(Cv=16), f=v(Cv=16)), dict(act=1), dict(act=3)]
    for kw in bad:
        a = dict(f=f, r=v(), Cr=8, g=v(halo=2), act=ACT_LRELU)
        a.update(kw)
        with pytest.raises(GanError):
            ops.featmatch(a["f"], a["r"], a["Cr"], 1.0, slot, 1.0, a["act"], a["g"], 1, ws)()
        sync(device)
        assert float(slot) == SENT, kw
    ops.featmatch(f, v(halo=0), 8, 1.0, slot, 1.0, ACT_NONE, v(halo=2), 1, ws)()      # the matching call passes
    sync(device)
    assert float(slot) == SENT


# ------------------------------------------------------------------------------------------------ the engine (nets.DPass / DFamilyPass)
S, B, W_FM = 32, 2, 10.0


def size_for(K):
    """32 x 32 for one scale; a second scale needs 64 x 64: at 32 x 32 its input is 16 x 16 and its two stride-1 convolutions leave no logit"""
    return S if K == 1 else 64


def config(w=W_FM, nce=True, warmup=None, K=1, sn=False, aug=False, key=True):
    cfg = cases.small_config()
    if K > 1:                         # at 64 x 64 a narrow, shallow generator keeps the case quick (tests/test_dfamily_cpu.py does the same)
        cfg["model"]["generator"]["ngf"], cfg["model"]["generator"]["n_blocks"] = 16, 3
    cfg["diffaugment"]["enable"] = aug
    cfg["model"]["discriminator"].update(num_scales=K, use_spectral_norm=sn)
    if key:
        cfg["loss_weights"]["featmatch"] = w
    else:
        cfg["loss_weights"].pop("featmatch", None)
    if not nce:
        cfg["loss_weights"]["patchnce"] = 0.0
    if warmup is not None:
        cfg["warmup_steps"] = warmup
    return cfg


def trainer(ops, device, cfg, batch_size=B, **kw):
    torch.set_num_threads(4)
    C.set_seed(42)
    gen, disc = C.build_models(cfg, "cpu")
    return C.CutTrainer(gen, disc, cfg, batch_size, size_for(cfg["model"]["discriminator"]["num_scales"]), device=device, amp=False, ops=ops, **kw)


def batch(device, size=S, seed=1234, n=B):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 3, size, size, generator=g) * 2 - 1).to(device), (torch.rand(n, 3, size, size, generator=g) * 2 - 1).to(device)


def step(tr, k, device, photos=None):
    """one step with the draws of seed 9000 + k -> (loss dict, the draws)"""
    torch.manual_seed(9000 + k)
    rnd = tr.sample_randomness()
    p, monets = batch(device, tr.S)
    out = tr.train_step(k, p if photos is None else photos, monets, rnd)
    sync(device)
    return out, rnd


def _names(prog):
    return [getattr(op, "__name__", type(op).__name__) for op in prog.ops]


def body_engine(make_ops, device):
    """defaults build the launches the engine always built; spectral=False drops the power iteration and the pack and nothing else; a hook
    sits right behind the input gradient that wrote its view and in front of every launch that reads it"""
    ops = make_ops()
    convs, alive = {}, []

    def wrap(layer):              # the discriminator's launches come from the forked op layer (its own stream) where there is one
        inner = layer.conv_igemm

        def conv_igemm(c):
            op = inner(c)
            convs[id(op)] = c
            alive.append(op)      # a discarded program's launches must not hand their ids on to later ones
            return op
        layer.conv_igemm = conv_igemm
    for layer in {id(o): o for o in (ops, ops.fork())}.values():
        wrap(layer)
    tr = trainer(ops, device, config(w=0.0, K=2, sn=True))
    fam = tr.d_fake
    gls = fam.grad_logits_views()
    L = tr.D.nconv - 1
    base = fam.bwd_program(gls, wgrad=False, need_input_grad=True)
    assert _names(base) == _names(fam.bwd_program(gls, wgrad=False, need_input_grad=True, hooks=None))
    assert _names(base) == _names(fam.bwd_program(gls, wgrad=False, need_input_grad=True, hooks=[{}, {}]))
    assert _names(base) == [n for n in _names(tr.prog_g_adversarial) if n in set(_names(base))][-len(base):], "the trainer's own program differs"
    dp = fam.dps[0]
    assert _names(dp.bwd_program(gls[0], wgrad=True)) == _names(dp.bwd_program(gls[0], wgrad=True, hooks=None)) == _names(dp.bwd_program(gls[0], wgrad=True, hooks={}))
    full, scales = fam.fwd_program(), fam.fwd_program(spectral=False)
    assert _names(full) == _names(fam.fwd_program(spectral=True)) and len(full) == len(scales) + 2
    assert _names(full)[2:] == _names(scales) and all(a is b or _names(Program_of(a)) == _names(Program_of(b)) for a, b in zip(full.ops[2:], scales.ops))
    plain = trainer(make_ops(), device, config(w=0.0, K=2, sn=False)).d_fake
    assert _names(plain.fwd_program()) == _names(plain.fwd_program(spectral=False)), "without spectral norm the switch changes nothing"
    # ---- hooks: every feature layer of every scale
    seen = []

    def mk(s, j):
        def hook(gv):
            def marker():
                pass
            marker.__name__ = f"marker{s}.{j}"
            seen.append((s, j, gv, marker))
            return [marker]
        return hook
    prog = fam.bwd_program(gls, wgrad=True, need_input_grad=True, hooks=[{j: mk(s, j) for j in range(L)} for s in range(2)])
    assert len(seen) == 2 * L and len(prog) == len(fam.bwd_program(gls, wgrad=True, need_input_grad=True)) + 2 * L
    for s, j, gv, marker in seen:
        a = fam.dps[s].acts[j]
        assert (gv.B, gv.H, gv.W, gv.C, gv.dtype) == (a.B, a.H, a.W, a.C, a.dtype) and gv.halo in (1, 2)
        p = prog.ops.index(marker)
        writers = [i for i, op in enumerate(prog.ops) if id(op) in convs and convs[id(op)].out.t.data_ptr() == gv.t.data_ptr()]
        readers = [i for i, op in enumerate(prog.ops) if id(op) in convs and convs[id(op)].x.t.data_ptr() == gv.t.data_ptr()]
        between = [i for i in writers if i < p]
        assert between and between[-1] == p - 1, f"scale {s} layer {j}: the hook does not follow the launch that wrote its view"
        assert readers and min(readers) > p and not [i for i in writers if p < i < min(readers)], f"scale {s} layer {j}: a launch reads the view in front of the hook"
    with pytest.raises(AssertionError):
        fam.dps[0].bwd_program(gls[0], hooks={L: mk(0, L)})          # the logits are no feature


def Program_of(op):
    from gan_variant_research_amd.runtime import Program
    p = Program()
    p.add(op)
    return p


# ------------------------------------------------------------------------------------------------ the fused trainer
def recording(ops, log):
    """wraps the featmatch constructor (an instance attribute, as a trainer calls it) of the op layer and of its fork -- the discriminator's
    stream, where the trainer queues the term -- and records its arguments"""
    def wrap(layer):
        inner = layer.featmatch

        def featmatch(f, r, Cr, loss_scale, loss, grad_scale, act, g, accumulate, ws):
            log.append(dict(f=f, r=r, Cr=Cr, loss_scale=loss_scale, loss=loss, grad_scale=grad_scale, act=act, g=g, accumulate=accumulate))
            return inner(f, r, Cr, loss_scale, loss, grad_scale, act, g, accumulate, ws)
        layer.featmatch = featmatch
    for layer in {id(o): o for o in (ops, ops.fork())}.values():
        wrap(layer)
    return ops


def own_statement(tr):
    """the float64 statement on the trainer's OWN activation buffers -> (fm, the kernel's accumulated bound)"""
    K, L = tr.num_scales, tr.D.nconv - 1
    terms = []
    for s in range(K):
        for j in range(L):
            f, r, Cr = tr.d_fake.dps[s].acts[j], tr.d_fm.dps[s].acts[j], tr.D.nets[s].chans[j + 1]
            terms.append((float(R.layer_loss(f.nhwc()[..., :Cr].cpu(), r.nhwc()[..., :Cr].cpu())) / (K * L), R.chain(f.B, f.H, f.W, Cr, f.dtype == F32)))
    fm = sum(t for t, _ in terms)
    return fm, sum(R.loss_bound(Lc, t, fm) for t, Lc in terms)


def d_state(tr):
    """the discriminator's parameters and spectral-norm buffers as float64 CPU tensors"""
    return ({k: v.detach().cpu().double() for k, v in tr.opt_D.params.items()}, {k: v.detach().cpu().double() for k, v in tr.d_buffers.items()})


def end_to_end(tr, fake, photos, rnd, g_params=None):
    """fm in float64 with torch: aug(fake) and aug(photos) under the generator step's draws through the restated discriminator with the
    trainer's current parameters; g_params: the generator's (float64) to derive fake from the photos through oracle.cut_ref instead"""
    from oracle import cut_ref
    params, bufs = d_state(tr)
    photos = photos.detach().cpu().double()
    if g_params is not None:
        fake = cut_ref.generator_forward(g_params, photos, tr.generator.n_blocks)
    aug = (lambda x: cut_ref.diffaugment(x, rnd["aug_fake_g"])) if tr.aug is not None else (lambda x: x)
    feats = lambda x: R.features(aug(x), params, tr.num_scales, tr.discriminator.n_layers, bufs)
    return R.fm(feats(fake.double()), feats(photos))


def body_trainer_term(make_ops, device, merged=True, nce=True, K=1, sn=False, aug=False):
    """(a) - (d) of the issue in one shape of the step"""
    log = []
    cfg = config(nce=nce, warmup=None if merged else 1, K=K, sn=sn, aug=aug)
    tr = trainer(recording(make_ops(), log), device, cfg)
    out = rnd = None
    for k in range(1 if merged else 2):
        out, rnd = step(tr, k, device)
    assert tr.mode_merged == merged and bool(tr.nce_layers) == nce and tr.featmatch and "featmatch" in out
    label = f"trainer merged={merged} nce={nce} K={K} sn={sn} aug={aug}"
    L = tr.D.nconv - 1
    # (a) the kernel on the trainer's own buffers
    own, tol = own_statement(tr)
    print(f"[featmatch] {label}: featmatch {out['featmatch']:.9g} own buffers {own:.9g} error {abs(out['featmatch'] - own):.3g} (allowed {tol:.3g})")
    assert own > 0 and abs(out["featmatch"] - own) <= tol
    # (b) end to end in float64
    photos, _ = batch(device, tr.S)
    e2e = float(end_to_end(tr, tr.generated().detach().cpu(), photos, rnd))
    print(f"[featmatch] {label}: end to end float64 {e2e:.9g} relative error {abs(out['featmatch'] - e2e) / e2e:.3g} (allowed 1e-3)")
    assert abs(out["featmatch"] - e2e) <= 1e-3 * e2e
    # (c) g_loss
    lw = cfg["loss_weights"]
    old = lw["adv"] * out["g_adv"] + lw["patchnce"] * out["nce"] + out["identity_weight"] * out["identity"]
    assert abs(out["g_loss"] - (old + W_FM * out["featmatch"])) <= 1e-6 * max(1.0, abs(out["g_loss"]))
    # (d) the launches of the current passes
    i = tr._featmatch_slot_index()
    assert i == tr._palette_slot_index() and tr.losses.numel() >= i + 1
    for s in range(K):
        for j in range(L):
            f, r = tr.d_fake.dps[s].acts[j], tr.d_fm.dps[s].acts[j]
            calls = [c for c in log if c["f"] is f and c["r"] is r]
            assert calls, f"{label}: no launch on scale {s} layer {j}"
            c = calls[-1]
            assert (c["Cr"], c["act"], bool(c["accumulate"])) == (tr.D.nets[s].chans[j + 1], ACT_LRELU, True)
            assert c["loss_scale"] == 1.0 / (K * L) and c["grad_scale"] == W_FM / (K * L)
            assert c["loss"].data_ptr() == tr.losses[i:i + 1].data_ptr()
            g = c["g"]
            assert (g.B, g.H, g.W, g.C, g.dtype) == (f.B, f.H, f.W, f.C, f.dtype) and g.halo in (1, 2)
    assert len(log) % (K * L) == 0 and _names(tr.prog_g_adversarial).count("gan_featmatch") == K * L
    return tr


def flat_g_after_step(make_ops, device, w):
    cfg = config(w=w) if w > 0 else config(key=False)
    tr = trainer(make_ops(), device, cfg)
    g_params = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in tr.opt_G.params.items()}
    _, rnd = step(tr, 0, device)
    return tr, tr.opt_G.flat_g.detach().cpu().double().clone(), g_params, rnd


def body_gradient(make_ops, device):
    """trainers with weights 0, w, 2w from one seed (merged shape, step 0): flat_g is affine in w, and flat_g(w) - flat_g(0) is w times the
    float64 autograd gradient of fm through the restated generator and discriminator"""
    (_, g0, _, _), (tr, g1, gp, rnd), (_, g2, _, _) = (flat_g_after_step(make_ops, device, w) for w in (0.0, W_FM, 2 * W_FM))
    d1, d2 = g1 - g0, g2 - g0
    # palette_cases.body_linearity's allowance: its loss-kernel term, plus the fp32 noise of three gradient blocks whose longest dot product
    # has 9 x 256 terms (tests/cases.py: BOUND_C sqrt(K) u), relative to the difference's norm
    rel = (4 * PC.FLOOR * 100.0) / 10.0 + cases.BOUND_C * math.sqrt(9 * 256) * cases.U_F32 * float(g0.norm() + 2 * g1.norm() + g2.norm()) / float(d2.norm())
    err = float((d2 - 2 * d1).norm() / d2.norm())
    print(f"[featmatch] linearity: |d(2w) - 2 d(w)| / |d(2w)| = {err:.3g} (allowed {rel:.3g}); |d(w)| / |g(0)| = {float(d1.norm() / g0.norm()):.3g}")
    assert float(d1.norm()) > 1e-6 * float(g0.norm()), "the featmatch weight does not reach the generator's gradient"
    assert err <= rel
    photos, _ = batch("cpu")
    fm = end_to_end(tr, None, photos, rnd, g_params=gp)
    grads = torch.autograd.grad(fm, [gp[k] for k in tr.opt_G.names])
    want = torch.zeros_like(g1)
    for k, g, o, n in zip(tr.opt_G.names, grads, tr.opt_G.offsets, tr.opt_G.sizes):
        want[int(o):int(o) + n] = W_FM * g.reshape(-1)
    err = float((d1 - want).norm() / want.norm())
    print(f"[featmatch] gradient: |flat_g(w) - flat_g(0) - w d fm / d theta| / |w d fm / d theta| = {err:.3g} (allowed {rel:.3g})")
    assert float(want.norm()) > 0 and err <= rel


def body_one_power_iteration(make_ops, device):
    """spectral norm: weight_u after a step is bit for bit the same with the key 0 and with it > 0"""
    us = []
    for w in (0.0, W_FM):
        tr = trainer(make_ops(), device, config(w=w, K=2, sn=True))
        step(tr, 0, device)
        us.append({k: v.detach().cpu().clone() for k, v in tr.d_buffers.items() if k.endswith("weight_u")})
    assert us[0] and all(same_bits(us[0][k], us[1][k]) for k in us[0]), "the real branch ran a power iteration of its own"


def body_nan_stop(make_ops, device):
    """a NaN planted in the photos raises the NaN stop; so does a NaN in the term's slot alone"""
    tr = trainer(make_ops(), device, config())
    photos, _ = batch(device)
    photos = photos.clone()
    photos[1, 2, 3, 4] = float("nan")
    with pytest.raises(ValueError, match="NaN loss"):
        step(tr, 0, device, photos=photos)
    v = [0.0] * tr.losses.numel()
    v[tr._featmatch_slot_index()] = float("nan")
    with pytest.raises(ValueError, match="NaN loss"):
        tr._loss_dict(v, (0, 0.1, False))
    assert "featmatch" in tr._loss_dict([0.0] * tr.losses.numel(), (0, 0.1, False))


def body_with_palette(make_ops, device):
    """both optional terms on: the palette's slot stays where it was, feature matching sits behind it"""
    cfg = config()
    cfg["loss_weights"]["palette"] = 0.5
    cfg["palette_prior"] = {"low_freq_size": 8, "use_ema": True, "ema_decay": 0.99}
    tr = trainer(make_ops(), device, cfg)
    assert tr._featmatch_slot_index() == tr._palette_slot_index() + 1
    out, _ = step(tr, 0, device)
    own, tol = own_statement(tr)
    assert abs(out["featmatch"] - own) <= tol and out["palette"] > 0
    lw = cfg["loss_weights"]
    old = lw["adv"] * out["g_adv"] + lw["patchnce"] * out["nce"] + out["identity_weight"] * out["identity"]
    assert abs(out["g_loss"] - (old + 0.5 * out["palette"] + W_FM * out["featmatch"])) <= 1e-6 * max(1.0, abs(out["g_loss"]))


# ------------------------------------------------------------------------------------------------ the module API
GOLDEN_CASES = {"ms2": ("ms2", "ms2", "x64", 2, False, False), "sn1-eval": ("sn1", "sn1.eval", "x", 1, True, False),
                "sn1-train": ("sn1", "sn1.train", "x", 1, True, True)}          # state dict, feature tag, input, scales, spectral norm, train mode
NDF, N_LAYERS = 8, 3


def golden_discriminator(g, name, device):
    sd_tag, ftag, xkey, K, sn, train = GOLDEN_CASES[name]
    D = C.MultiscaleDiscriminator(3, NDF, N_LAYERS, K, sn)
    sd = {k[len(sd_tag) + 4:]: torch.tensor(v) for k, v in g.items() if k.startswith(sd_tag + ".sd.")}
    D.load_state_dict(sd)
    D = D.to(device)
    D.train(train)
    return D, sd, torch.tensor(g[xkey]), ftag, K, sn, train


def body_module_features(device, g, name):
    """get_intermediate_features against the reference's recorded tensors (nesting, shapes, values within the 1e-3 parity margin), and its
    gradients with respect to x and the parameters against float64 autograd through the restatement, for a random cotangent on every feature"""
    D, sd, x, ftag, K, sn, train = golden_discriminator(g, name, device)
    xg = x.to(device).requires_grad_(True)
    feats = D.get_intermediate_features(xg)
    assert isinstance(feats, list) and len(feats) == K and all(isinstance(f, list) and len(f) == N_LAYERS + 1 for f in feats)
    gen = torch.Generator().manual_seed(5)
    cots, total = [], 0.0
    for sc in range(K):
        for j in range(N_LAYERS + 1):
            want = torch.tensor(g[f"{ftag}.feat.{sc}.{j}"])
            got = feats[sc][j]
            assert got.shape == want.shape and got.dtype == torch.float32, (name, sc, j, got.shape, want.shape)
            err = float((got.detach().cpu() - want).abs().max())
            assert err <= 1e-3 * float(want.abs().max()), (name, sc, j, err)
            cot = torch.randn(want.shape, generator=gen)
            cots.append(cot)
            total = total + (got * cot.to(device)).sum()
    names = [k for k, _ in D.named_parameters()]
    grads = torch.autograd.grad(total, [xg] + list(D.parameters()))
    # float64 autograd through the restatement, from the state dict as stored (train mode: one power iteration from the stored u, v)
    x64 = x.double().requires_grad_(True)
    p64 = {k: sd[k].double().requires_grad_(True) for k in names}
    b64 = {k: v.double() for k, v in sd.items() if k not in p64}
    f64 = R.features(x64, p64, K, N_LAYERS, b64, power_iteration=train)
    tot64 = sum((t * c.double()).sum() for t, c in zip([t for fs in f64 for t in fs], cots))
    want = torch.autograd.grad(tot64, [x64] + [p64[k] for k in names], allow_unused=True)
    for k, got, w in zip(["x"] + names, grads, want):
        w = torch.zeros_like(got.cpu().double()) if w is None else w          # the logits' convolution takes no gradient from the features
        scale = float(w.norm())
        err = float((got.cpu().double() - w).norm())
        assert err <= 1e-3 * scale + 1e-12, (name, k, err, scale)
    assert float(want[0].norm()) > 0
    return D


def body_feature_matching_loss(device):
    """losses.feature_matching_loss: nested and flat lists, the float64 statement within the kernel's bound, the header's fp32 gradient with
    respect to the fake features only"""
    from gan_variant_research_amd import losses as L
    gen = torch.Generator().manual_seed(11)
    shapes = [[(2, 8, 16, 16), (2, 12, 5, 7)], [(2, 8, 8, 8), (2, 3, 3, 3)]]
    real = [[torch.randn(sh, generator=gen).bfloat16().float() for sh in grp] for grp in shapes]
    fake = [[torch.randn(sh, generator=gen).bfloat16().float() for sh in grp] for grp in shapes]
    fake[0][0].view(-1)[:40] = real[0][0].view(-1)[:40]                                   # sign(0) = 0
    fd = [[t.clone().to(device).requires_grad_(True) for t in grp] for grp in fake]
    rd = [[t.clone().to(device).requires_grad_(True) for t in grp] for grp in real]
    loss = L.feature_matching_loss(rd, fd)
    want = float(R.fm([[t.double() for t in grp] for grp in fake], [[t.double() for t in grp] for grp in real]))
    tol = sum(R.loss_bound(R.chain(t.shape[0], t.shape[2], t.shape[3], t.shape[1], True), float(R.layer_loss(t, r)), float(R.layer_loss(t, r))) / (2 * len(grp))
              for grp, rg in zip(fake, real) for t, r in zip(grp, rg)) + 8 * R.U * want       # + the fp32 sums and quotients of the python side
    assert abs(float(loss.detach()) - want) <= tol, (float(loss.detach()), want, tol)
    flat = L.feature_matching_loss(rd[0], fd[0])
    assert abs(float(flat.detach()) - float(R.fm([fake[0]], [real[0]]))) <= tol
    loss.backward()
    assert all(t.grad is None for grp in rd for t in grp), "a gradient reached the real features"
    for gi, grp in enumerate(fake):
        for t, r, d in zip(grp, real[gi], fd[gi]):
            # header: v = +-inv, inv = 1 / (float)n; then the python side's chain rule in fp32: / layers, / scales
            inv = R.grad32(t.permute(0, 2, 3, 1).contiguous(), r.permute(0, 2, 3, 1).contiguous(), 1.0, ACT_NONE).permute(0, 3, 1, 2)
            assert d.grad is not None and float((d.grad.cpu() - inv / len(grp) / len(fake)).abs().max()) <= 4 * R.U * float(inv.abs().max())
            assert bool(((d.grad.cpu() == 0) == (t == r)).all())


def body_module_step(device):
    """module_step.train_step: the dict has `featmatch` only when the weight is > 0, g_loss gains w * featmatch, and the value is the float64
    statement on the step's own G(photos) under the injected draws"""
    from gan_variant_research_amd import losses as L
    from gan_variant_research_amd import module_step as MS
    from gan_variant_research_amd import training as TR
    torch.set_num_threads(4)
    outs = {}
    for w in (0.0, W_FM):
        cfg = config(w=w, aug=True)
        cfg["model"]["generator"].update(ngf=8, n_blocks=1)
        cfg["model"]["discriminator"].update(ndf=8, n_layers=2)
        cfg["patchnce"]["nce_layers"] = [0, 2]
        C.set_seed(42)
        gen, disc = C.build_models(cfg, "cpu")
        gen, disc = gen.to(device), disc.to(device)
        opt_G, opt_D = TR.get_optimizer(gen, cfg["optim"]["G"]), TR.get_optimizer(disc, cfg["optim"]["D"])
        photos, monets = batch(device)
        torch.manual_seed(7)
        outs[w] = MS.train_step(0, photos, monets, gen, disc, opt_G, opt_D, None, TR.AMPContext(False), L.DiffAugment(cfg["diffaugment"]["policy"]), cfg,
                                torch.device(device))
    assert "featmatch" not in outs[0.0] and outs[W_FM]["featmatch"] > 0
    o = outs[W_FM]
    lw = config()["loss_weights"]
    old = lw["adv"] * o["g_adv"] + lw["patchnce"] * o["nce"] + o["identity_weight"] * o["identity"]
    assert abs(o["g_loss"] - (old + W_FM * o["featmatch"])) <= 1e-5 * max(1.0, abs(o["g_loss"]))
    for k in ("d_loss", "g_adv", "nce", "identity", "r1"):          # the term changes nothing else of the step's forward values
        assert abs(outs[0.0][k] - o[k]) <= 1e-6 * max(1.0, abs(o[k])), k
