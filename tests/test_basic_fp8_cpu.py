"""fp8 mode of the fused CycleGAN trainer (basic.CycleGANTrainer(fp8=..., fp8_wgrad=...)) on the CPU emulator: the switches, that the trainer
plans exactly the parent's launches with them off, what it plans with them on, the event order that protects the e4m3 gradient buffers,
the planner's answer under the power-of-two promise, the power-of-two quantiser's statement, and one emulated iteration."""
import json
import os

import pytest
import torch

from gan_variant_research_amd import FP8
from gan_variant_research_amd import basic as BG
from gan_variant_research_amd.runtime import WgradCall
from tests import cases
from tests import emulator_basic_fp8 as E
from tests.emulator import EmuOps
from tests.emulator_basic_fp8 import BasicFp8EmuOps
from tests.emulator_fp8wgrad import Fp8WgradEmuOps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "basic_fp8_parent_launches.json")


# ---------------------------------------------------------------------------------------------------------------------- switches
def test_trainer_builds_with_fp8_and_fp8_wgrad():
    """CycleGANTrainer(..., fp8=True, fp8_wgrad=True) exists (before the feature: TypeError, unknown keyword) and hands the switches, and
    the power-of-two gradient scales, to both generator engines."""
    tr = E.make_trainer("cpu", BasicFp8EmuOps(), 64, 2, True, True, True)
    assert tr.fp8 and tr.fp8_wgrad
    for net in (tr.Gab, tr.Gba):
        assert net.fp8 and net.fp8_wgrad and net.fp8_pow2_scales


def _trainer_from_cfg(cfg, **kw):
    torch.manual_seed(0)
    mods = BG.build_models(cfg, "cpu")
    return BG.CycleGANTrainer(*mods, cfg, 2, 64, device="cpu", ops=BasicFp8EmuOps(), **kw)


def test_config_keys_reach_the_trainer():
    cfg = cases.basic_config()
    cfg["training"]["amp"] = True
    cfg["mi355x"] = {"fp8": True, "fp8_wgrad": True}
    tr = _trainer_from_cfg(cfg)
    assert tr.fp8 and tr.fp8_wgrad and tr.Gab.fp8_wgrad and tr.Gba.fp8_wgrad
    cfg["mi355x"] = {"fp8": True}
    tr = _trainer_from_cfg(cfg)
    assert tr.fp8 and not tr.fp8_wgrad and tr.Gab.fp8 and not tr.Gab.fp8_wgrad
    tr = _trainer_from_cfg(cfg, fp8=False)          # the keyword wins over the config
    assert not tr.fp8 and not tr.Gab.fp8
    del cfg["mi355x"]
    tr = _trainer_from_cfg(cfg)
    assert not tr.fp8 and not tr.fp8_wgrad and not tr.Gab.fp8 and not tr.Gab.fp8_pow2_scales


def test_the_two_value_errors():
    with pytest.raises(ValueError, match="fp8_wgrad needs fp8"):
        E.make_trainer("cpu", BasicFp8EmuOps(), 64, 2, True, False, True)
    with pytest.raises(ValueError, match=r"bf16 \(amp\) mode only"):
        E.make_trainer("cpu", BasicFp8EmuOps(), 64, 2, False, True, False)
    cfg = cases.basic_config()
    cfg["training"]["amp"] = True
    cfg["mi355x"] = {"fp8_wgrad": True}
    with pytest.raises(ValueError, match="fp8_wgrad needs fp8"):
        _trainer_from_cfg(cfg)
    cfg["training"]["amp"] = False
    cfg["mi355x"] = {"fp8": True}
    with pytest.raises(ValueError, match=r"bf16 \(amp\) mode only"):
        _trainer_from_cfg(cfg)


# ---------------------------------------------------------------------------------------------------------------------- switches off
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_switches_off_plan_the_parents_launches(mode):
    """With both switches off the trainer asks for exactly the launches, with exactly the arguments, of the commit before the switches
    existed.  The parent's sequence is tests/golden/basic_fp8_parent_launches.json: recorded ON that commit by
    tools/make_golden_basic_fp8.py (emulator_basic_fp8.build_programs on tests.emulator.EmuOps, 32x32, batch 2) -- it is not recomputed
    from the code under test."""
    want = json.load(open(GOLDEN))[mode]
    tr, log = E.build_programs(EmuOps(), 32, 2, amp=mode == "bf16")
    assert not tr.fp8 and not tr.fp8_wgrad
    got = log.hashed()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w, log.entries[i])


# ---------------------------------------------------------------------------------------------------------------------- switches on
def _is_residual(w):
    return w["ntaps"] == 9 and w["Cx"] == 256 and w["N"] == 256 and (w["x_sy"], w["g_sy"]) == (1, 1)


def _wgrads(log):
    return [(s, a[0][0][1]) for s, n, a in log.entries if n == "conv_wgrad"]


def _geometry(w):
    strip = lambda v: v[:7] if isinstance(v, list) and v and v[0] == "V" else v[:3] if isinstance(v, list) and v and v[0] == "T" else v
    return {k: strip(v) for k, v in w.items()}


def test_all_six_passes_take_the_e4m3_weight_gradient():
    """64x64, batch 2 (16x16 residual maps): in each of the six generator passes -- the second-generator passes built with
    need_input_grad=True and the first-generator passes with a second, folded gradient included -- every residual weight gradient is a
    dtype FP8, variant 1 launch on that pass's in8 / mid8 copy and an e4m3 gradient buffer, with the power-of-two promise; every other
    launch is the one the fp8 mode plans."""
    tr, log = E.build_programs(BasicFp8EmuOps(), 64, 2, True, True, True)
    tr_off, log_off = E.build_programs(BasicFp8EmuOps(), 64, 2, True, True, False)
    passes = E.generator_passes(tr)
    assert len(passes) == 6 and sorted(tr.Gab.passes + tr.Gba.passes, key=id) == sorted((p for _, p in passes), key=id)
    for name, p in passes:
        assert p.net is (tr.Gab if name.startswith("ab") else tr.Gba)
        assert p.wgrad8_layers == {(k, w): True for k in range(9) for w in "ab"}, name
        assert len(p.wgrad8_calls) == 18
        calls = iter(p.wgrad8_calls)
        for k in reversed(range(9)):
            cb, ca = next(calls), next(calls)
            for c, x8 in ((cb, p.mid8[k]), (ca, p.in8[k])):
                assert c.x is x8 and c.x.dtype == FP8 and c.g.dtype == FP8 and c.variant == 1 and c.g.halo == 2
                assert c.g_scale is not None and c.g_scale_pow2 is True
                assert c.nsplit == c.B * BasicFp8EmuOps().wgrad_patch_splits(c) == 2
            assert cb.g.t is not ca.g.t
        assert (p.g_input is not None) == (name in ("ba_fb", "ab_fa"))
    for _, p in E.generator_passes(tr_off):
        assert p.wgrad8_layers == {} and p.wgrad8_calls == []
    n8 = 6 * 18
    on, off = _wgrads(log), _wgrads(log_off)
    assert len(on) == len(off)
    fp8_on = [w for _, w in on if w["x"][6] == FP8]
    assert len(fp8_on) == n8 and all(_is_residual(w) and w["variant"] == 1 and w["g_scale_pow2"] is True for w in fp8_on)
    assert [s for s, w in on if w["x"][6] == FP8] == ["main.side"] * n8
    assert sum(_is_residual(w) for _, w in off) == n8 and not any(w["x"][6] == FP8 for _, w in off)
    assert [(s, _geometry(w)) for s, w in on if w["x"][6] != FP8] == [(s, _geometry(w)) for s, w in off if not _is_residual(w)]
    count = lambda lg: {n: sum(1 for _, m, _ in lg.entries if m == n) for n in set(m for _, m, _ in lg.entries)}
    assert count(log) == count(log_off)
    # the output gradients' copies come from the power-of-two quantiser (two per block and pass), the activations' copies do not
    assert count(log)["quantize_fp8_pow2"] == n8 and "quantize_fp8" not in count(log)
    # ... and, launch by launch and argument by argument, everything but the residual weight gradients is what fp8 mode plans
    got, want = _canonical(log), _canonical(log_off)
    assert len(got) == len(want) and len(got) == sum(1 for _, n, _ in log.entries if n not in ("record", "wait")) - n8
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)


def _canonical(log):
    """A LaunchLog with fp8 mode's and fp8 + fp8_wgrad's legitimate differences taken out, for an entry-by-entry comparison: per stream
    (the weight gradients' place on the main stream's timeline moves behind the quantiser, the order inside each stream does not), without
    the event operations and the residual weight-gradient launches themselves, buffer ordinals renumbered by first appearance, and the e4m3
    gradient copies (FP8 views with halo 2) and their per-image amax / scale vectors (fp32, one value per image) without an ordinal: fp8
    mode has one set of them per network and shape, fp8_wgrad four alternating ones."""
    ids = {}

    def canon(v):
        if isinstance(v, list) and v and v[0] == "V":
            return v[:7] + (["grad8"] if v[6] == FP8 and v[5] == 2 else [ids.setdefault(v[7], len(ids))])
        if isinstance(v, list) and v and v[0] == "T":
            return v[:3] + (["per-image"] if v[1] == 2 and v[2] == "torch.float32" else [ids.setdefault(v[3], len(ids))])
        if isinstance(v, list):
            return [canon(x) for x in v]
        if isinstance(v, dict):
            return {k: canon(x) for k, x in v.items()}
        return v
    out = []
    for stream in sorted({s for s, _, _ in log.entries}):
        for s, n, a in log.entries:
            if s != stream or n in ("record", "wait"):
                continue
            if n == "conv_wgrad" and _is_residual(a[0][0][1]):
                continue
            out.append((s, n, canon(a)))
    return out


@pytest.mark.parametrize("kind", ["second", "first_folded", "identity"])
def test_main_stream_waits_for_the_side_readers_before_it_rewrites_an_e4m3_gradient_buffer(kind):
    """The check of test_fp8_wgrad_cpu's test of the same name on the three kinds of backward program this trainer builds: a quantiser
    launch (main stream) into an e4m3 gradient buffer or its scales that an earlier side-stream weight gradient of the program read is
    preceded, after that reader, by a main-stream wait on the event the side stream recorded after the reader."""
    tr = E.make_trainer("cpu", BasicFp8EmuOps(), 64, 2, True, True, True)
    p = tr.Gab.new_pass(2, 64, 64)
    p.fwd_program(torch.zeros(2, 3, 64, 64))
    ops = tr.ops
    real_q = ops.quantize_fp8_pow2

    def quantize_fp8_pow2(src, dst, amax, scale_out):
        op = real_q(src, dst, amax, scale_out)
        op.writes = [dst.t, scale_out]
        return op
    ops.quantize_fp8_pow2 = quantize_fp8_pow2
    try:
        if kind == "second":
            prog = p.bwd_program(tr.ctx.view(2, 64, 64, 8, 0), accumulate=False, need_input_grad=True)
        elif kind == "first_folded":
            prog = p.bwd_program(tr.ctx.view(2, 64, 64, 8, 3), True, tr.ctx.view(2, 64, 64, 8, 0), accumulate=True)
        else:
            prog = p.bwd_program(tr.ctx.view(2, 64, 64, 8, 0), accumulate=True)
    finally:
        del ops.quantize_fp8_pow2
    assert all(p.wgrad8_layers.values()) and len(p.wgrad8_layers) == 18
    seq, checked = prog.ops, 0
    for i, op in enumerate(seq):
        for buf in getattr(op, "writes", []):
            assert getattr(op, "stream", "main") == "main"
            readers = [j for j in range(i) if getattr(seq[j], "stream", "main") == "side" and hasattr(seq[j], "wgrad")
                       and any(t is not None and t.data_ptr() == buf.data_ptr() for t in (seq[j].wgrad.g.t, seq[j].wgrad.g_scale))]
            if not readers:
                continue
            j = readers[-1]
            rec = next(k for k in range(j + 1, i) if getattr(seq[k], "stream", "main") == "side" and hasattr(seq[k], "ev_record"))
            assert all(getattr(seq[k], "stream", "main") != "side" or not hasattr(seq[k], "wgrad") for k in range(j + 1, rec))
            ev = seq[rec].ev_record
            assert any(getattr(seq[k], "stream", "main") == "main" and getattr(seq[k], "ev_wait", None) is ev for k in range(rec + 1, i)), \
                f"op {i} rewrites a buffer the side-stream launch {j} reads without waiting for it"
            checked += 1
    assert checked == 2 * (18 - 4)      # four buffer sets (a0 a1 b0 b1), copy and scales: all but each set's first use


# ---------------------------------------------------------------------------------------------------------------------- planner
def _planner_call(ctx, B, H, C_, dtype, pow2=None):
    x, g = ctx.view(B, H, H, C_, 1, dtype=dtype), ctx.view(B, H, H, C_, 2, dtype=dtype)
    tapoff = ctx.i32([(kh * x.Wp + kw) * C_ for kh in range(3) for kw in range(3)])
    return WgradCall(B, H, H, C_, 9, C_, 1, x, 0, 0, 1, 1, tapoff, g, 2, 2, 1, 1, None, max_tapoff=(2 * x.Wp + 2) * C_,
                     g_scale=ctx.f32(B, 1.0) if dtype == FP8 else None, g_scale_pow2=pow2)


PLANNER_GEOMS = [(64, 16, 256), (256, 16, 256), (48, 16, 256), (96, 16, 256), (512, 16, 128), (64, 16, 128), (2, 16, 256), (16, 64, 256),
                 (4, 128, 256), (64, 32, 256), (2, 8, 256)]


def test_planner_answer_with_the_promise_is_the_bf16_answer():
    """Emulator statements: for B in {64, 256, 48} at 16x16, C = 256, the e4m3 query with the promise answers what the bf16 query answers.
    That answer is negative (whole images per split) at B = 64 (-2) and B = 256 (-8), and without the promise the e4m3 query answers 0
    there.  B = 48 does not group: 48 * 8 blocks / 256 rounds down to one image per split, so all three queries answer 1 -- the grouping
    case with a batch that is no power of two is B = 96 (-3), checked beside it."""
    from gan_variant_research_amd import BF16
    from gan_variant_research_amd.runtime import Ctx
    ops = BasicFp8EmuOps()
    ctx = Ctx(ops, torch.device("cpu"), BF16)
    want = {64: -2, 256: -8, 48: 1, 96: -3}
    for B, w in want.items():
        bf = ops.wgrad_patch_splits(_planner_call(ctx, B, 16, 256, BF16))
        f8p = ops.wgrad_patch_splits(_planner_call(ctx, B, 16, 256, FP8, True))
        f8 = ops.wgrad_patch_splits(_planner_call(ctx, B, 16, 256, FP8))
        assert bf == f8p == w, (B, bf, f8p)
        assert f8 == (0 if w < 0 else w), (B, f8)
        assert f8 == Fp8WgradEmuOps().wgrad_patch_splits(_planner_call(ctx, B, 16, 256, FP8))       # no promise: the older statement


def test_planner_predicates_equal_their_emulator_statements():
    """gan_wgrad_patch_splits of the built library (a host-side predicate: no GPU needed) against BasicFp8EmuOps.wgrad_patch_splits for
    bf16 descriptors, e4m3 descriptors without the promise and e4m3 descriptors with it."""
    from gan_variant_research_amd import BF16
    from gan_variant_research_amd.runtime import Ctx, HipOps
    emu = BasicFp8EmuOps()
    ctx = Ctx(emu, torch.device("cpu"), BF16)
    hip = HipOps(torch.device("cpu"))
    seen = set()
    for B, H, C_ in PLANNER_GEOMS:
        for dtype, pow2 in ((BF16, None), (FP8, None), (FP8, True)):
            c = _planner_call(ctx, B, H, C_, dtype, pow2)
            got, want = hip.wgrad_patch_splits(c), emu.wgrad_patch_splits(c)
            assert got == want, (B, H, C_, dtype, pow2, got, want)
            seen.add((dtype, pow2, (want > 0) - (want < 0)))
    assert {(FP8, True, -1), (FP8, None, 0), (FP8, True, 1), (FP8, True, 0), (BF16, None, -1)} <= seen


def test_wgrad8_plans_whole_images_per_split_only_under_the_promise():
    """ConvLayer.wgrad8_call at B = 64, 16x16: with pow2=True nsplit = B // 2 and the flag is set; without it None (the bf16 kernel)."""
    from gan_variant_research_amd import BF16
    from gan_variant_research_amd.convplan import ConvLayer
    from gan_variant_research_amd.runtime import Ctx
    ctx = Ctx(BasicFp8EmuOps(), torch.device("cpu"), BF16)
    w = torch.zeros(256, 256, 3, 3)
    layer = ConvLayer(ctx, w, None, torch.zeros_like(w), None, 3, 1, 1)
    x8, g8 = ctx.view(64, 16, 16, 256, 1, dtype=FP8), ctx.view(64, 16, 16, 256, 2, dtype=FP8)
    sc = ctx.f32(64, 1.0)
    assert layer.wgrad8_call(x8, g8, sc) is None
    call = layer.wgrad8_call(x8, g8, sc, pow2=True)
    assert call is not None and call.nsplit == 32 and call.variant == 1 and call.g_scale_pow2 is True
    ops = layer.wgrad8(x8, g8, sc, False, pow2=True)
    assert ops[0].wgrad.nsplit == 32 and ops[0].wgrad.part.numel() >= 32 * 256 * 9 * 256


def test_the_benchmark_configuration_plans_in_fp8_mode():
    """BASELINE configs[1]: 64x64 at batch 256.  The e4m3 input gradient of a residual layer runs on the 18x18 padded domain; the library's
    gan_conv_patch_ok takes that GAN_FP8 descriptor at batch 256 as at batch 2 (there is no other e4m3 convolution, so the tile-utilisation
    rule that sends the bf16 launch to the generic kernel does not apply), as the emulator states; the same descriptor in bf16 is refused
    by both.  The weight gradient plans 8 images per split."""
    from gan_variant_research_amd import BF16
    from gan_variant_research_amd.convplan import ConvLayer
    from gan_variant_research_amd.runtime import Ctx, HipOps
    emu, hip = BasicFp8EmuOps(), HipOps(torch.device("cpu"))          # descriptors only: nothing is launched on `hip`
    convs = []
    conv_op = emu.conv_igemm
    emu.conv_igemm = lambda c: (convs.append(c), conv_op(c))[1]
    ctx = Ctx(emu, torch.device("cpu"), BF16)
    w = torch.zeros(256, 256, 3, 3)
    layer = ConvLayer(ctx, w, None, torch.zeros_like(w), None, 3, 1, 1)
    for B in (2, 64, 256):
        x8, y = ctx.view(B, 16, 16, 256, 1, dtype=FP8), ctx.view(B, 16, 16, 256, 0)
        dy8, dy, dx = ctx.view(B, 16, 16, 256, 2, dtype=FP8), ctx.view(B, 16, 16, 256, 2), ctx.view(B, 16, 16, 256, 1)
        sc = ctx.f32(B, 1.0)
        del convs[:]
        layer.fwd8(x8, y)
        layer.dgrad8(dy8, dx, sc, padded_domain=True)
        assert len(convs) == 2 and (convs[1].Ho, convs[1].Wo) == (18, 18) and convs[1].x.dtype == FP8
        for c in convs:
            assert hip.conv_patch_ok(c) and emu.conv_patch_ok(c), (B, c.Ho)
            assert hip.conv_patch_tile_rows(c) == 256
        del convs[:]
        layer.dgrad(dy, dx, padded_domain=True)
        assert bool(hip.conv_patch_ok(convs[0])) == bool(emu.conv_patch_ok(convs[0])) == (B <= 64)
    call = layer.wgrad8_call(x8, dy8, sc, pow2=True)
    assert call is not None and call.B == 256 and call.nsplit == 32


# ---------------------------------------------------------------------------------------------------------------------- quantiser
def test_pow2_quantiser_statement():
    """The STATEMENT of the power-of-two quantiser (tests/emulator_basic_fp8.py: test infrastructure, what the CPU suite plans and steps
    with), not the product: scale is a power of two with amax / 448 <= scale < 2 amax / 448; amax == 0 gives 1; the copy is
    e4m3(src / scale), its largest magnitude in (224, 448].  That csrc/fp8.hip equals this statement bit for bit is checked on the GPU
    (test_basic_fp8_gpu.test_pow2_quantiser_equals_its_emulator_statement)."""
    g = torch.Generator().manual_seed(3)
    amax = torch.cat([torch.tensor([448.0, 447.99, 448.01, 1.75, 1.7500001, 1.0, 7e-5, 3.0e4, 2.0 ** -20, 1.75 * 2.0 ** -30]),
                      torch.exp(torch.rand(200, generator=g) * 40 - 30)]).float()
    sc = E.pow2_scale(amax)
    m, _ = torch.frexp(sc)
    assert bool((m == 0.5).all())
    q = amax.double() / 448.0
    assert bool((q <= sc.double()).all()) and bool((sc.double() < 2 * q).all())
    assert float(E.pow2_scale(torch.tensor([448.0]))) == 1.0 and float(E.pow2_scale(torch.tensor([448.01]))) == 2.0
    assert float(E.pow2_scale(torch.tensor([1.75 * 2.0 ** -30]))) == 2.0 ** -38
    assert E.pow2_scale(torch.zeros(3)).tolist() == [1.0, 1.0, 1.0]
    assert float(E.pow2_scale(torch.tensor([1e-45]))) == 2.0 ** -126          # clamped: a normal float
    from gan_variant_research_amd import BF16
    from gan_variant_research_amd.runtime import Ctx
    ops = BasicFp8EmuOps()
    ctx = Ctx(ops, torch.device("cpu"), BF16)
    src, dst = ctx.view(3, 4, 4, 16, 2), ctx.view(3, 4, 4, 16, 2, dtype=FP8)
    v = torch.randn(3, 8, 8, 16, generator=g) * torch.tensor([1e-3, 5.0, 0.0]).view(3, 1, 1, 1)
    src.padded().copy_(v.bfloat16())
    am, so = src.padded().float().abs().amax((1, 2, 3)), ctx.f32(3)
    ops.quantize_fp8_pow2(src, dst, am, so)()
    assert torch.equal(so, E.pow2_scale(am)) and float(so[2]) == 1.0
    back = dst.padded().view(torch.float8_e4m3fn).float()
    top = back.abs().amax((1, 2, 3))
    assert bool((top[:2] > 224).all()) and bool((top[:2] <= 448).all()) and float(top[2]) == 0.0
    err = (back * so.view(3, 1, 1, 1) - src.padded().float()).abs().amax((1, 2, 3))
    assert bool((err[:2] <= am[:2] * 2.0 ** -3).all())


# ---------------------------------------------------------------------------------------------------------------------- iteration
def test_emulated_iteration_fp8_wgrad_vs_oracle():
    """One emulated iteration at 64x64, batch 2 with fp8 + fp8_wgrad against oracle.basic_ref.train_iteration: iteration-0 losses within
    8 %, every parameter within 2 lr + 5e-5 = 4.5e-4 after the update (the tolerances of test_cut_step_fp8_wgrad_vs_oracle); the residual
    weight gradients differ from the fp8-only run's by a relative Frobenius norm strictly between 0 and 0.2."""
    tr, got, _ = E.run_iteration_vs_oracle("cpu", BasicFp8EmuOps(), 64, 2, True, True, tol0=8e-2, ptol=4.5e-4, threads=8)
    assert tr.fp8 and tr.fp8_wgrad and all(all(p.wgrad8_layers.values()) and len(p.wgrad8_layers) == 18 for _, p in E.generator_passes(tr))
    tr0 = E.make_trainer("cpu", BasicFp8EmuOps(), 64, 2, True, True, False)
    a, b = E.inputs(64, 2)
    l0 = tr0.train_iteration(a, b)
    assert l0["loss_G"] == got["loss_G"], (l0, got)      # the weight gradient does not enter the generator's iteration-0 loss
    d = [E.rel_frobenius(x, y) for x, y in zip(E.block_grads(tr), E.block_grads(tr0))]
    print("relative Frobenius difference of the residual weight gradients, e4m3 vs bf16 operands (emulator):", " ".join(f"{v:.4f}" for v in d))
    assert len(d) == 36 and all(0 < v < 0.2 for v in d), d
