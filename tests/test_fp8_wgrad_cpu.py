"""fp8_wgrad (e4m3 weight gradients of the residual convolutions) on the CPU emulator: what the trainer plans with the switch on, that it
plans exactly the parent's launches with the switch off, the event order that protects the e4m3 gradient buffers, and one emulated step."""
import json
import os

import numpy as np
import pytest
import torch

from gan_variant_research_amd import FP8
from gan_variant_research_amd._lib import GanError
from tests import cases
from tests import emulator_fp8wgrad as E
from tests.emulator import EmuOps
from tests.emulator_fp8wgrad import Fp8WgradEmuOps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fp8_wgrad_parent_launches.json")


def _is_residual(w):
    """A WgradCall summary (LaunchLog) of a residual 3x3 256 -> 256 convolution's weight gradient."""
    return w["ntaps"] == 9 and w["Cx"] == 256 and w["N"] == 256 and (w["x_sy"], w["g_sy"]) == (1, 1)


def _wgrads(log):
    return [(s, a[0][0][1]) for s, n, a in log.entries if n == "conv_wgrad"]


def _geometry(w):
    """The call without buffer ordinals (they shift when a trainer allocates further buffers)."""
    strip = lambda v: v[:7] if isinstance(v, list) and v and v[0] == "V" else v[:3] if isinstance(v, list) and v and v[0] == "T" else v
    return {k: strip(v) for k, v in w.items()}


def test_trainer_builds_with_fp8_wgrad():
    """CutTrainer(fp8=True, fp8_wgrad=True) exists (before the feature: TypeError, unknown keyword) and hands the switch to the generator."""
    tr = E.make_trainer("cpu", Fp8WgradEmuOps(), 64, 2, True, True)
    assert tr.fp8 and tr.fp8_wgrad and tr.G.fp8 and tr.G.fp8_wgrad


def test_fp8_wgrad_without_fp8_is_a_value_error():
    with pytest.raises(ValueError, match="fp8_wgrad needs fp8"):
        E.make_trainer("cpu", Fp8WgradEmuOps(), 64, 2, False, True)
    cfg = cases.small_config()
    cfg["mi355x"] = {"fp8_wgrad": True}
    gen, disc = cases.C.build_models(cfg, "cpu")
    with pytest.raises(ValueError, match="fp8_wgrad needs fp8"):
        cases.C.CutTrainer(gen, disc, cfg, 2, 64, device="cpu", amp=True, ops=Fp8WgradEmuOps())


def test_config_switch_reaches_the_trainer():
    """train_cutpp --set mi355x.fp8=true --set mi355x.fp8_wgrad=true: the overrides land in config['mi355x'], the trainer's default."""
    from gan_variant_research_amd.train_cutpp import override_config
    cfg = override_config(cases.small_config(), ["mi355x.fp8=true", "mi355x.fp8_wgrad=true", "amp=true"])
    assert cfg["mi355x"] == {"fp8": True, "fp8_wgrad": True}
    gen, disc = cases.C.build_models(cfg, "cpu")
    tr = cases.C.CutTrainer(gen, disc, cfg, 2, 64, device="cpu", ops=Fp8WgradEmuOps())
    assert tr.fp8 and tr.fp8_wgrad


def test_exactly_the_residual_weight_gradients_are_e4m3_launches():
    """Step programs at 64x64, batch 2 (16x16 residual maps): per pass and block two weight-gradient launches with dtype FP8, variant 1, on
    the pass's in8 / mid8 copies and an e4m3 gradient buffer; every other weight gradient is the launch the fp8 mode plans."""
    tr, log = E.build_step_programs(Fp8WgradEmuOps(), 64, 2, True, True)
    _, log_off = E.build_step_programs(Fp8WgradEmuOps(), 64, 2, True, False)
    passes = [p for p in tr.G.passes if getattr(p, "wgrad8_layers", None)]
    # merged mode: one generator pass of 2B images; separate mode: G(photos) and G(monets); the PatchNCE feature pass serves both modes
    assert sorted(p.B for p in passes) == [2, 2, 2, 4]
    n8 = 0
    for p in passes:
        nblk = min(tr.G.n_blocks, p.last - 2)
        assert p.wgrad8_layers == {(k, w): True for k in range(nblk) for w in "ab"}
        assert len(p.wgrad8_calls) == 2 * nblk
        calls = iter(p.wgrad8_calls)
        for k in reversed(range(nblk)):          # the backward walks the blocks from the last; second convolution first
            cb, ca = next(calls), next(calls)
            for c, x8 in ((cb, p.mid8[k]), (ca, p.in8[k])):
                assert c.x is x8 and c.x.dtype == FP8 and c.g.dtype == FP8 and c.variant == 1 and c.g.halo == 2 and c.g_scale is not None
                assert c.nsplit == c.B * Fp8WgradEmuOps().wgrad_patch_splits(c)
            assert cb.g.t is not ca.g.t          # alternating buffer sets: a{k % 2} / b{k % 2}
        n8 += 2 * nblk * (2 if p is tr.p2 else 1)      # the feature pass's backward is planned once per mode
    on, off = _wgrads(log), _wgrads(log_off)
    assert len(on) == len(off)
    fp8_on = [w for _, w in on if w["x"][6] == FP8]
    assert len(fp8_on) == n8 and all(_is_residual(w) and w["variant"] == 1 for w in fp8_on)
    assert [s for s, w in on if w["x"][6] == FP8] == ["main.side"] * n8            # on the generator's second stream, like the bf16 ones
    assert sum(_is_residual(w) for _, w in off) == n8 and not any(w["x"][6] == FP8 for _, w in off)
    # the others: same launches, same order
    rest_on = [(s, _geometry(w)) for s, w in on if w["x"][6] != FP8]
    rest_off = [(s, _geometry(w)) for s, w in off if not _is_residual(w)]
    assert rest_on == rest_off
    # and nothing else changed but the weight gradients' place: per op name the same number of launches (the waits that protected the bf16
    # gradient buffers now protect the e4m3 ones -- as many)
    count = lambda lg: {n: sum(1 for _, m, _ in lg.entries if m == n) for n in set(m for _, m, _ in lg.entries)}
    assert count(log) == count(log_off)


@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_switch_off_plans_the_parents_launches(mode):
    """With fp8_wgrad off the trainer asks for exactly the launches, with exactly the arguments, of the commit before the switch existed.
    The parent's sequence is tests/golden/fp8_wgrad_parent_launches.json: recorded ON that commit by build_step_programs (this file's
    recorder copied into its tree) on tests.emulator.EmuOps -- it is not recomputed from the code under test."""
    want = json.load(open(GOLDEN))[mode]
    _, log = E.build_step_programs(EmuOps(), 32, 2, mode == "fp8")
    got = log.hashed()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w, log.entries[i])


def test_main_stream_waits_for_the_side_readers_before_it_rewrites_an_e4m3_gradient_buffer():
    """In every backward program: quantize_fp8 into an e4m3 gradient buffer (main stream) that an earlier side-stream weight gradient of the
    program read is preceded, after that reader, by a main-stream wait on the event the side stream recorded after the reader."""
    tr = E.make_trainer("cpu", Fp8WgradEmuOps(), 64, 2, True, True)
    p = tr.G.new_pass(2, 64, 64)
    p.fwd_program(torch.zeros(2, 3, 64, 64))
    ops, checked = tr.ops, 0
    real_q, real_w = ops.quantize_fp8, ops.conv_wgrad

    def quantize_fp8(src, dst, amax=None, scale_out=None):
        op = real_q(src, dst, amax, scale_out)
        op.writes = [dst.t] + ([scale_out] if scale_out is not None else [])
        return op
    ops.quantize_fp8 = quantize_fp8
    try:
        prog = p.bwd_program(tr.ctx.view(2, 64, 64, 8, 0), accumulate=True)
    finally:
        del ops.quantize_fp8
    assert all(p.wgrad8_layers.values()) and len(p.wgrad8_layers) == 18
    seq = prog.ops
    for i, op in enumerate(seq):
        for buf in getattr(op, "writes", []):
            assert getattr(op, "stream", "main") == "main"
            readers = [j for j in range(i) if getattr(seq[j], "stream", "main") == "side" and hasattr(seq[j], "wgrad")
                       and any(t is not None and t.data_ptr() == buf.data_ptr() for t in (seq[j].wgrad.g.t, seq[j].wgrad.g_scale))]
            if not readers:
                continue
            j = readers[-1]
            rec = next(k for k in range(j + 1, i) if getattr(seq[k], "stream", "main") == "side" and hasattr(seq[k], "ev_record"))
            # nothing else may sit between the reader's launches (conv_wgrad + wgrad_reduce) and the record
            assert all(getattr(seq[k], "stream", "main") != "side" or not hasattr(seq[k], "wgrad") for k in range(j + 1, rec))
            ev = seq[rec].ev_record
            assert any(getattr(seq[k], "stream", "main") == "main" and getattr(seq[k], "ev_wait", None) is ev for k in range(rec + 1, i)), \
                f"op {i} rewrites a buffer the side-stream launch {j} reads without waiting for it"
            checked += 1
    assert checked == 2 * (18 - 4)      # four buffer sets (a0 a1 b0 b1): all but each set's first use rewrite a set that was read; copy and scales


def test_emulated_step_with_fp8_wgrad():
    """One emulated step at 64x64, batch 2 (16x16 residual maps: all 18 layers on the e4m3 path, asserted): losses equal the fp8 step's (the
    weight gradient does not enter step-0 losses), every parameter within 2 lr + 5e-5 = 4.5e-4 of the fp32 oracle's after the update."""
    tr, img, ref = E.run_cut_steps_fp8_wgrad("cpu", Fp8WgradEmuOps(), S=64, B=2, nsteps=1, tol0=8e-2, ptol=4.5e-4, threads=8)
    assert tr.fp8 and tr.fp8_wgrad
    passes = [p for p in tr.G.passes if getattr(p, "wgrad8_layers", None)]
    assert any(len(p.wgrad8_layers) == 18 for p in passes) and all(all(p.wgrad8_layers.values()) for p in passes)
    tr0 = E.make_trainer("cpu", Fp8WgradEmuOps(), 64, 2, True, False)
    tr1 = E.make_trainer("cpu", Fp8WgradEmuOps(), 64, 2, True, True)
    l0, l1 = E.run_steps(tr0, 64, 2, 1, "cpu")[0], E.run_steps(tr1, 64, 2, 1, "cpu")[0]
    assert l0 == l1, (l0, l1)
    d = [E.rel_frobenius(a, b) for a, b in zip(E.block_grads(tr1), E.block_grads(tr0))]
    print("relative Frobenius difference of the residual weight gradients, e4m3 vs bf16 operands (emulator):", " ".join(f"{v:.4f}" for v in d))
    assert all(0 < v < 0.2 for v in d), d       # the e4m3 path really ran (not bit-equal) and is the same gradient up to the format


def test_maps_under_128_pixels_keep_the_bf16_weight_gradient():
    """32x32 images: the residual maps are 8x8 = 64 pixels, the e4m3 kernel does not take them -> bf16 launches, as without the switch."""
    tr, log = E.build_step_programs(Fp8WgradEmuOps(), 32, 2, True, True)
    passes = [p for p in tr.G.passes if getattr(p, "wgrad8_layers", None)]
    assert passes and all(not any(p.wgrad8_layers.values()) and not p.wgrad8_calls for p in passes)
    assert not any(w["x"][6] == FP8 for _, w in _wgrads(log))
    conv = tr.G.c_blk[0][0]
    p = passes[0]
    with pytest.raises(GanError):
        conv.wgrad8(p.in8[0], tr.ctx.view(p.B, 8, 8, 256, 2, dtype=FP8), None, False)
