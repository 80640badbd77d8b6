"""Palette prior on the CPU: the float64 statement against the reference's recorded values (tests/golden/palette_lab.npz), then the bodies of
tests/palette_cases.py -- the kernel family at its edge shapes, the edge semantics, losses.PalettePriorLoss, cut.CutTrainer with
loss_weights.palette, train_cutpp -- on tests/emulator_palette.py.  tests/test_palette_gpu.py runs the same bodies on the HIP kernels."""
import json
import os

import numpy as np
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from tests import palette_cases as P
from tests import palette_ref64 as R
from tests.emulator_palette import PaletteEmuOps


def test_statement_equals_the_reference_fixture(golden):
    """float64: statistics and analytic gradient to 1e-12 relative of the reference's own functions and their autograd gradient; float32: the
    statement reproduces the reference's float32 run within the family's allowance (so that run is a fair yardstick of fp32 error)"""
    g = golden("palette_lab.npz")
    pm, ps = torch.tensor(g["prior_mean"]), torch.tensor(g["prior_std"])
    assert (tuple(pm.tolist()), tuple(ps.tolist())) == P.FIXTURE_PRIOR
    for tag, (shape, T, seed) in P.FIXTURE_INPUTS.items():
        x = P.fixture_input(shape, seed)
        assert np.array_equal(x.numpy(), g[f"{tag}.x"]) and int(g[f"{tag}.T"]) == T
        m, s = R.stats(x, T)
        for got, key in ((m, "mean"), (s, "std"), (R.grad(x, T, pm, ps), "grad"), (R.loss(x, T, pm, ps), "loss")):
            want = g[f"{tag}.{key}.f64"]
            assert float(np.abs(got.numpy() - want).max()) <= 1e-12 * float(np.abs(want).max()), (tag, key)
        m32, s32 = R.stats(x, T, torch.float32)
        for got, key in ((m32, "mean"), (s32, "std")):
            ref32, ref64 = g[f"{tag}.{key}.f32"], g[f"{tag}.{key}.f64"]
            assert float(np.abs(got.numpy() - ref32).max()) <= 4 * float(np.abs(ref32 - ref64).max()) + P.FLOOR * 100.0, (tag, key)
        g32, r32, r64 = R.grad(x, T, pm, ps, torch.float32).numpy(), g[f"{tag}.grad.f32"], g[f"{tag}.grad.f64"]
        assert float(np.abs(g32 - r32).max()) <= 4 * float(np.abs(r32 - r64).max()) + P.FLOOR * float(np.abs(r64).max()), tag


def test_cells_are_torchs_adaptive_average_pooling():
    """the windows of the statement (overlapping when T does not divide H, repeated pixels when H < T) against torch's own pooling"""
    for (H, W, T) in ((16, 16, 4), (20, 12, 8), (4, 4, 8), (7, 9, 3)):
        x = torch.rand(2, 3, H, W, dtype=torch.float64)
        want = torch.nn.functional.adaptive_avg_pool2d(x, (T, T))
        got = torch.einsum("ih,bchw,jw->bcij", R.pool_matrix(H, T), x, R.pool_matrix(W, T))
        assert float((got - want).abs().max()) < 1e-14


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "B%d_%dx%d_T%d" % s)
def test_family_against_float64(shape, dtype):
    P.body_family(PaletteEmuOps(), "cpu", shape, dtype)


@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "B%d_%dx%d_T%d" % s)
def test_family_with_nan_in_halo_and_pad_channels(shape):
    P.body_family(PaletteEmuOps(), "cpu", shape, BF16, halo=3, nan=True)


def test_saturated_pixels():
    P.body_saturation(PaletteEmuOps(), "cpu")


def test_constant_image():
    P.body_constant(PaletteEmuOps(), "cpu")


def test_nan_pixel_poisons_its_own_image_only():
    P.body_nan_pixel(PaletteEmuOps(), "cpu")


def test_one_cell_is_refused():
    P.body_t1_raises(PaletteEmuOps(), "cpu")


def test_batch_mean_and_prior_update():
    P.body_prior_update(PaletteEmuOps(), "cpu")


def test_autograd_of_the_reference_functions_is_nan_where_the_kernel_is_finite():
    """why the hot path differentiates the branch it took: torch.where's untaken pow branch gives 0 * inf at a black pixel"""
    x = torch.full((1, 3, 4, 4), -1.0, dtype=torch.float64, requires_grad=True)
    v = torch.clamp(x * 0.5 + 0.5, 0, 1)
    f = torch.where(v > 0.008856, torch.pow(v, 1 / 3), (903.3 * v + 16) / 116)
    (g,) = torch.autograd.grad(f.sum(), x)
    assert bool(torch.isnan(g).all())
    pm, ps = (torch.tensor(p, dtype=torch.float64) for p in P.FIXTURE_PRIOR)
    assert bool(torch.isfinite(R.grad(x.detach(), 2, pm, ps)).all())


@pytest.fixture()
def emu_module_api(monkeypatch):
    from gan_variant_research_amd import autograd as AG
    from gan_variant_research_amd import losses as L
    from gan_variant_research_amd import ops_library as OL
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: PaletteEmuOps())
    monkeypatch.setattr(L, "_PLANS", {})
    monkeypatch.setattr(OL, "_PLANS", {})


def test_module_path(emu_module_api):
    P.body_module("cpu")


def test_ops_are_registered(emu_module_api):
    from gan_variant_research_amd import ops_library  # noqa: F401
    for name in ("palette_stats", "palette_prior_fwd", "palette_prior_bwd"):
        assert "Tensor" in str(getattr(torch.ops.mi355x_gan, name).default._schema)


def test_module_step_honours_the_weight(emu_module_api):
    """module_step.train_step reads loss_weights.palette and palette_prior.* like the fused trainer: the dict gains `palette` (the float64
    statement on G(photos) of the step), g_loss its weighted term, and without the weight the dict is what it was"""
    from gan_variant_research_amd import cut as C
    from gan_variant_research_amd import module_step as MS
    from gan_variant_research_amd import training as TR
    torch.set_num_threads(4)
    outs = {}
    for w in (0.0, P.W_PAL):
        cfg = P.config(w=w)
        cfg["model"]["generator"].update(ngf=8, n_blocks=1)
        cfg["model"]["discriminator"].update(ndf=8, n_layers=2)
        cfg["patchnce"]["nce_layers"] = [0, 2]
        C.set_seed(42)
        gen, disc = C.build_models(cfg, "cpu")
        opt_G, opt_D = TR.get_optimizer(gen, cfg["optim"]["G"]), TR.get_optimizer(disc, cfg["optim"]["D"])
        photos, monets = P.batch("cpu")
        with torch.no_grad():
            fake = gen(photos).clone()
        torch.manual_seed(7)
        outs[w] = MS.train_step(0, photos, monets, gen, disc, opt_G, opt_D, None, TR.AMPContext(False), None, cfg, torch.device("cpu"))
        if w > 0:
            prior, prior_tol = P.expected_prior(monets, 1)
            l64, l32 = R.loss(fake, P.T_TR, prior[:, 0], prior[:, 1]), R.loss(fake, P.T_TR, prior[:, 0], prior[:, 1], torch.float32)
            # the discriminator's update precedes the generator's second forward; the generator itself has not moved: G(photos) is `fake`
            assert abs(outs[w]["palette"] - float(l64)) <= P.stat_tol(l32, l64) + 6.0 / 300.0 * prior_tol
    assert "palette" not in outs[0.0] and "palette" in outs[P.W_PAL]
    o = outs[P.W_PAL]
    lw = P.config()["loss_weights"]
    old = lw["adv"] * o["g_adv"] + lw["patchnce"] * o["nce"] + o["identity_weight"] * o["identity"]
    assert abs(o["g_loss"] - (old + P.W_PAL * o["palette"])) <= 1e-5 * max(1.0, abs(o["g_loss"]))


# ------------------------------------------------------------------------------------------------ the fused trainer
@pytest.mark.parametrize("merged,nce", [(True, True), (True, False), (False, True), (False, False)], ids=["merged-fold", "merged-plain", "separate-fold", "separate-plain"])
def test_trainer_term_in_every_shape_of_the_step(merged, nce):
    P.body_trainer_term(PaletteEmuOps, "cpu", merged, nce)


def test_trainer_gradient_is_affine_in_the_weight():
    P.body_linearity(PaletteEmuOps, "cpu")


def test_weight_zero_builds_todays_programs():
    P.body_weight_zero(PaletteEmuOps, "cpu")


def test_saturated_generator_does_not_raise_the_nan_stop():
    P.body_saturated_generator(PaletteEmuOps, "cpu")


def test_checkpoint_carries_the_prior_and_resumes_bit_for_bit(tmp_path):
    P.body_checkpoint(PaletteEmuOps, "cpu", tmp_path)


def test_train_cutpp_with_the_help_texts_override_runs_and_logs_the_key(tmp_path):
    """--set loss_weights.palette=0.5 against a YAML that carries the shipped `palette: {enabled: false}` and `loss_weights.palette: 0.0`"""
    import yaml
    from gan_variant_research_amd import train_cutpp as D
    from tests.test_train_driver import SCHEMA
    cfg = yaml.safe_load(SCHEMA)
    cfg["loss_weights"]["palette"] = 0.0
    cfg["palette"] = {"enabled": False}
    cfg["palette_prior"] = {"low_freq_size": 8, "use_ema": True, "ema_decay": 0.99}
    cfg_path = str(tmp_path / "cfg.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    torch.set_num_threads(4)
    ck, lg = str(tmp_path / "ck"), str(tmp_path / "lg")
    sets = ["loss_weights.palette=0.5", "image_size=32", "batch_size=2", "max_steps=2", "amp=false", f"output.checkpoint_dir={ck}", f"output.log_dir={lg}",
            "metrics.save_checkpoint_every=1", "log_every=1"]
    r = D.main(["--config", cfg_path, "--set"] + sets + ["--synthetic"], ops=PaletteEmuOps(), device="cpu")
    assert r["step"] == 2 and r["losses"]["palette"] > 0
    line = open(os.path.join(lg, "train_log.txt")).read().strip().splitlines()[-1]
    summary = json.loads(line.split(": ", 1)[1])
    assert summary["palette"] > 0
    ckpt = torch.load(os.path.join(ck, "ckpt_final.pt"), weights_only=True)
    assert ckpt["palette_prior"]["steps"] == 2
