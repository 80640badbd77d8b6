"""Feature matching on the CPU: the bodies of tests/featmatch_cases.py -- the kernel family at the issue's shapes, the engine's hooks,
cut.CutTrainer with loss_weights.featmatch, the module API against the reference's recorded features -- on tests/emulator_featmatch.py.
tests/test_featmatch_gpu.py runs the same bodies on the HIP kernels."""
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from tests import featmatch_cases as P
from tests.emulator_featmatch import FeatmatchEmuOps


# ------------------------------------------------------------------------------------------------ the kernel family
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", P.SHAPES, ids=P.SHAPE_ID)
def test_family(shape, dtype):
    P.body_family(FeatmatchEmuOps(), "cpu", shape, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_nan_element_poisons_the_loss_and_no_other_gradient(dtype):
    P.body_nan_element(FeatmatchEmuOps(), "cpu", dtype)


def test_mismatched_geometry_is_refused():
    P.body_refusals(FeatmatchEmuOps(), "cpu")


# ------------------------------------------------------------------------------------------------ the engine
def test_engine_defaults_hooks_and_the_spectral_switch():
    P.body_engine(FeatmatchEmuOps, "cpu")


# ------------------------------------------------------------------------------------------------ the fused trainer
TRAINER_CASES = [(True, True, 1, False, False), (True, False, 1, False, False), (False, True, 1, False, False), (False, False, 1, False, False),
                 (True, True, 1, True, False), (True, True, 2, True, False), (True, True, 1, False, True), (True, True, 2, True, True)]
TRAINER_IDS = ["merged-nce", "merged-plain", "separate-nce", "separate-plain", "k1-sn", "k2-sn", "k1-aug", "k2-sn-aug"]


@pytest.mark.parametrize("merged,nce,K,sn,aug", TRAINER_CASES, ids=TRAINER_IDS)
def test_trainer_term(merged, nce, K, sn, aug):
    P.body_trainer_term(FeatmatchEmuOps, "cpu", merged, nce, K, sn, aug)


def test_trainer_gradient_is_affine_in_the_weight_and_matches_float64_autograd():
    P.body_gradient(FeatmatchEmuOps, "cpu")


def test_one_power_iteration_per_generator_step():
    P.body_one_power_iteration(FeatmatchEmuOps, "cpu")


def test_nan_stop_covers_the_term():
    P.body_nan_stop(FeatmatchEmuOps, "cpu")


def test_with_the_palette_prior_the_slots_do_not_collide():
    from tests.emulator_palette import PaletteEmuOps

    class BothEmuOps(FeatmatchEmuOps, PaletteEmuOps):
        pass
    P.body_with_palette(BothEmuOps, "cpu")


# ------------------------------------------------------------------------------------------------ the module API
@pytest.fixture()
def emu_module_api(monkeypatch):
    from gan_variant_research_amd import autograd as AG
    from gan_variant_research_amd import losses as L
    from gan_variant_research_amd import ops_library as OL
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: FeatmatchEmuOps())
    monkeypatch.setattr(L, "_PLANS", {})
    monkeypatch.setattr(OL, "_PLANS", {})


@pytest.mark.parametrize("name", list(P.GOLDEN_CASES))
def test_intermediate_features_match_the_reference_and_float64_autograd(emu_module_api, golden, name):
    P.body_module_features("cpu", golden("featmatch_reference.npz"), name)


def test_reference_module_api_no_longer_raises_attribute_error(emu_module_api):
    from gan_variant_research_amd import cut as C
    from gan_variant_research_amd import losses as L
    assert callable(C.MultiscaleDiscriminator.get_intermediate_features) and callable(L.feature_matching_loss)


def test_feature_matching_loss(emu_module_api):
    P.body_feature_matching_loss("cpu")


def test_module_step_has_the_key_only_when_active(emu_module_api):
    P.body_module_step("cpu")
