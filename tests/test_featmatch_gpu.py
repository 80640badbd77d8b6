"""Feature matching on the GPU: the bodies of tests/featmatch_cases.py on HipOps (tests/test_featmatch_cpu.py runs them on the emulator) --
csrc/featmatch.hip at the issue's shapes against the float64 statement and the header's fp32 statement, the engine's hooks, cut.CutTrainer
with loss_weights.featmatch and the module API."""
import pytest
import torch

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd.runtime import HipOps
from tests import featmatch_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_ops():
    return HipOps(torch.device(DEV))


# ------------------------------------------------------------------------------------------------ the kernel family
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", P.SHAPES, ids=P.SHAPE_ID)
def test_family(shape, dtype):
    P.body_family(make_ops(), DEV, shape, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_nan_element_poisons_the_loss_and_no_other_gradient(dtype):
    P.body_nan_element(make_ops(), DEV, dtype)


def test_mismatched_geometry_is_refused():
    P.body_refusals(make_ops(), DEV)


# ------------------------------------------------------------------------------------------------ the engine
def test_engine_defaults_hooks_and_the_spectral_switch():
    P.body_engine(make_ops, DEV)


# ------------------------------------------------------------------------------------------------ the fused trainer
TRAINER_CASES = [(True, True, 1, False, False), (True, False, 1, False, False), (False, True, 1, False, False), (False, False, 1, False, False),
                 (True, True, 1, True, False), (True, True, 2, True, False), (True, True, 1, False, True), (True, True, 2, True, True)]
TRAINER_IDS = ["merged-nce", "merged-plain", "separate-nce", "separate-plain", "k1-sn", "k2-sn", "k1-aug", "k2-sn-aug"]


@pytest.mark.parametrize("merged,nce,K,sn,aug", TRAINER_CASES, ids=TRAINER_IDS)
def test_trainer_term(merged, nce, K, sn, aug):
    P.body_trainer_term(make_ops, DEV, merged, nce, K, sn, aug)


def test_trainer_gradient_is_affine_in_the_weight_and_matches_float64_autograd():
    P.body_gradient(make_ops, DEV)


def test_one_power_iteration_per_generator_step():
    P.body_one_power_iteration(make_ops, DEV)


def test_nan_stop_covers_the_term():
    P.body_nan_stop(make_ops, DEV)


def test_with_the_palette_prior_the_slots_do_not_collide():
    P.body_with_palette(make_ops, DEV)


# ------------------------------------------------------------------------------------------------ the module API
@pytest.mark.parametrize("name", list(P.GOLDEN_CASES))
def test_intermediate_features_match_the_reference_and_float64_autograd(golden, name):
    P.body_module_features(DEV, golden("featmatch_reference.npz"), name)


def test_feature_matching_loss():
    P.body_feature_matching_loss(DEV)


def test_module_step_has_the_key_only_when_active():
    P.body_module_step(DEV)
