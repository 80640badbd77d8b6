"""cut.CutTrainer with optim.{G,D}.weight_decay and mi355x.decoupled_weight_decay on the GPU: the bodies of tests/cut_wd_cases.py on HipOps
(tests/test_cut_trainer_wd_cpu.py runs them on the emulator)."""
import pytest
import torch

from gan_variant_research_amd.runtime import HipOps
from tests import cut_wd_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_ops():
    return HipOps(torch.device(DEV))


@pytest.fixture(scope="module")
def l2_trainer():
    return T.body_config_and_update(make_ops, DEV, False, True)


def test_l2_decay_builds_launches_and_updates_as_the_statement(l2_trainer):
    assert l2_trainer[0].opt_G.weight_decay == T.WD_G


def test_decoupled_decay_builds_launches_and_updates_as_the_statement():
    T.body_config_and_update(make_ops, DEV, True, False)


def test_checkpoint_carries_the_decay_and_resumes_bit_for_bit(l2_trainer, tmp_path):
    T.body_checkpoint(make_ops, DEV, *l2_trainer, tmp_path)
