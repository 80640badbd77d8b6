"""cut.CutTrainer with patchnce.nce_includes_all_negatives_from_minibatch on the HIP kernels, 64 x 64, batch 2, the shipped PatchNCE layers,
fp32 and bf16 (bodies: tests/cut_nce_all_cases.py): the step's `nce` and the gradient the hooks add are the float64 statement on the trainer's
own feature buffers, and `nce` differs from the key-false step's by more than both bounds."""
import pytest
import torch

from gan_variant_research_amd.runtime import HipOps
from tests import cut_nce_all_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_ops():
    return HipOps(torch.device(DEV))


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_key_true_is_the_float64_statement_on_the_trainers_own_features(amp):
    K.body_term(make_ops, DEV, amp)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_key_true_differs_from_key_false_by_more_than_both_bounds(amp):
    nce_img, bound = K.key_false_step(make_ops, DEV, amp)
    nce_all = K.nce_of(make_ops, DEV, True, amp)
    print(f"[cut-nce-all] nce: key true {nce_all:.8g}, key false {nce_img:.8g}, bound of one path {bound:.3g}")
    assert nce_all - nce_img > 2 * bound, "with the key true the step computes what it computes with the key false"
