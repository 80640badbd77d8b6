"""cut.CutTrainer and module_step.train_step with patchnce.nce_includes_all_negatives_from_minibatch on the emulator, 64 x 64, batch 2, the
shipped PatchNCE layers (bodies: tests/cut_nce_all_cases.py; tests/test_cut_nce_all_gpu.py runs the first two on the HIP kernels).  Until
the key was read, `true` trained exactly as `false` does: the second test fails on such a trainer."""
import numpy as np
import torch

from gan_variant_research_amd import autograd as AG
from gan_variant_research_amd import cut as C
from tests import cut_nce_all_cases as K
from tests.emulator_nce_all import NceAllEmuOps


def test_key_true_is_the_float64_statement_on_the_trainers_own_features():
    K.body_term(NceAllEmuOps, "cpu", False)


def test_key_true_differs_from_key_false_by_more_than_both_bounds():
    nce_img, bound = K.key_false_step(NceAllEmuOps, "cpu", False)
    nce_all = K.nce_of(NceAllEmuOps, "cpu", True, False)
    nce_absent = K.nce_of(NceAllEmuOps, "cpu", None, False)
    print(f"[cut-nce-all] nce: key true {nce_all:.8g}, key false {nce_img:.8g}, bound of one path {bound:.3g}")
    assert nce_absent == nce_img
    assert nce_all - nce_img > 2 * bound, "with the key true the step computes what it computes with the key false"


def test_batch_of_one_agrees_with_key_false():
    nce_all, bound, _ = K.body_term(NceAllEmuOps, "cpu", False, n=1)
    nce_img = K.nce_of(NceAllEmuOps, "cpu", False, False, n=1)
    assert abs(nce_all - nce_img) <= 2 * bound, (nce_all, nce_img, bound)


def test_module_step_reads_the_key_like_the_trainer(monkeypatch):
    """module_step.train_step with the key true against the fused trainer, with the tolerances of
    test_autograd_bridge.test_fused_trainer_matches_module_step_over_three_steps; and it differs from the key-false value"""
    from gan_variant_research_amd import losses as L, module_step as MS, training as T
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: NceAllEmuOps())
    monkeypatch.setattr(L, "_PLANS", {})
    cfg = K.config(True)
    tr = K.trainer(NceAllEmuOps(), "cpu", cfg)
    C.set_seed(42)
    gen2, disc2 = C.build_models(cfg, "cpu")
    opt_G, opt_D = T.get_optimizer(gen2, cfg["optim"]["G"]), T.get_optimizer(disc2, cfg["optim"]["D"])
    ema, amp = T.EMA(gen2, cfg["ema"]["decay"], optimizer=opt_G), T.AMPContext(False)
    photos, monets = K.batch("cpu")
    torch.manual_seed(9000)
    rnd = tr.sample_randomness()
    a = tr.train_step(0, photos, monets, rnd)
    b = MS.train_step(0, photos, monets, gen2, disc2, opt_G, opt_D, ema, amp, None, cfg, torch.device("cpu"), rnd={"nce_ids": rnd["nce_ids"]})
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=2e-3, atol=1e-3 if k == "g_adv" else 2e-4, err_msg=k)
    assert abs(b["nce"] - K.nce_of(NceAllEmuOps, "cpu", False, False)) > 0.1
