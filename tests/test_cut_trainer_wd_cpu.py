"""cut.CutTrainer with optim.{G,D}.weight_decay and mi355x.decoupled_weight_decay, host logic on the CPU (tests/emulator_optim_wd.py): the
update programs launch gan_adam_step_wd, a generator update equals the float64 statement, the R1 skip table still protects its tensors, the
checkpoint carries the decay and resumes bit for bit, and train_cutpp --set optim.G.weight_decay=1e-4 runs.
tests/test_cut_trainer_wd_gpu.py runs the same bodies on the HIP kernels."""
import os

import pytest
import torch
import yaml

from tests import cut_wd_cases as T
from tests.emulator_optim_wd import WdEmuOps


class NamedWdEmuOps(WdEmuOps):
    """the emulator's optimiser launches carry the name of the entry point HipOps would call"""

    def adam_step(self, *a, **k):
        op = super().adam_step(*a, **k)
        op.__name__ = "gan_adam_step"
        return op

    def adam_step_wd(self, *a, **k):
        inner = super().adam_step_wd(*a, **k)

        def op():
            inner()
        op.__name__ = "gan_adam_step_wd" if a[14] != 0.0 else "gan_adam_step"
        return op


@pytest.fixture(scope="module")
def l2_trainer():
    return T.body_config_and_update(NamedWdEmuOps, "cpu", False, True)


def test_l2_decay_builds_launches_and_updates_as_the_statement(l2_trainer):
    assert l2_trainer[0].opt_G.weight_decay == T.WD_G


def test_decoupled_decay_builds_launches_and_updates_as_the_statement():
    T.body_config_and_update(NamedWdEmuOps, "cpu", True, False)


def test_checkpoint_carries_the_decay_and_resumes_bit_for_bit(l2_trainer, tmp_path):
    T.body_checkpoint(NamedWdEmuOps, "cpu", *l2_trainer, tmp_path)


def test_train_cutpp_with_a_weight_decay_override_runs_and_checkpoints(tmp_path):
    from gan_variant_research_amd import train_cutpp as D
    from tests.test_train_driver import SCHEMA
    cfg_path = str(tmp_path / "cfg.yaml")
    with open(cfg_path, "w") as f:
        f.write(SCHEMA)
    torch.set_num_threads(4)
    ck, lg = str(tmp_path / "ck"), str(tmp_path / "lg")
    sets = ["optim.G.weight_decay=1e-4", "image_size=32", "batch_size=2", "max_steps=2", "amp=false", f"output.checkpoint_dir={ck}", f"output.log_dir={lg}",
            "metrics.save_checkpoint_every=1", "log_every=1"]
    calls = []

    class Ops(NamedWdEmuOps):
        def adam_step_wd(self, *a, **k):
            calls.append(a[14])
            return super().adam_step_wd(*a, **k)
    r = D.main(["--config", cfg_path, "--set"] + sets + ["--synthetic"], ops=Ops(), device="cpu")
    assert r["step"] == 2 and calls and set(calls) == {1e-4}
    ckpt = torch.load(os.path.join(ck, "ckpt_final.pt"), weights_only=True)
    assert ckpt["opt_G"]["param_groups"][0]["weight_decay"] == 1e-4 and ckpt["opt_D"]["param_groups"][0]["weight_decay"] == 0.0
    assert yaml.safe_load(SCHEMA)["optim"]["G"].get("weight_decay", 0.0) == 0.0
