"""inference.load_generator on a CycleGAN checkpoint (the dict of Basic_GAN/src/train.py:127-137, as basic.CycleGANTrainer saves it):
recognised by its keys, loaded strictly into basic.ResnetGenerator of the architecture the keys tell; `which` picks the generator; a CUT
checkpoint loads as before.  CPU: the trainer and the generator pass run on the emulator."""
import pytest
import torch

from gan_variant_research_amd import autograd as AG, basic as BG, cut as C, generate_folder as GF, inference as I
from tests import cases
from tests.emulator import EmuOps
from tests.emulator_infer import InferEmuOps


@pytest.fixture(scope="module")
def cyclegan_ckpt(tmp_path_factory):
    """A checkpoint of the emulator-driven trainer after one iteration: 6 blocks, ngf 8."""
    cfg = cases.basic_config()
    cfg["model"].update({"ngf": 8, "ndf": 8, "n_blocks": 6})
    cfg["training"].update({"epochs": 2, "save_every": 1})
    torch.manual_seed(0)
    tr = BG.CycleGANTrainer(*BG.build_models(cfg, "cpu"), cfg, 1, 16, device="cpu", amp=False, ops=EmuOps())
    g = torch.Generator().manual_seed(3)
    tr.train_iteration(torch.rand(1, 3, 16, 16, generator=g) * 2 - 1, torch.rand(1, 3, 16, 16, generator=g) * 2 - 1)
    path = str(tmp_path_factory.mktemp("basic") / "ckpt_e1.pt")
    tr.save_checkpoint(path, 1)
    return path


@pytest.mark.parametrize("which", [None, "G_A2B", "G_B2A"])
def test_cyclegan_checkpoint_loads_the_named_generator(cyclegan_ckpt, which, capsys):
    ck = torch.load(cyclegan_ckpt, weights_only=True)
    assert I.is_cyclegan_checkpoint(ck)
    G = I.load_generator(cyclegan_ckpt, device="cpu", bf16=False, **({} if which is None else {"which": which}))
    assert capsys.readouterr().out == ""                       # strict: nothing missing, nothing to warn about
    assert type(G) is BG.ResnetGenerator and G.n_blocks == 6 and G.ngf == 8 and not G.training
    want = ck[which or "G_A2B"]
    sd = G.state_dict()
    assert list(sd) == list(want) and all(torch.equal(sd[k], want[k]) for k in want)
    assert not any(p.requires_grad for p in G.parameters())
    other = ck["G_B2A" if (which or "G_A2B") == "G_A2B" else "G_A2B"]
    assert any(not torch.equal(sd[k], other[k]) for k in other)      # the two generators differ after a step


def test_loaded_generator_stylizes_on_the_emulator(cyclegan_ckpt, monkeypatch):
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: InferEmuOps())
    G = I.load_generator(cyclegan_ckpt, device="cpu", bf16=False, which="G_B2A")
    x = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(4)) * 2 - 1
    with torch.no_grad():
        want = I.to_uint8(G(x)).permute(0, 2, 3, 1)
    assert torch.equal(G.forward_u8(x), want) and torch.equal(I.stylize_hwc(G, x), want) and torch.equal(I.stylize(G, x), want.permute(0, 3, 1, 2))
    assert len(set(want.flatten().tolist())) > 8


def test_bad_which_and_broken_checkpoint_raise(cyclegan_ckpt, tmp_path):
    with pytest.raises(ValueError, match="G_A2B and G_B2A"):
        I.load_generator(cyclegan_ckpt, device="cpu", which="G")
    ck = torch.load(cyclegan_ckpt, weights_only=True)
    del ck["G_A2B"]["net.12.block.5.weight"]
    torch.save(ck, tmp_path / "broken.pt")
    with pytest.raises(RuntimeError, match="net.12.block.5.weight"):          # strictly: never a silent run on random weights
        I.load_generator(str(tmp_path / "broken.pt"), device="cpu")
    a = GF.parse_args(["--ckpt", "c", "--photos", "p", "--out", "o"])
    assert a.which == "G_A2B" and GF.parse_args(["--ckpt", "c", "--photos", "p", "--out", "o", "--which", "G_B2A"]).which == "G_B2A"


def test_cut_checkpoint_still_yields_the_cut_generator(tmp_path, capsys):
    torch.manual_seed(3)
    G = C.ResNetGenerator(3, 3, ngf=8, n_blocks=2)
    shadow = {k: v.detach() * 0.5 for k, v in G.state_dict().items()}
    torch.save({"step": 7, "generator": G.state_dict(), "ema_G": {"decay": 0.999, "shadow": shadow}, "config": {}}, tmp_path / "ckpt_final.pt")
    G2 = I.load_generator(str(tmp_path / "ckpt_final.pt"), device="cpu", ngf=8, n_blocks=2, which="G_B2A")      # `which` does not apply
    assert type(G2) is C.ResNetGenerator and capsys.readouterr().out == ""
    assert all(torch.equal(v, shadow[k]) for k, v in G2.state_dict().items())
