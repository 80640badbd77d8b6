"""Generates tests/golden/basic_sn.npz: two iterations of the reference's CycleGAN loop with spectral-norm discriminators.

Run from the repo root on a machine that has the reference checkout (build machine only):  python tools/make_golden_basic_sn.py

The loop is the restated inner loop of oracle/make_golden.py (gen_basic: Basic_GAN/src/train.py:66-122) with the reference's own
ResnetGenerator / NLayerDiscriminator(spectral=True) / GANLoss and torch's Adam: ngf 16, n_blocks 6, ndf 8, 64x64, batch 2, seed 0,
amp off, lsgan, lambda 10 / 0.5, Adam 2e-4 (0.5, 0.999).  Every D forward runs in training mode, so each discriminator runs three power
iterations per iteration (G-step D(fake), D-step D(real), D-step D(fake.detach())).

Pinned (float32 run): the initial D_A / D_B state_dicts, 16-value slices of the generators, both inputs, the three losses per iteration,
weight_u / weight_v of the six spectral-norm convolutions after each iteration, and the iteration-0 D-step gradients of every D parameter.
Beside them, for each pinned quantity q (max |difference| / max |reference|):
  spread.q       float32 run vs the same loop in float64 (the reference's own rounding error);
  wrong.nopi.q   the D-step's fake forward without its power iteration (that forward in eval mode);
  wrong.plain.q  spectral norm ignored: plain convolutions on weight_orig;
  wrong.nobwd.q  the spectral-norm backward skipped: the weight_orig gradient replaced by dL/dW_sn (summed over the D-step's two forwards).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import _import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "basic_sn.npz")
NGF, NB, NDF, S, B = 16, 6, 8, 64, 2
SN_KEYS = ("net.2", "net.5", "net.8")


def _inputs():
    g = torch.Generator().manual_seed(77)
    return torch.rand(B, 3, S, S, generator=g) * 2 - 1, torch.rand(B, 3, S, S, generator=g) * 2 - 1


def run(dtype=torch.float32, variant="ref"):
    """The loop; variant: 'ref', 'nopi' (no power iteration in the D-step fake forward) or 'plain' (spectral norm ignored).
    -> (pinned quantities, initial state, dL/dW_sn of the iteration-0 D-steps)."""
    from src.losses import GANLoss, cycle_loss, identity_loss  # Basic_GAN/src
    from src.models import NLayerDiscriminator, ResnetGenerator
    from torch.optim import Adam

    torch.manual_seed(0)
    G_ab, G_ba = ResnetGenerator(ngf=NGF, n_blocks=NB), ResnetGenerator(ngf=NGF, n_blocks=NB)
    D_a, D_b = NLayerDiscriminator(ndf=NDF, spectral=True), NLayerDiscriminator(ndf=NDF, spectral=True)
    init = {}
    for name, net in (("G_ab", G_ab), ("G_ba", G_ba)):
        for k, v in net.state_dict().items():
            init[f"init.{name}.{k}"] = v.reshape(-1)[:16].clone()
    for name, net in (("D_A", D_a), ("D_B", D_b)):
        for k, v in net.state_dict().items():
            init[f"init.{name}.{k}"] = v.clone()
    rename = {}
    if variant == "plain":           # same initial weights, no spectral norm
        plain = []
        for D in (D_a, D_b):
            P = NLayerDiscriminator(ndf=NDF, spectral=False)
            sd = {k.replace("weight_orig", "weight"): v for k, v in D.state_dict().items() if not k.endswith(("_u", "_v"))}
            P.load_state_dict(sd)
            plain.append(P)
        D_a, D_b = plain
        rename = {f"{k}.weight": f"{k}.weight_orig" for k in SN_KEYS}
    nets = [G_ab, G_ba, D_a, D_b]
    for n in nets:
        n.to(dtype)
    a, b = (t.to(dtype) for t in _inputs())
    # dL/dW_sn of the D-step: the normalised weight each forward used (a pre-hook registered after spectral norm's own)
    capture, wsn = [False], {}
    for dname, D in (("D_A", D_a), ("D_B", D_b)):
        for k in SN_KEYS:
            conv = D.net[int(k.split(".")[1])]
            conv.register_forward_pre_hook(lambda mod, inp, key=(dname, k): wsn.setdefault(key, []).append(mod.weight) if capture[0] else None)
    gan = GANLoss("lsgan")
    oG = Adam(list(G_ab.parameters()) + list(G_ba.parameters()), lr=2e-4, betas=(0.5, 0.999))
    oA = Adam(D_a.parameters(), lr=2e-4, betas=(0.5, 0.999))
    oB = Adam(D_b.parameters(), lr=2e-4, betas=(0.5, 0.999))
    out, gsn = {}, {}

    def fake_forward(D, x):
        if variant != "nopi":
            return D(x)
        D.eval()                     # spectral norm's hook skips the power iteration outside training mode
        try:
            return D(x)
        finally:
            D.train()

    def d_step(name, D, opt, real, fake, it):
        opt.zero_grad(set_to_none=True)
        capture[0] = it == 0 and variant == "ref"
        loss = 0.5 * (gan(D(real), True) + gan(fake_forward(D, fake.detach()), False))
        capture[0] = False
        if it == 0 and variant == "ref":
            for k in SN_KEYS:
                ws = wsn[(name, k)]
                gsn[f"grad0.{name}.{k}.weight_orig"] = sum(torch.autograd.grad(loss, ws, retain_graph=True)).detach().clone()
        loss.backward()
        if it == 0:
            for k, p in D.named_parameters():
                out[f"grad0.{name}.{rename.get(k, k)}"] = p.grad.detach().clone()
        opt.step()
        return loss

    for it in range(2):
        oG.zero_grad(set_to_none=True)
        fake_B = G_ab(a); rec_A = G_ba(fake_B); fake_A = G_ba(b); rec_B = G_ab(fake_A)
        idt_B = G_ab(b); idt_A = G_ba(a)
        loss_G = (gan(D_b(fake_B), True) + gan(D_a(fake_A), True) + cycle_loss(rec_A, a, 10.0) + cycle_loss(rec_B, b, 10.0)
                  + identity_loss(idt_A, a, 0.5) + identity_loss(idt_B, b, 0.5))
        loss_G.backward(); oG.step()
        loss_A = d_step("D_A", D_a, oA, a, fake_A, it)
        loss_B = d_step("D_B", D_b, oB, b, fake_B, it)
        out[f"it{it}.loss_G"], out[f"it{it}.loss_D_A"], out[f"it{it}.loss_D_B"] = loss_G.detach(), loss_A.detach(), loss_B.detach()
        if variant != "plain":
            for name, D in (("D_A", D_a), ("D_B", D_b)):
                for k, v in D.state_dict().items():
                    if k.endswith(("_u", "_v")):
                        out[f"it{it}.{name}.{k}"] = v.clone()
    return out, init, gsn


def dist(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).abs().max() / ref.abs().max())


def main():
    _import_reference()
    torch.set_num_threads(1)
    ref, init, gsn = run(torch.float32, "ref")
    f64, _, _ = run(torch.float64, "ref")
    nopi, _, _ = run(torch.float32, "nopi")
    plain, _, _ = run(torch.float32, "plain")
    a, b = _inputs()
    out = {"real_a": a, "real_b": b, **init, **ref}
    for k, v in ref.items():
        out[f"spread.{k}"] = torch.tensor(dist(v, f64[k]), dtype=torch.float64)
        if k in nopi:
            out[f"wrong.nopi.{k}"] = torch.tensor(dist(nopi[k], v), dtype=torch.float64)
        if k in plain:
            out[f"wrong.plain.{k}"] = torch.tensor(dist(plain[k], v), dtype=torch.float64)
        if k in gsn:
            out[f"wrong.nobwd.{k}"] = torch.tensor(dist(gsn[k], v), dtype=torch.float64)
    np.savez_compressed(OUT, **{k: v.detach().numpy() for k, v in out.items()})
    for group in ("spread", "wrong.nopi", "wrong.plain", "wrong.nobwd"):
        for kind in ("loss", "weight_u", "weight_v", "grad0"):
            vals = [float(out[k]) for k in out if k.startswith(group + ".") and kind in k]
            if vals:
                print(f"{group:12s} {kind:9s} n={len(vals):3d} min {min(vals):.3g} max {max(vals):.3g}")
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
