"""Records what the discriminator family plans and computes BEFORE its three host-side planners (the multiscale net of the CUT trainer,
the partially normalised net of the CycleGAN trainer, the autograd bridge's own loops) became one, for
tests/test_dfamily_parent_launches.py and tests/test_dfamily_bridge_gpu.py.

The records were made on the commit before the merge (this file copied into its tree, as tools/make_golden_plan.py describes for its own)
and are never recomputed from the code under test:

  python tools/make_golden_dfamily_plan.py launches       -> tests/golden/dfamily_parent_launches.json
      "launches": LaunchLog.hashed() of every launch the fused trainers of RECORDS plan (tests.emulator_fp8wgrad.RecOps on
      DFamilyEmuOps; nothing is stepped; pack / unpack of make_golden_plan.py).  Building a trainer plans its step programs, R1, the
      update / repack programs and refresh_pack; the CUT trainers are switched through both identity modes.
      "bridge": for every module-API discriminator of BRIDGE, the number of launches per "stream name" that the autograd bridge plans
      for a slot's forward, for its backward with each (need_x, need_w) and for R1 (EmuOps through autograd._OPS_FACTORY).
  python tools/make_golden_dfamily_plan.py gpu [--out F]  -> tests/golden/dfamily_bridge_parent_gpu.json
      on the MI355X, fp32: ms3 / sn2 / bsn of tests/golden/cut_optional.npz through the module API -- SHA-256 of every scale's logits, of
      the input and parameter gradients of test_autograd_bridge.optional_cases' loss mix, the R1 value (float.hex()) with its parameter
      gradients, and weight_u / weight_v afterwards.  Each case runs twice from fresh modules and is written only if both runs agree.
"""
from __future__ import annotations

import collections
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_plan import pack, unpack  # noqa: E402
from tests import emulator_basic_sn as EB  # noqa: E402
from tests.emulator_fp8wgrad import RecOps  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
B, NDF = 2, 4
# name -> (trainer, discriminator scales, spectral norm, image size, bf16); the size is the smallest whose last scale still has a logit map
RECORDS = {
    "cut_ms3_fp32": ("cut", 3, False, 96, False),
    "cut_sn2_fp32": ("cut", 2, True, 64, False),
    "cut_sn1_fp32": ("cut", 1, True, 64, False),
    "cut_ms3_bf16": ("cut", 3, False, 96, True),
    "cut_sn2_bf16": ("cut", 2, True, 64, True),
    "cut_sn1_bf16": ("cut", 1, True, 64, True),
    "basic_sn_fp32": ("basic", 1, True, 64, False),
    "basic_sn_bf16": ("basic", 1, True, 64, True),
}
# name -> (style, scales, spectral norm, image size, R1)
BRIDGE = {
    "cut_plain": ("cut", 1, False, 64, True),
    "ms3": ("cut", 3, False, 96, True),
    "sn2": ("cut", 2, True, 64, True),
    "bsn": ("basic", 1, True, 64, False),
    "basic_plain": ("basic", 1, False, 64, False),
}
GPU_TAGS = ("ms3", "sn2", "bsn")


def plan(name):
    """The trainer of RECORDS[name] built on a recording op layer -> its LaunchLog."""
    from tests import cases
    from tests.emulator_dfamily import DFamilyEmuOps
    which, K, sn, S, amp = RECORDS[name]
    rec = RecOps(DFamilyEmuOps())
    if which == "basic":
        from gan_variant_research_amd import basic as BG
        cfg = EB.basic_sn_config(sn, amp)
        cfg["model"]["ndf"] = NDF
        BG.CycleGANTrainer(*EB.make_models(cfg), cfg, B, S, device="cpu", amp=amp, ops=rec)
        return rec.log
    C = cases.C
    cfg = cases.small_config()
    cfg["diffaugment"]["enable"] = True
    cfg["model"]["discriminator"].update(num_scales=K, use_spectral_norm=sn, ndf=NDF)
    cfg["model"]["generator"].update(ngf=16, n_blocks=3)
    C.set_seed(42)
    gen, disc = C.build_models(cfg, "cpu")
    tr = C.CutTrainer(gen, disc, cfg, B, S, device="cpu", amp=amp, ops=rec)
    tr._use_mode(True)
    tr._use_mode(False)
    return rec.log


def bridge_module(name):
    from gan_variant_research_amd import basic as BG, cut as C
    style, K, sn, _, _ = BRIDGE[name]
    torch.manual_seed(0)
    if style == "basic":
        return BG.NLayerDiscriminator(3, NDF, 3, spectral=sn)
    return C.MultiscaleDiscriminator(3, NDF, 3, num_scales=K, use_spectral_norm=sn)


def bridge_counts(name):
    """{phase: {"stream name": launches planned}} of the bridge of BRIDGE[name]."""
    from gan_variant_research_amd import autograd as AG
    from tests.emulator import EmuOps
    S, r1 = BRIDGE[name][3], BRIDGE[name][4]
    rec = RecOps(EmuOps())
    saved = AG._OPS_FACTORY
    AG._OPS_FACTORY = lambda device: rec
    out = {}

    def phase(tag, mark):
        out[tag] = dict(sorted(collections.Counter(f"{s} {n}" for s, n, _ in rec.log.entries[mark:]).items()))
        return len(rec.log.entries)
    try:
        torch.set_num_threads(4)
        D = bridge_module(name)
        x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1
        mark = len(rec.log.entries)
        outs = D(x.clone().requires_grad_(True))
        outs = outs if isinstance(outs, list) else [outs]
        mark = phase("fwd", mark)
        bridge = D._hip_bridge
        (slot,) = [s for slots in bridge.pool.values() for s in slots]
        for need_x in (True, False):
            for need_w in (True, False):
                bridge.backward(slot, [torch.zeros_like(o) for o in outs], need_x, need_w)
                mark = phase(f"bwd_x{int(need_x)}_w{int(need_w)}", mark)
        if r1:
            AG.r1_regularization(D, x)
            phase("r1", mark)
    finally:
        AG._OPS_FACTORY = saved
    return out


def launches(out):
    rec = {name: plan(name).hashed() for name in RECORDS}
    assert unpack(pack(rec)) == rec
    blob = {"launches": pack(rec), "bridge": {name: bridge_counts(name) for name in BRIDGE}}
    with open(out, "w") as f:
        json.dump(blob, f, separators=(",", ":"))
    print({k: len(v) for k, v in rec.items()}, {k: {p: sum(c.values()) for p, c in v.items()} for k, v in blob["bridge"].items()}, "->", out)


def _sha(t):
    return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()


def bridge_bits(tag, dev="cuda:0"):
    """One case of test_autograd_bridge.optional_cases (same inputs, state dict and loss mix) from a fresh module -> its bit-level record."""
    from gan_variant_research_amd import autograd as AG, basic as BG, cut as C, losses as L
    g = np.load(os.path.join(GOLDEN, "cut_optional.npz"))
    T = lambda k: torch.from_numpy(np.asarray(g[k])).to(dev)
    x, y = T("x"), T("y")
    if tag == "bsn":
        D = BG.NLayerDiscriminator(3, 4, 3, spectral=True).to(dev)
        x, y = x[:, :, :64, :64].contiguous(), y[:, :, :64, :64].contiguous()
    else:
        ns, sn = (3, False) if tag == "ms3" else (2, True)
        D = C.MultiscaleDiscriminator(3, 4, 3, num_scales=ns, use_spectral_norm=sn).to(dev)
    D.load_state_dict({k[len(tag) + 4:]: T(k) for k in g.files if k.startswith(f"{tag}.sd.")})
    if tag != "ms3":
        D(x)                                            # the fixture ran one extra training-mode forward first
    xr = x.clone().requires_grad_(True)
    outs = D(xr)
    if tag == "bsn":
        loss = L.GANLoss("lsgan")(outs, True) + 0.5 * L.GANLoss("lsgan")(D(y), False)
        outs = [outs]
    else:
        loss = L.discriminator_hinge_loss(outs, D(y)) + 0.25 * L.generator_hinge_loss(outs)
    names = [k for k, _ in D.named_parameters()]
    grads = torch.autograd.grad(loss, [xr] + [p for _, p in D.named_parameters()])
    rec = {f"out{i}": _sha(o) for i, o in enumerate(outs)}
    rec["loss"] = float(loss.detach()).hex()
    rec["gx"] = _sha(grads[0])
    rec.update({f"gw.{k}": _sha(gr) for k, gr in zip(names, grads[1:])})
    if tag != "bsn":
        D.zero_grad()
        r1 = AG.r1_regularization(D, x.clone())
        rec["r1"] = float(r1.detach()).hex()
        r1.backward()
        rec.update({f"r1.gw.{k}": None if p.grad is None else _sha(p.grad) for k, p in D.named_parameters()})
    rec.update({f"buf.{k}": _sha(v) for k, v in D.state_dict().items() if k.endswith(("weight_u", "weight_v"))})
    torch.cuda.synchronize()
    return rec


def gpu(out):
    rec = {}
    for tag in GPU_TAGS:
        first, second = bridge_bits(tag), bridge_bits(tag)
        print(tag, first)
        if first != second:      # not bit-reproducible on this commit: no record for it
            print(tag, "NOT REPRODUCIBLE, dropped; differing keys:", [k for k in first if first[k] != second[k]])
            continue
        rec[tag] = first
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print("->", out)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if what == "launches":
        launches(out or os.path.join(GOLDEN, "dfamily_parent_launches.json"))
    elif what == "gpu":
        gpu(out or os.path.join(GOLDEN, "dfamily_bridge_parent_gpu.json"))
    else:
        sys.exit(__doc__)
