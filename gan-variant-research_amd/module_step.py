"""The reference's CUT `train_step` (GAN_Variant1/training/train_cutpp.py:206-331) written against the drop-in module API of this
package: differentiable HIP `generator` / `discriminator` modules (autograd.py), the reference-named losses (losses.py) and
training utilities (training.py).  Same signature, same order of operations, same returned keys, same NaN behaviour.

This is the compatibility path -- every forward the reference runs is run (five generator passes per step); the fused
`cut.CutTrainer` computes the same step with one shared `G(photos)` forward and is what `bench.py` measures.
`rnd` (optional, not in the reference's signature) injects the device-RNG draws of the step for parity tests:
{"aug_real", "aug_fake_d", "aug_fake_g": DiffAugment draws, "nce_ids": one id tensor per PatchNCE layer}.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from .cut import identity_weight_at
from .autograd import r1_regularization
from .losses import PalettePriorLoss, PatchNCELoss, discriminator_hinge_loss, feature_matching_loss, generator_hinge_loss, identity_loss

_PALETTE = {}      # id(generator) -> (generator, PalettePriorLoss): the prior of a run whose caller passes no module of its own


def palette_prior_for(generator, config) -> PalettePriorLoss:
    """The run's PalettePriorLoss, built from `palette_prior.*` (the shipped YAML's defaults when the block is absent)."""
    ent = _PALETTE.get(id(generator))
    if ent is None or ent[0] is not generator:
        pp = config.get("palette_prior") or {}
        ent = _PALETTE[id(generator)] = (generator, PalettePriorLoss(pp.get("low_freq_size", 32), pp.get("use_ema", True), pp.get("ema_decay", 0.99)))
    return ent[1]


def train_step(step, photos, monets, generator, discriminator, opt_G, opt_D, ema_G, amp_ctx, diffaugment, config, device, rnd: Optional[dict] = None,
               palette_prior: Optional[PalettePriorLoss] = None):
    """palette_prior (optional, not in the reference's signature): the module that holds the palette prior when `loss_weights.palette` > 0
    (default: one per generator, kept here).  The loss dict gains `palette` only then, as in cut.CutTrainer.
    loss_weights.featmatch > 0 adds cut.CutTrainer's feature-matching term: the discriminator's intermediate features of aug(fake) against
    those of aug(photos), detached, under the generator step's DiffAugment draws; the dict gains `featmatch` only then."""
    lw = config["loss_weights"]
    palette_w = float(lw.get("palette", 0) or 0)
    featmatch_w = float(lw.get("featmatch", 0) or 0)
    identity_weight = identity_weight_at(step, config)                                    # :224-228
    rnd = rnd or {}

    def aug(x, key):
        return x if diffaugment is None else diffaugment(x, draws=rnd.get(key))

    # ---- discriminator step (:231-254)
    opt_D.zero_grad()
    with amp_ctx.autocast():
        fake = generator(photos)
        real_pred = discriminator(aug(photos, "aug_real"))
        fake_pred = discriminator(aug(fake.detach(), "aug_fake_d"))
        d_loss = discriminator_hinge_loss(real_pred, fake_pred)
    amp_ctx.scale_backward(d_loss)
    amp_ctx.step_optimizer(opt_D, max_grad_norm=config.get("grad_clip_d", 10.0))
    # ---- lazy R1 (:257-263)
    r1_loss = torch.tensor(0.0, device=device)
    if config["r1"]["gamma"] > 0 and step % config["r1"]["every"] == 0:
        opt_D.zero_grad()
        r1_loss = r1_regularization(discriminator, photos, amp_ctx)
        amp_ctx.scale_backward(r1_loss * config["r1"]["gamma"] * config["r1"]["every"])
        amp_ctx.step_optimizer(opt_D, max_grad_norm=config.get("grad_clip_d", 10.0))
    # ---- generator step (:266-308)
    opt_G.zero_grad()
    with amp_ctx.autocast():
        fake = generator(photos)
        fake_aug = aug(fake, "aug_fake_g")
        fm_draws = None if diffaugment is None else diffaugment.last_draws      # the real branch is augmented with the SAME draws
        g_adv_loss = generator_hinge_loss(discriminator(fake_aug))
        nce_loss = torch.tensor(0.0, device=device)
        if lw["patchnce"] > 0:
            pn = config["patchnce"]
            fn = PatchNCELoss(pn["temperature"], pn["num_patches"], pn["nce_layers"],
                              all_negatives=bool(pn.get("nce_includes_all_negatives_from_minibatch", False)))
            with torch.no_grad():
                src_feats = generator.get_feature_layers(photos, pn["nce_layers"])
            tgt_feats = generator.get_feature_layers(fake, pn["nce_layers"])
            nce_loss = fn(src_feats, tgt_feats, rnd.get("nce_ids"))                           # compute_patchnce_loss, :113-149
        idt_loss = torch.tensor(0.0, device=device)
        if identity_weight > 0:
            idt_loss = identity_loss(generator, monets)
        g_loss = lw["adv"] * g_adv_loss + lw["patchnce"] * nce_loss + identity_weight * idt_loss
        if palette_w > 0:
            fn = palette_prior if palette_prior is not None else palette_prior_for(generator, config)
            palette_loss = fn(fake, monets)
            g_loss = g_loss + palette_w * palette_loss
        if featmatch_w > 0:
            # eval mode for both feature passes: with spectral norm the weights are those of discriminator(fake_aug) above, whose power
            # iteration was this generator step's only one
            was_training = discriminator.training
            discriminator.eval()
            try:
                with torch.no_grad():
                    real_feats = discriminator.get_intermediate_features(photos if diffaugment is None else diffaugment(photos, draws=fm_draws))
                featmatch_loss = feature_matching_loss(real_feats, discriminator.get_intermediate_features(fake_aug))
            finally:
                discriminator.train(was_training)
            g_loss = g_loss + featmatch_w * featmatch_loss
    amp_ctx.scale_backward(g_loss)
    amp_ctx.step_optimizer(opt_G, max_grad_norm=config.get("grad_clip_g", 10.0))
    if ema_G is not None:
        ema_G.update()
    losses = {"d_loss": d_loss.item(), "g_loss": g_loss.item(), "g_adv": g_adv_loss.item(), "nce": nce_loss.item(), "identity": idt_loss.item(),
              "r1": r1_loss.item(), "identity_weight": identity_weight}
    if palette_w > 0:
        losses["palette"] = palette_loss.item()
    if featmatch_w > 0:
        losses["featmatch"] = featmatch_loss.item()
    if any(not math.isfinite(v) for k, v in losses.items() if k != "identity_weight"):
        raise ValueError(f"NaN loss detected at step {step}. Training stopped to prevent corruption.")   # :325-329
    return losses
