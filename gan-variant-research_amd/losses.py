"""The reference's loss / augmentation callables on the HIP kernels, as ordinary differentiable PyTorch functions.

Same names, signatures and RNG consumption as GAN_Variant1/losses/{adv_hinge,patchnce_cut,identity_l1}.py,
GAN_Variant1/training/diffaugment.py and Basic_GAN/src/losses.py, so a script written against the reference imports them from
here unchanged.  Each call is one autograd node whose forward launches the fused HIP kernel (value and input gradient come out
of the same pass) on NCHW fp32 tensors; the fused trainers (cut.py / basic.py) use the same kernels without the layout round
trip.  There is no CPU fallback: tensors must live on the GPU.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from . import autograd as AG
from ._lib import ACT_NONE, F32, HALO_NONE, HALO_ZERO
from .cut import DiffAugment as _DiffAugmentSampler
from .runtime import Program, cached_plan, cpad

_PLANS: Dict[tuple, object] = {}


class _Plan:
    """Persistent staging tensors + prebuilt launches for one (op, shape, device): ops hold raw pointers, so nothing per call."""

    def __init__(self, device):
        self.ctx = AG._new_ctx(device, F32)
        self.ops = self.ctx.ops
        self.device = device


# ------------------------------------------------------------------------------------------------ patch losses (a9)
class _PatchLossPlan(_Plan):
    def __init__(self, shape, device, mode, target):
        super().__init__(device)
        B, C, H, W = shape
        assert C == 1, "PatchGAN logits are (B,1,h,w)"
        self.x = torch.zeros(shape, dtype=torch.float32, device=device)
        self.g = torch.zeros(shape, dtype=torch.float32, device=device)
        self.loss = self.ctx.f32(1)
        v, gv = self.ctx.view(B, H, W, cpad(1), 0), self.ctx.view(B, H, W, cpad(1), 0)
        self.prog = Program("patch_loss")
        self.prog.add(self.ops.nchw_to_view(self.x, 1, v, HALO_NONE))
        self.prog.add(self.ops.patch_loss(v, mode, float(target), 1.0, self.loss, gv))
        self.prog.add(self.ops.view_to_nchw(gv, 1, self.g))


class _PatchLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode, target):
        p = cached_plan(_PLANS, ("patch_loss", tuple(x.shape), x.device, mode, float(target)), x.device, lambda: _PatchLossPlan(tuple(x.shape), x.device, mode, target))
        p.x.copy_(x)
        p.prog.run()
        ctx.save_for_backward(p.g.clone())
        return p.loss.clone().reshape(())

    @staticmethod
    def backward(ctx, g):
        return ctx.saved_tensors[0] * g, None, None


def _patch_loss(x: torch.Tensor, mode: int, target: float = 0.0) -> torch.Tensor:
    return _PatchLossFn.apply(x.float().contiguous(), mode, target)


def _as_list(p):
    return list(p) if isinstance(p, (list, tuple)) else [p]


def discriminator_hinge_loss(real_preds, fake_preds):
    """adv_hinge.py:6-36: mean over scales of 0.5 * (mean(relu(1 - real)) + mean(relu(1 + fake)))."""
    real_preds, fake_preds = _as_list(real_preds), _as_list(fake_preds)
    loss = 0.0
    for r, f in zip(real_preds, fake_preds):
        loss = loss + (_patch_loss(r, 0) + _patch_loss(f, 1)) * 0.5
    return loss / len(real_preds)


def generator_hinge_loss(fake_preds):
    """adv_hinge.py:39-62: mean over scales of -mean(fake)."""
    fake_preds = _as_list(fake_preds)
    loss = 0.0
    for f in fake_preds:
        loss = loss + _patch_loss(f, 2)
    return loss / len(fake_preds)


class GANLoss:
    """Basic_GAN/src/losses.py:5-22: 'lsgan' -> MSE against {1,0}; 'bce' -> BCE-with-logits."""

    def __init__(self, mode: str = "lsgan"):
        assert mode in ("lsgan", "bce")
        self.mode = mode

    def __call__(self, pred: torch.Tensor, is_real: bool) -> torch.Tensor:
        return _patch_loss(pred, 3 if self.mode == "lsgan" else 4, 1.0 if is_real else 0.0)


# ------------------------------------------------------------------------------------------------ L1 (a9)
class _L1Plan(_Plan):
    def __init__(self, shape, device):
        super().__init__(device)
        B, C, H, W = shape
        self.x = torch.zeros(shape, dtype=torch.float32, device=device)
        self.t = torch.zeros(shape, dtype=torch.float32, device=device)
        self.g = torch.zeros(shape, dtype=torch.float32, device=device)
        self.loss = self.ctx.f32(1)
        v, gv = self.ctx.view(B, H, W, cpad(C), 0), self.ctx.view(B, H, W, cpad(C), 0)
        self.prog = Program("l1")
        self.prog.add(self.ops.nchw_to_view(self.x, C, v, HALO_NONE))
        self.prog.add(self.ops.l1_loss(v, C, self.t, 1.0, None, self.loss, gv, self.ctx.scratch("l1_ws", 1024)))
        self.prog.add(self.ops.view_to_nchw(gv, C, self.g))


class _L1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target):
        p = cached_plan(_PLANS, ("l1", tuple(x.shape), x.device), x.device, lambda: _L1Plan(tuple(x.shape), x.device))
        p.x.copy_(x); p.t.copy_(target)
        p.prog.run()
        ctx.save_for_backward(p.g.clone())
        return p.loss.clone().reshape(())

    @staticmethod
    def backward(ctx, g):
        d = ctx.saved_tensors[0] * g
        return d, (-d if ctx.needs_input_grad[1] else None)


def l1_loss(x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """mean |x - target| (Basic_GAN/src/losses.py:24-30 cycle_loss / identity_loss bodies)."""
    return _L1Fn.apply(x.float().contiguous(), target.float().contiguous())


def identity_loss(generator, monet_images):
    """identity_l1.py:6-22: mean |G(monet) - monet| in fp32."""
    return l1_loss(generator(monet_images.float()), monet_images)


def cycle_loss(rec, real, lambda_cycle: float = 10.0):
    """Basic_GAN/src/losses.py:24-26."""
    return lambda_cycle * l1_loss(rec, real)


# ------------------------------------------------------------------------------------------------ feature matching
class _FeatmatchPlan(_Plan):
    """gan_featmatch for one feature shape: mean |fake - real| and its gradient wrt fake (act = none), through NCHW staging tensors."""

    def __init__(self, shape, device):
        super().__init__(device)
        B, C, H, W = shape
        self.f = torch.zeros(shape, dtype=torch.float32, device=device)
        self.r = torch.zeros(shape, dtype=torch.float32, device=device)
        self.g = torch.zeros(shape, dtype=torch.float32, device=device)
        self.loss = self.ctx.f32(1)
        ops, ctx = self.ops, self.ctx
        vf, vr, gv = ctx.view(B, H, W, cpad(C), 0), ctx.view(B, H, W, cpad(C), 0), ctx.view(B, H, W, cpad(C), 0)
        self.prog = Program("featmatch")
        self.prog.add(ops.nchw_to_view(self.f, C, vf, HALO_NONE))
        self.prog.add(ops.nchw_to_view(self.r, C, vr, HALO_NONE))
        self.prog.add(ops.fill(self.loss, 0.0))
        self.prog.add(ops.featmatch(vf, vr, C, 1.0, self.loss, 1.0, ACT_NONE, gv, False, ctx.f32(ops.featmatch_ws_floats(vf))))
        self.prog.add(ops.view_to_nchw(gv, C, self.g))


class _FeatmatchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fake, real):
        p = cached_plan(_PLANS, ("featmatch", tuple(fake.shape), fake.device), fake.device, lambda: _FeatmatchPlan(tuple(fake.shape), fake.device))
        p.f.copy_(fake); p.r.copy_(real)
        p.prog.run()
        ctx.save_for_backward(p.g.clone())
        return p.loss.clone().reshape(())

    @staticmethod
    def backward(ctx, g):
        return ctx.saved_tensors[0] * g, None


def _flat_feats(feats) -> list:
    return [t for f in feats for t in (_flat_feats(f) if isinstance(f, (list, tuple)) else [f])]


def feature_matching_loss(real_feats, fake_feats):
    """The name the reference's trainer imported from losses/feat_matching.py (a file it no longer has; the formula is this project's,
    DESIGN 3.11): over MultiscaleDiscriminator.get_intermediate_features' nested lists [scale][layer], or flat lists, of NCHW tensors,
    mean over scales of mean over a scale's layers of mean |fake - real.detach()|.  Gradient with respect to fake_feats only."""
    nested = bool(real_feats) and isinstance(real_feats[0], (list, tuple))
    groups_r = [list(g) for g in real_feats] if nested else [list(real_feats)]
    groups_f = [list(g) for g in fake_feats] if nested else [list(fake_feats)]
    assert len(groups_r) == len(groups_f) and groups_r, "feature_matching_loss: the two feature lists differ in structure"
    total = 0.0
    for gr, gf in zip(groups_r, groups_f):
        assert len(gr) == len(gf) and gr, "feature_matching_loss: the two feature lists differ in structure"
        layer_sum = 0.0
        for r, f in zip(gr, gf):
            assert r.shape == f.shape and f.dim() == 4, "feature_matching_loss: features are (B, C, h, w) tensors of equal shape"
            layer_sum = layer_sum + _FeatmatchFn.apply(f.float().contiguous(), r.detach().float().contiguous())
        total = total + layer_sum / len(gr)
    return total / len(groups_r)


# ------------------------------------------------------------------------------------------------ PatchNCE (a8)
class _NcePlan(_Plan):
    def __init__(self, shape, device, P, temperature, all_negatives=False):
        super().__init__(device)
        B, C, H, W = shape
        self.src = torch.zeros(shape, dtype=torch.float32, device=device)
        self.tgt = torch.zeros(shape, dtype=torch.float32, device=device)
        self.g = torch.zeros(shape, dtype=torch.float32, device=device)
        self.ids = torch.zeros(P, dtype=torch.int32, device=device)
        self.loss = self.ctx.f32(1)
        ops, ctx = self.ops, self.ctx
        vs, vt, gv = ctx.view(B, H, W, cpad(C), 0), ctx.view(B, H, W, cpad(C), 0), ctx.view(B, H, W, cpad(C), 0)
        ws = ctx.f32(ops.patchnce_ws_floats(B, P, C))
        self.fwd = Program("patchnce.fwd")
        self.fwd.add(ops.nchw_to_view(self.src, C, vs, HALO_NONE))
        self.fwd.add(ops.nchw_to_view(self.tgt, C, vt, HALO_NONE))
        self.fwd.add(ops.fill(self.loss, 0.0))
        if all_negatives:                                    # one process: the keys are the workspace's own normalised source rows
            self.fwd.add(ops.patchnce_all_gather(vs, vt, self.ids, P, C, ws))
            self.fwd.add(ops.patchnce_all_fwd(vt, P, C, temperature, 1.0, ws, 1, 0, 0, self.loss, ws))
        else:
            self.fwd.add(ops.patchnce_fwd(vs, vt, self.ids, P, C, temperature, 1.0, self.loss, ws))
        self.fwd.add(ops.zero_(gv.t))                       # the backward kernel ADDS into the feature gradient
        if all_negatives:
            self.fwd.add(ops.patchnce_all_bwd(vt, self.ids, P, C, temperature, 1.0, ws, 1, 0, 0, gv, ws))
        else:
            self.fwd.add(ops.patchnce_bwd(vt, self.ids, P, C, temperature, 1.0, gv, ws))
        self.fwd.add(ops.view_to_nchw(gv, C, self.g))


class PatchNCELoss(nn.Module):
    """patchnce_cut.py:7-110.  One patch-id draw per layer (`torch.randint(0, H*W, (num_patches,), device=...)`, :63) shared by
    the batch and by source / target; the source features carry no gradient (compute_patchnce_loss detaches them).
    all_negatives (patchnce.nce_includes_all_negatives_from_minibatch; this project's statement, include/mi355x_gan.h): every target row is
    scored against the source rows of the whole batch, not of its own image only."""

    def __init__(self, temperature: float = 0.07, num_patches: int = 256, nce_layers: Sequence[int] = (0, 4, 8, 12, 16), *,
                 all_negatives: bool = False):
        super().__init__()
        self.temperature, self.num_patches, self.nce_layers = temperature, num_patches, list(nce_layers)
        self.all_negatives = bool(all_negatives)

    def _compute_nce_loss(self, src_feat, tgt_feat, patch_ids: Optional[torch.Tensor] = None):
        B, C, H, W = tgt_feat.shape
        if patch_ids is None:
            patch_ids = torch.randint(0, H * W, (self.num_patches,), device=tgt_feat.device)
        from . import ops_library  # noqa: F401  (registers torch.ops.mi355x_gan.*)
        op = torch.ops.mi355x_gan.patchnce_all_fwd if self.all_negatives else torch.ops.mi355x_gan.patchnce_fwd
        loss, _ = op(src_feat.detach(), tgt_feat, patch_ids.to(torch.int32), self.temperature)
        return loss

    def forward(self, src_feats, tgt_feats, patch_ids: Optional[List[torch.Tensor]] = None):
        total = 0.0
        for i, (s, t) in enumerate(zip(src_feats, tgt_feats)):
            total = total + self._compute_nce_loss(s, t, None if patch_ids is None else patch_ids[i])
        return total / len(src_feats)


def compute_patchnce_loss(generator, src_images, tgt_images, nce_layers, temperature=0.07, num_patches=256, *, all_negatives=False):
    """patchnce_cut.py:113-149."""
    fn = PatchNCELoss(temperature, num_patches, nce_layers, all_negatives=all_negatives)
    with torch.no_grad():
        src_feats = generator.get_feature_layers(src_images, nce_layers)
    src_feats = [f.detach() for f in src_feats]
    tgt_feats = generator.get_feature_layers(tgt_images, nce_layers)
    return fn(src_feats, tgt_feats)


# ------------------------------------------------------------------------------------------------ palette prior
class _PalettePlan(_Plan):
    """Statistics, batch mean / prior update and loss + image gradient of csrc/palette.hip for one (shape, T, EMA setting)."""

    def __init__(self, shape, device, T, use_ema, decay):
        super().__init__(device)
        B, C, H, W = shape
        assert C == 3, "the palette prior reads RGB images (B,3,H,W)"
        ops, ctx = self.ops, self.ctx
        self.x = torch.zeros(shape, dtype=torch.float32, device=device)
        self.g = torch.zeros(shape, dtype=torch.float32, device=device)
        v, gv = ctx.view(B, H, W, 8, 0), ctx.view(B, H, W, 8, 0)
        cells = ctx.f32(B * T * T * 3)
        self.stats, gstats, batch = ctx.f32(B * 6), ctx.f32(B * 6), ctx.f32(8)
        self.prior, self.loss = ctx.f32(8), ctx.f32(1)
        self.steps = torch.zeros(1, dtype=torch.int32, device=device)
        self.fwd = Program("palette.stats")
        self.fwd.add(ops.nchw_to_view(self.x, 3, v, HALO_NONE))
        self.fwd.add(ops.palette_stats(v, T, cells, self.stats))
        self.update = Program("palette.prior")                       # after fwd on the Monet batch
        self.update.add(ops.palette_batch_mean(self.stats, B, batch))
        self.update.add(ops.palette_prior_update(batch, 1.0, self.prior, self.steps, use_ema, decay))
        self.lossbwd = Program("palette.loss")                       # after fwd on the fake batch
        self.lossbwd.add(ops.palette_loss(self.stats, self.prior, B, 1.0, self.loss, gstats))
        self.lossbwd.add(ops.palette_bwd(v, T, cells, self.stats, gstats, 1.0, gv, False))
        self.lossbwd.add(ops.view_to_nchw(gv, 3, self.g))


def _palette_plan(shape, device, T, use_ema=True, decay=0.99) -> _PalettePlan:
    from .runtime import check_palette_size
    check_palette_size(T)
    key = ("palette", tuple(shape), device, int(T), bool(use_ema), float(decay))
    return cached_plan(_PLANS, key, device, lambda: _PalettePlan(tuple(shape), device, int(T), bool(use_ema), float(decay)))


def low_freq_lab_stats(images: torch.Tensor, target_size: int = 32):
    """get_low_freq_stats(rgb_to_lab(denormalize(images)), target_size) of GAN_Variant1/dataio/transforms.py:52-119 in one pass:
    (mean, std), each (B, 3), of the Lab image pooled to target_size x target_size.  Forward only."""
    from . import ops_library  # noqa: F401
    return torch.ops.mi355x_gan.palette_stats(images, int(target_size))


class PalettePriorLoss(nn.Module):
    """mean over images and channels of (|mean_fake - mean_prior| + |std_fake - std_prior|) / 100 on the low-frequency Lab statistics,
    against a prior that follows the Monet batches (`use_ema`: prior = decay * prior + (1 - decay) * batch, the first call sets it;
    otherwise prior = batch).  The statistic is the reference's (transforms.py:52-119); the reference's own loss file was deleted, so
    this formula is the project's.  forward(fake, monets) updates the prior, then returns the scalar with gradient to `fake`; the prior
    is a constant for the gradient.  `prior` is a (3, 2) buffer of (mean, std) per Lab channel, `steps` the number of updates."""

    def __init__(self, low_freq_size: int = 32, use_ema: bool = True, ema_decay: float = 0.99):
        super().__init__()
        from .runtime import check_palette_size
        check_palette_size(low_freq_size)
        self.low_freq_size, self.use_ema, self.ema_decay = int(low_freq_size), bool(use_ema), float(ema_decay)
        self.register_buffer("prior", torch.zeros(3, 2))
        self.register_buffer("steps", torch.zeros(1, dtype=torch.int32))

    @property
    def prior_mean(self):
        return self.prior[:, 0]

    @property
    def prior_std(self):
        return self.prior[:, 1]

    @torch.no_grad()
    def update_prior(self, monets: torch.Tensor):
        x = monets.detach().float().contiguous()
        if self.prior.device != x.device:
            self.to(x.device)
        p = _palette_plan(x.shape, x.device, self.low_freq_size, self.use_ema, self.ema_decay)
        p.x.copy_(x)
        p.prior[:6].copy_(self.prior.reshape(-1)); p.steps.copy_(self.steps)
        p.fwd.run()
        p.update.run()
        self.prior.copy_(p.prior[:6].view(3, 2)); self.steps.copy_(p.steps)

    def forward(self, fake: torch.Tensor, monets: torch.Tensor) -> torch.Tensor:
        self.update_prior(monets)
        from . import ops_library  # noqa: F401
        loss, _ = torch.ops.mi355x_gan.palette_prior_fwd(fake, self.prior.detach().clone(), self.low_freq_size)
        return loss


# ------------------------------------------------------------------------------------------------ DiffAugment (a11)
class _AugPlan(_Plan):
    def __init__(self, shape, device):
        super().__init__(device)
        B, C, H, W = shape
        self.x = torch.zeros(shape, dtype=torch.float32, device=device)
        self.y = torch.zeros(shape, dtype=torch.float32, device=device)
        self.gy = torch.zeros(shape, dtype=torch.float32, device=device)
        self.gx = torch.zeros(shape, dtype=torch.float32, device=device)
        self.prm = torch.zeros(B, 12, dtype=torch.float32, device=device)
        ops, ctx = self.ops, self.ctx
        vx, vy, vgy, vgx = (ctx.view(B, H, W, cpad(C), 0) for _ in range(4))
        ws = ctx.scratch("aug_ws", B + 16)
        self.fwd = Program("diffaug.fwd")
        self.fwd.add(ops.nchw_to_view(self.x, C, vx, HALO_NONE))
        self.fwd.add(ops.diffaug_fwd(vx, C, self.prm, vy, ws))
        self.fwd.add(ops.view_to_nchw(vy, C, self.y))
        self.bwd = Program("diffaug.bwd")
        self.bwd.add(ops.nchw_to_view(self.gy, C, vgy, HALO_NONE))
        self.bwd.add(ops.diffaug_bwd(vgy, C, self.prm, vgx, ws))
        self.bwd.add(ops.view_to_nchw(vgx, C, self.gx))


class DiffAugment(_DiffAugmentSampler):
    """training/diffaugment.py:76-106 as a differentiable callable: brightness, saturation, contrast, translation and cutout in
    one gather pass each way.  `generator` (optional) makes the per-sample draws reproducible; `last_draws` keeps them."""

    def __call__(self, x: torch.Tensor, generator: Optional[torch.Generator] = None, draws: Optional[dict] = None) -> torch.Tensor:
        B, C, H, W = x.shape
        self.last_draws = draws if draws is not None else self.sample(B, H, W, generator)
        prm = self.to_params(self.last_draws, B, H, W).to(x.device)
        from . import ops_library  # noqa: F401
        return torch.ops.mi355x_gan.diffaugment_fwd(x, prm)
