"""TEST INFRASTRUCTURE: the feature-matching term (include/mi355x_gan.h "feature matching") stated in float64, the header's fp32
statement of its gradient, the header's accumulation structure (chain length, error bound), and a functional torch restatement of the CUT
discriminator's intermediate features (conv2d, leaky_relu, avg_pool2d: GAN_Variant1/models/discriminator_patchgan.py:65-72, 118-128),
written afresh: nothing here imports the product package."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
ACT_NONE, ACT_LRELU = 0, 2


# ------------------------------------------------------------------------------------------------ the kernel's statement
def layer_loss(f, r):
    """mean over every element of |f - r| in float64"""
    return (f.double() - r.double()).abs().mean()


def chain(B, H, W, C, fp32):
    """L of the header: the longest fp32 chain of one lane -- N * ceil(items / (256 nblocks)), items = B H W ceil(C / N),
    nblocks = min(2048, ceil(items / 256))"""
    N = 4 if fp32 else 8
    items = B * H * W * ((C + N - 1) // N)
    nblocks = min(2048, max(1, (items + 255) // 256))
    return N * ((items + 256 * nblocks - 1) // (256 * nblocks))


def loss_bound(L, term, after):
    """the header's bound on one call's `+=`: (L + 1) 2^-24 term + 2^-24 |slot after|"""
    return (L + 1) * U * abs(term) + U * abs(after)


def grad32(f, r, grad_scale, act, g_old=None):
    """the header's fp32 statement: f, r (..., C) float32 tensors of the stored values -> what the call writes (g_old None: accumulate = 0),
    float32 before the rounding to the view's dtype"""
    n = f.numel()
    inv = np.float32(grad_scale) / np.float32(n)
    inv02 = np.float32(0.2) * inv
    d = f - r
    m = torch.full_like(f, float(inv))
    if act == ACT_LRELU:
        m = torch.where(f > 0, m, torch.full_like(f, float(inv02)))
    v = torch.where(d > 0, m, torch.where(d < 0, -m, torch.zeros_like(m)))
    return v if g_old is None else g_old.float() + v


# ------------------------------------------------------------------------------------------------ the term
def fm(fake_feats, real_feats):
    """(1/K) sum_s (1/L) sum_j mean |F_sj(fake) - F_sj(real)| over nested lists [scale][layer] of tensors, in the dtype of the tensors"""
    assert len(fake_feats) == len(real_feats)
    total = 0.0
    for fs, rs in zip(fake_feats, real_feats):
        assert len(fs) == len(rs)
        total = total + sum((a - b.detach()).abs().mean() for a, b in zip(fs, rs)) / len(fs)
    return total / len(fake_feats)


def sn_weight(w_orig, u, v, power_iteration, eps=1e-12):
    """torch.nn.utils.spectral_norm's weight: optionally one power iteration from (u, v), then w_orig / (u^T W v) -> (weight, u, v)"""
    m = w_orig.reshape(w_orig.shape[0], -1)
    if power_iteration:
        v = F.normalize(torch.mv(m.t(), u), dim=0, eps=eps).detach()
        u = F.normalize(torch.mv(m, v), dim=0, eps=eps).detach()
    return w_orig / torch.dot(u, torch.mv(m, v)), u, v


def features(x, params, num_scales, n_layers, buffers=None, power_iteration=False):
    """the nested list get_intermediate_features returns: per scale every LeakyReLU output (n_layers + 1 of them; the logits are no feature),
    scale s on x average-pooled s times.  params: the discriminator's state_dict keys (weight or weight_orig, bias), any dtype;
    buffers: weight_u / weight_v for a spectral-norm discriminator."""
    out = []
    for s in range(num_scales):
        h, feats = x, []
        for i in range(n_layers + 1):
            k = f"discriminators.{s}.model.{2 * i}"
            w = params.get(k + ".weight")
            if w is None:
                w, _, _ = sn_weight(params[k + ".weight_orig"], buffers[k + ".weight_u"].to(x.dtype), buffers[k + ".weight_v"].to(x.dtype), power_iteration)
            h = F.leaky_relu(F.conv2d(h, w, params[k + ".bias"], stride=2 if i < n_layers else 1, padding=1), 0.2)
            feats.append(h)
        out.append(feats)
        x = F.avg_pool2d(x, 3, 2, 1, count_include_pad=False)
    return out
