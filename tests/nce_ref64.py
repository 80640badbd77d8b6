"""TEST INFRASTRUCTURE: the float64 statement of PatchNCE for one feature layer (csrc/patchnce.hip; the reference's
PatchNCELoss._compute_nce_loss), independent of tests/emulator.py.  Inputs are the stored buffers (bf16 or fp32 values widened exactly);
every step below is float64.

    gather      row i of image b = feat[b, id // W, id % W, :C]                      (ids shared by the batch and by source / target)
    normalise   n = x / max(||x||, eps),  eps = the float 1e-6f
    logits      raw = (Tn . Sn^T) / T,  lg = clamp(raw, -50, 50)  (a NaN stays a NaN)
    row loss    rowloss_i = lse_i - lg_ii,  lse_i = log sum_j exp(lg_ij)
    image       per_b = mean_i rowloss;  flag_b = isfinite(per_b);  an image with flag 0 counts as the constant 0
    loss        += weight * sum_b flag_b per_b / B
    gradient    dlg_ij = weight flag_b (softmax_ij - [i = j]) / (P B),  zero where raw is outside [-50, 50];  dTn = dlg . Sn / T
                dX_i = (dTn_i - Tn_i <Tn_i, dTn_i>) / ||x_i||   where ||x_i|| > eps,   dTn_i / eps   otherwise
                rows of a flag-0 image are exactly 0 and its part of gtgt is not touched
    scatter     gtgt[b, id // W, id % W, :C] += dX_i, duplicates accumulating; channels >= C and halos are never written

`Ref` holds the switches of the deliberately wrong statements tests/nce_cases.py holds the kernels to.
"""
import numpy as np
import torch

EPS = float(np.float32(1e-6))       # the kernels' 1e-6f, widened
CLAMP = 50.0


class Ref:
    no_mask = False            # the clamp passes gradient everywhere
    eps = EPS
    dup_overwrite = False      # duplicates overwrite instead of accumulating
    no_B = False               # division by P without B
    no_invT_grad = False       # 1/T missing from the gradient
    div_H = False              # id // H instead of id // W
    no_projection = False      # Jacobian of the normalisation without the projection term
    count_nonfinite = False    # a non-finite image counted in the loss
    view_channels = False      # channels :viewC instead of :C
    loss_overwrite = False     # the += on the loss turned into an overwrite


def positions(ids, H, W, ref=None):
    ids = ids.long()
    if ref is not None and ref.div_H:
        return (ids // H).clamp_max(H - 1), ids % W
    return ids // W, ids % W


def gather64(v, ids, C, ref=None):
    """v: (B, H, W, Cv) float64 interior -> (B, P, C) sampled rows"""
    B, H, W, Cv = v.shape
    ys, xs = positions(ids, H, W, ref)
    return v[:, ys, xs, :(Cv if ref is not None and ref.view_channels else C)]


def normalise64(x, eps=EPS):
    nrm = torch.sqrt((x * x).sum(2, keepdim=True))
    den = torch.where(nrm > eps, nrm, torch.full_like(nrm, eps))        # max(|x|, eps) with a NaN norm falling to eps, as fmaxf does
    return x / den, nrm.squeeze(2), den.squeeze(2)


def forward64(s, t, T, ref=None):
    """s, t: (B, P, C) float64 sampled source / target rows; T: the temperature as the kernels hold it (a float).  Returns the
    intermediates by name."""
    ref = ref or Ref()
    Sn, _, _ = normalise64(s, ref.eps)
    Tn, tn_true, tnorm = normalise64(t, ref.eps)
    raw = torch.bmm(Tn, Sn.transpose(1, 2)) / T
    lg = torch.where(torch.isnan(raw), raw, raw.clamp(-CLAMP, CLAMP))
    mx = torch.where(torch.isnan(lg), torch.full_like(lg, -float("inf")), lg).max(2, keepdim=True).values
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    lse = (mx + torch.log(torch.exp(lg - mx).sum(2, keepdim=True))).squeeze(2)
    rowloss = lse - torch.diagonal(lg, dim1=1, dim2=2)
    per = rowloss.mean(1)
    flag = torch.isfinite(per)
    return dict(Sn=Sn, Tn=Tn, tnorm=tnorm, tnorm_true=tn_true, raw=raw, lg=lg, lse=lse, rowloss=rowloss, per=per, flag=flag)


def loss64(fw, weight, ref=None):
    """what the call adds to *loss"""
    ref = ref or Ref()
    per = fw["per"] if ref.count_nonfinite else torch.where(fw["flag"], fw["per"], torch.zeros_like(fw["per"]))
    return weight * per.sum() / (1 if ref.no_B else per.numel())


def backward64(fw, T, weight, ref=None):
    """closed form: (dlg, dTn, dX), each float64; rows of a flag-0 image exactly 0"""
    ref = ref or Ref()
    Sn, Tn, raw, lg, lse = fw["Sn"], fw["Tn"], fw["raw"], fw["lg"], fw["lse"]
    B, P, _ = Sn.shape
    soft = torch.exp(lg - lse.unsqueeze(2))
    dlg = (soft - torch.eye(P, dtype=torch.float64).unsqueeze(0)) * (weight / (P * (1 if ref.no_B else B)))
    if not ref.no_mask:
        dlg = torch.where((raw < -CLAMP) | (raw > CLAMP), torch.zeros_like(dlg), dlg)
    live = fw["flag"].view(B, 1, 1)
    dlg = torch.where(live, dlg, torch.zeros_like(dlg))
    Sn0 = torch.where(live, Sn, torch.zeros_like(Sn))
    Tn0 = torch.where(live, Tn, torch.zeros_like(Tn))
    dTn = torch.bmm(dlg, Sn0) / (1.0 if ref.no_invT_grad else T)
    dot = (Tn0 * dTn).sum(2, keepdim=True)
    nrm = fw["tnorm"].unsqueeze(2)
    proj = dTn if ref.no_projection else dTn - Tn0 * dot
    dX = torch.where(nrm > ref.eps, proj / nrm, dTn / nrm)
    dX = torch.where(live, dX, torch.zeros_like(dX))
    return dlg, dTn, dX


def scatter64(prior, dX, ids, C, flag, ref=None):
    """prior: (B, H, W, Cg) float64 interior of gtgt before the call -> the exact (unrounded) result, the per-pixel count of rows added and
    the per-element sum of |terms| (for the tolerance)"""
    ref = ref or Ref()
    B, H, W, Cg = prior.shape
    ys, xs = positions(ids, H, W, ref)
    out, mag = prior.clone(), prior.abs()
    n = torch.zeros(H, W, dtype=torch.int64)
    for i in range(ids.numel()):
        y, x = int(ys[i]), int(xs[i])
        if ref.dup_overwrite:
            out[:, y, x, :C] = prior[:, y, x, :C] + dX[:, i, :C]
            mag[:, y, x, :C] = prior[:, y, x, :C].abs() + dX[:, i, :C].abs()
        else:
            out[:, y, x, :C] += dX[:, i, :C]
            mag[:, y, x, :C] += dX[:, i, :C].abs()
        n[y, x] += 1
    dead = ~flag
    out[dead], mag[dead] = prior[dead], prior[dead].abs()
    return out, n, mag


def loss_autograd64(s, t, T, weight, eps=EPS):
    """the forward statement written with differentiable torch ops only (for the autograd check of `backward64`)"""
    sn = s / torch.linalg.vector_norm(s, dim=2, keepdim=True).clamp_min(eps)       # vector_norm: subgradient 0 at a zero row
    tn = t / torch.linalg.vector_norm(t, dim=2, keepdim=True).clamp_min(eps)
    lg = (torch.bmm(tn, sn.transpose(1, 2)) / T).clamp(-CLAMP, CLAMP)
    B, P, _ = lg.shape
    rowloss = torch.logsumexp(lg, 2) - torch.diagonal(lg, dim1=1, dim2=2)
    return weight * rowloss.mean(1).sum() / B
