"""TEST INFRASTRUCTURE: the float64 statement of PatchNCE with negatives from the whole minibatch (gan_patchnce_all_*, include/mi355x_gan.h),
independent of tests/emulator.py and tests/emulator_nce_all.py.  Inputs are the stored buffers (bf16 or fp32 values widened exactly); every
step below is float64.  The gather, the normalisation and the scatter are the per-image statement's (tests/nce_ref64.py).

    queries     Tn, the Q = B P normalised target rows, row b P + i
    keys        S segments of Q rows: segment `self` = Sn, the call's own normalised source rows; the others are given (already normalised)
    logits      raw = (Tn . Keys^T) / T,  lg = clamp(raw, -50, 50)  (a NaN stays a NaN)
    row loss    rowloss_i = lse_i - lg_{i, self Q + i},  lse_i = log sum_j exp(lg_ij) over all K = S Q keys
    call        call = mean_i rowloss_i;  flag = isfinite(call);  loss += weight (flag ? call : 0)
    gradient    dlg_ij = weight flag (softmax_ij - [j = self Q + i]) / Q,  zero where raw is outside [-50, 50];  dTn = dlg . Keys / T
                dX_i = (dTn_i - Tn_i <Tn_i, dTn_i>) / ||x_i||   where ||x_i|| > eps,   dTn_i / eps   otherwise
                with flag 0 every row is exactly 0 and gtgt is not touched

`Ref` holds the switches of the deliberately wrong statements tests/nce_all_cases.py holds the kernels to.
"""
import torch

from tests import nce_ref64 as R0

EPS, CLAMP = R0.EPS, R0.CLAMP
gather64, scatter64 = R0.gather64, R0.scatter64


class Ref:
    pos_at_i = False          # the positive taken at column i instead of self Q + i
    div_P = False             # division by P instead of Q
    per_image = False         # the mean per image with a per-image flag
    own_segment = False       # the keys restricted to the own segment
    no_mask = False           # the clamp passes gradient
    no_invT_grad = False      # 1/T missing from the gradient
    loss_overwrite = False    # the += on the loss turned into an overwrite


def keys64(Sn, foreign, self_seg):
    """Sn: (Q, C) own normalised rows; foreign: list of the S - 1 other segments (Q, C) in segment order -> (S Q, C)"""
    segs = list(foreign)
    segs.insert(self_seg, Sn)
    return torch.cat(segs, 0)


def forward64(s, t, T, foreign=(), self_seg=0, ref=None):
    """s, t: (B, P, C) float64 sampled source / target rows; T: the temperature as the kernels hold it.  Intermediates by name."""
    ref = ref or Ref()
    B, P, C = s.shape
    Q = B * P
    Sn, _, _ = R0.normalise64(s)
    Tn, tn_true, tnorm = R0.normalise64(t)
    Sn, Tn, tn_true, tnorm = Sn.reshape(Q, C), Tn.reshape(Q, C), tn_true.reshape(Q), tnorm.reshape(Q)
    if ref.own_segment:
        foreign, self_seg = (), 0
    keys = keys64(Sn, foreign, self_seg)
    raw = Tn @ keys.t() / T
    lg = torch.where(torch.isnan(raw), raw, raw.clamp(-CLAMP, CLAMP))
    mx = torch.where(torch.isnan(lg), torch.full_like(lg, -float("inf")), lg).max(1, keepdim=True).values
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    lse = (mx + torch.log(torch.exp(lg - mx).sum(1, keepdim=True))).squeeze(1)
    pos = torch.arange(Q) + (0 if ref.pos_at_i else self_seg * Q)
    rowloss = lse - lg[torch.arange(Q), pos]
    call = rowloss.mean()
    per = rowloss.view(B, P).mean(1)
    flag_b = torch.isfinite(per) if ref.per_image else torch.isfinite(call).expand(B)
    return dict(Sn=Sn, Tn=Tn, tnorm=tnorm, tnorm_true=tn_true, keys=keys, raw=raw, lg=lg, mx=mx.squeeze(1), lse=lse, pos=pos, rowloss=rowloss, call=call,
                per=per, flag=bool(torch.isfinite(call)), flag_b=flag_b, B=B, P=P)


def loss64(fw, weight, ref=None):
    """what the call adds to *loss"""
    ref = ref or Ref()
    if ref.per_image:
        return weight * torch.where(fw["flag_b"], fw["per"], torch.zeros_like(fw["per"])).sum() / fw["B"]
    return weight * (fw["call"] if fw["flag"] else torch.zeros((), dtype=torch.float64))


def backward64(fw, T, weight, ref=None):
    """closed form: (dlg, dTn, dX), dX (Q, C); with flag 0 (per image under Ref.per_image) the rows are exactly 0"""
    ref = ref or Ref()
    B, P = fw["B"], fw["P"]
    Q, K = fw["raw"].shape
    C = fw["Tn"].shape[1]
    live = fw["flag_b"].repeat_interleave(P).view(Q, 1)
    if not bool(live.any()):
        return torch.zeros(Q, K, dtype=torch.float64), torch.zeros(Q, C, dtype=torch.float64), torch.zeros(Q, C, dtype=torch.float64)
    soft = torch.exp(fw["lg"] - fw["lse"].unsqueeze(1))
    onehot = torch.zeros(Q, K, dtype=torch.float64)
    onehot[torch.arange(Q), fw["pos"]] = 1.0
    dlg = (soft - onehot) * (weight / (P if ref.div_P else Q))
    if not ref.no_mask:
        dlg = torch.where((fw["raw"] < -CLAMP) | (fw["raw"] > CLAMP), torch.zeros_like(dlg), dlg)
    dlg = torch.where(live, dlg, torch.zeros_like(dlg)).nan_to_num(0.0) if not bool(live.all()) else dlg
    keys = fw["keys"] if bool(live.all()) else fw["keys"].nan_to_num(0.0)
    Tn = fw["Tn"] if bool(live.all()) else torch.where(live, fw["Tn"], torch.zeros_like(fw["Tn"]))
    dTn = dlg @ keys / (1.0 if ref.no_invT_grad else T)
    dot = (Tn * dTn).sum(1, keepdim=True)
    nrm = fw["tnorm"].unsqueeze(1)
    dX = torch.where(nrm > EPS, (dTn - Tn * dot) / nrm, dTn / nrm)
    dX = torch.where(live, dX, torch.zeros_like(dX))
    return dlg, dTn, dX


def loss_autograd64(s, t, T, weight, foreign=(), self_seg=0):
    """the forward statement written with differentiable torch ops only (for the autograd check of `backward64`)"""
    B, P, C = s.shape
    Q = B * P
    sn = (s / torch.linalg.vector_norm(s, dim=2, keepdim=True).clamp_min(EPS)).reshape(Q, C)
    tn = (t / torch.linalg.vector_norm(t, dim=2, keepdim=True).clamp_min(EPS)).reshape(Q, C)
    lg = (tn @ keys64(sn, foreign, self_seg).t() / T).clamp(-CLAMP, CLAMP)
    rowloss = torch.logsumexp(lg, 1) - lg[torch.arange(Q), torch.arange(Q) + self_seg * Q]
    return weight * rowloss.mean()
