"""The InstanceNorm kernel family without a GPU: the float64 statements of tests/norm_ref64.py against float64 autograd, the regimes the
cases of tests/norm_cases.py name, the emulator's statements and an fp32 model of per-lane strided summation inside the derived bounds
(which therefore do not reject an honest fp32 implementation), and every deliberately wrong reference outside them (so they do reject
the mistakes they are meant for).  tests/test_norm_family_gpu.py runs the same bodies on the HIP kernels."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd.runtime import Ctx
from tests import norm_cases as N
from tests import norm_ref64 as R
from tests.emulator import EmuOps

TOL = dict(rtol=1e-12, atol=1e-12)


def make():
    return Ctx(EmuOps(), "cpu", BF16)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def act_torch(v, act):
    return {R.ACT_NONE: lambda t: t, R.ACT_RELU: torch.relu, R.ACT_LRELU: lambda t: F.leaky_relu(t, 0.2), R.ACT_TANH: torch.tanh}[act](v)


# ---------------------------------------------------------------------------------------------- the references against autograd
@pytest.mark.parametrize("act", N.ACTS_ALL)
def test_forward_and_backward_statements_equal_float64_autograd(act):
    g = torch.Generator().manual_seed(1)
    v = torch.randn(2, 7, 5, 6, generator=g, dtype=torch.float64) * 3 + 1.5
    res = torch.randn(2, 7, 5, 6, generator=g, dtype=torch.float64)
    gy = torch.randn(2, 7, 5, 6, generator=g, dtype=torch.float64)
    mean, var, rstd = R.stats64(v)
    xt = nchw(v).clone().requires_grad_(True)
    xh = F.instance_norm(xt, eps=R.EPS64)
    torch.testing.assert_close(nchw(R.apply64(v, mean, rstd, act, res)), act_torch(xh, act) + nchw(res), **TOL)
    torch.testing.assert_close(var, nchw(v).flatten(2).var(2, unbiased=False), **TOL)
    act_torch(xh, act).backward(nchw(gy))
    if act == R.ACT_TANH:       # the norm backward takes relu / lrelu masks; tanh's derivative comes from gan_act_bwd
        gm = gy * R.act_grad_from_out64(torch.tanh(nhwc(xh.detach())), act)
    else:
        gm = R.act_mask64(gy, v, mean, act)
    torch.testing.assert_close(nchw(R.bwd64(v, mean, rstd, gm)), xt.grad, **TOL)


@pytest.mark.parametrize("mode,name", [(R.HALO_REFLECT, "reflect"), (R.HALO_REPLICATE, "replicate")])
@pytest.mark.parametrize("H,W,p", [(4, 4, 1), (8, 9, 3), (6, 20, 2), (5, 7, 1)])
def test_halo_and_fold_statements_equal_float64_autograd(H, W, p, mode, name):
    g = torch.Generator().manual_seed(2)
    v = torch.randn(2, H, W, 3, generator=g, dtype=torch.float64)
    xt = nchw(v).clone().requires_grad_(True)
    padded = F.pad(xt, (p, p, p, p), mode=name)
    torch.testing.assert_close(nchw(R.halo64(v, p, mode)), padded.detach(), **TOL)
    gp = torch.randn(2, H + 2 * p, W + 2 * p, 3, generator=g, dtype=torch.float64)
    padded.backward(nchw(gp))
    torch.testing.assert_close(nchw(R.fold_full64(gp, p, mode)), xt.grad, **TOL)
    if mode == R.HALO_REFLECT:      # what the wrong variants state differs from it
        assert not torch.allclose(R.fold_full64(gp, p, mode, corners=False), nhwc(xt.grad))
        assert not torch.allclose(R.fold_full64(gp, p, mode, pad=p - 1), nhwc(xt.grad))


@pytest.mark.parametrize("act", N.ACTS_ALL)
def test_activation_gradient_from_the_output_equals_autograd(act):
    v = torch.randn(500, generator=torch.Generator().manual_seed(3), dtype=torch.float64).requires_grad_(True)
    y = act_torch(v, act)
    y.sum().backward()
    torch.testing.assert_close(R.act_grad_from_out64(y.detach(), act), v.grad, **TOL)


def test_view_statements_kept_for_the_e4m3_tests():
    """norm_ref64 / fold64 / bwd_ref64 moved out of tests/fp8_producer_cases.py: still the biased InstanceNorm and its gradient"""
    ctx = make()
    x, gy = ctx.view(2, 6, 7, 8, 0, dtype=F32), ctx.view(2, 6, 7, 8, 1, dtype=F32)
    g = torch.Generator().manual_seed(4)
    x.t.copy_(torch.randn(x.t.shape, generator=g))
    gy.t.copy_(torch.randn(gy.t.shape, generator=g))
    xt = nchw(x.nhwc().double()).clone().requires_grad_(True)
    y = torch.relu(F.instance_norm(xt, eps=R.EPS64))
    out, _, _ = R.norm_ref64(x, 1, None)
    torch.testing.assert_close(nchw(out), y.detach(), **TOL)
    pad = F.pad(y, (1, 1, 1, 1), mode="reflect")
    pad.backward(nchw(gy.padded().double()))
    torch.testing.assert_close(nchw(R.bwd_ref64(x, 1, gy, True)), xt.grad, **TOL)


# ---------------------------------------------------------------------------------------------- regimes and data
@pytest.mark.parametrize("p", N.CASE_IDS, ids=N.case_id)
def test_case_is_in_the_regime_it_names(p):
    idx, dtype = p
    case = N.CASES[idx]
    N.check_regime(make(), case, dtype, None)
    B, H, W, C, halo = case.shape
    assert B * (H + 2 * halo) * (W + 2 * halo) * C <= 3.3e6           # the largest buffer of the suite


def test_offset_100_channels_are_well_conditioned_on_the_small_maps_only():
    """mean / sigma = 100 is inside the bounded group up to about a thousand pixels and outside it on the 96-chunk maps: both sides of
    the condition are exercised"""
    inside = outside = 0
    for idx, dtype in N.CASE_IDS:
        shape = N.CASES[idx].shape
        if shape[1] * shape[2] == 1:
            continue
        well = N.stats_tol(N.make_x(shape, dtype).double())[-1]
        sel = torch.tensor([k in ("off+100", "off-100") for k in N.channel_classes(shape[3])])
        inside += int(well[:, sel].sum())
        outside += int((~well[:, sel]).sum())
    assert inside > 0 and outside > 0, (inside, outside)


# ---------------------------------------------------------------------------------------------- looseness: an honest fp32 sum stays inside
def lane_model(v32, n, RL):
    """fp32 model of in_partial_kernel: n chunks of ceil(HW / n) pixels, RL row lanes striding each chunk and adding sequentially, the
    lanes added sequentially, the chunks' partials in float64.  v32: (HW, C) float32.  Returns float64 (S, Q) per channel."""
    HW, C = v32.shape
    per = -(-HW // n)
    S, Q = np.zeros(C), np.zeros(C)
    for ch in range(n):
        blk = v32[ch * per:(ch + 1) * per]
        if not len(blk):
            continue
        steps = -(-len(blk) // RL)
        pad = np.zeros((steps * RL, C), np.float32)
        pad[:len(blk)] = blk
        pad = pad.reshape(steps, RL, C)
        s = np.cumsum(np.cumsum(pad, 0, dtype=np.float32)[-1], 0, dtype=np.float32)[-1]
        q = np.cumsum(np.cumsum(pad * pad, 0, dtype=np.float32)[-1], 0, dtype=np.float32)[-1]
        S, Q = S + s.astype(np.float64), Q + q.astype(np.float64)
    return S, Q


@pytest.mark.parametrize("p", N.CASE_IDS, ids=N.case_id)
def test_fp32_lane_model_stays_inside_the_statistics_bound(p):
    idx, dtype = p
    shape = N.CASES[idx].shape
    B, H, W, C, _ = shape
    geom = N.geometry(shape, dtype)
    v = N.make_x(shape, dtype)
    mean, var, rstd, tm, tv, lo, hi, well = N.stats_tol(v.double())
    worst = 0.0
    for n in {geom["nch"], geom["nparts"]}:
        for b in range(min(B, 3)):
            S, Q = lane_model(v[b].float().reshape(H * W, C).numpy(), n, geom["RL"])
            m, va, r = R.stats_from_sums64(torch.from_numpy(S), torch.from_numpy(Q), H * W)
            worst = max(worst, N.ratio(m.float(), mean[b], tm[b]), N.ratio(va, var[b], tv[b]))
            assert bool(((r >= lo[b]) & (r <= hi[b])).all())
    print(f"[norm-family] lane model {N.case_id(p)}: sums at {worst:.3g} of the bound")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------- the emulator inside the bounds
@pytest.mark.parametrize("group", ["stats", "apply", "bwd", "fold"])
@pytest.mark.parametrize("p", N.CASE_IDS, ids=N.case_id)
def test_emulated_family_within_the_derived_bounds(p, group):
    N.body(make, group, p[0], p[1])


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("shape", N.LIMIT_SHAPES)
def test_emulated_known_limit(shape, dtype):
    N.body_limit(make, shape, dtype)


# ---------------------------------------------------------------------------------------------- the assertions bite
@pytest.mark.parametrize("group,wrong", [(g, w) for g, ws in N.WRONG.items() for w in ws], ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_emulated_family_rejects_a_wrong_reference(group, wrong):
    N.rejects(make, group, wrong)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_emulated_nan_plane(dtype):
    """a NaN in x reaches its whole (image, channel) plane of y through every activation -- ReLU included -- and no other plane"""
    assert N.body_nan_plane(make, dtype) == 16
