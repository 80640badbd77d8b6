"""The per-element error bound of the float64 convolution checks (cases.BOUND_C, cases.conv_ref64) on the CPU: an honest fp32
convolution of bf16 operands passes it; a reference with one kernel tap dropped or one image missing from the weight gradient fails it."""
import torch
import torch.nn.functional as F

from tests import cases


def _operands(B, cin, cout, k, H, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, H, generator=g).bfloat16().double()
    w = (torch.randn(cout, cin, k, k, generator=g) * (0.5 / (cin * k * k) ** 0.5)).bfloat16().double()
    return x, w


def test_reference_matches_torch_in_float64():
    x, w = _operands(2, 16, 24, 3, 10)
    for reflect in (False, True):
        ref, A, K = cases.conv_ref64("fwd", 3, 1, 1, False, reflect, w, x=x)
        torch.testing.assert_close(ref, F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect" if reflect else "constant"), w), rtol=1e-12, atol=1e-12)
        assert K == 9 * 16 and bool((A >= ref.abs()).all())
    wt = w.transpose(0, 1).contiguous()          # ConvTranspose2d weight [in = 16][out = 24][k][k]
    xin = torch.randn(2, 16, 5, 5, dtype=torch.float64)
    ref, _, _ = cases.conv_ref64("fwd", 3, 2, 1, True, False, wt, x=xin)
    torch.testing.assert_close(ref, F.conv_transpose2d(xin, wt, stride=2, padding=1, output_padding=1), rtol=1e-12, atol=1e-12)
    dy = torch.randn(2, 24, 5, 5, dtype=torch.float64)
    xs = torch.randn(2, 16, 10, 10, dtype=torch.float64, requires_grad=True)
    wr = w.clone().requires_grad_(True)
    F.conv2d(xs, wr, stride=2, padding=1).backward(dy)
    torch.testing.assert_close(cases.conv_ref64("dgrad", 3, 2, 1, False, False, w, dy=dy, x_hw=(10, 10))[0], xs.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(cases.conv_ref64("wgrad", 3, 2, 1, False, False, w, x=xs.detach(), dy=dy)[0], wr.grad, rtol=1e-12, atol=1e-12)


def test_fp32_convolution_of_bf16_operands_is_within_the_bound_and_dropped_work_is_not():
    B, cin, cout, k, H = 4, 64, 32, 3, 24
    x, w = _operands(B, cin, cout, k, H)
    ref, A, K = cases.conv_ref64("fwd", k, 1, 1, False, True, w, x=x)
    got32 = F.conv2d(F.pad(x.float(), (1, 1, 1, 1), mode="reflect"), w.float())
    assert cases.bound_ratio(got32.bfloat16().float(), ref, A, K, cases.U_BF16) <= 1.0      # bf16-stored output
    assert cases.bound_ratio(got32, ref, A, K, cases.U_F32) <= 1.0                          # fp32-stored output
    w_drop = w.clone()
    w_drop[:, :, 1, 1] = 0
    assert cases.bound_ratio(got32.bfloat16().float(), cases.conv_ref64("fwd", k, 1, 1, False, True, w_drop, x=x)[0], A, K, cases.U_BF16) > 1.0
    # input gradient: same, dropped tap rejected
    dy = torch.randn(B, cout, H, H, generator=torch.Generator().manual_seed(1)).bfloat16().double()
    ref, A, K = cases.conv_ref64("dgrad", k, 1, 1, False, False, w, dy=dy, x_hw=(H, H))
    xs = torch.zeros(B, cin, H, H, requires_grad=True)
    F.conv2d(xs, w.float(), padding=1).backward(dy.float())
    assert cases.bound_ratio(xs.grad.bfloat16().float(), ref, A, K, cases.U_BF16) <= 1.0
    assert cases.bound_ratio(xs.grad.bfloat16().float(), cases.conv_ref64("dgrad", k, 1, 1, False, False, w_drop, dy=dy, x_hw=(H, H))[0], A, K,
                             cases.U_BF16) > 1.0
    # weight gradient (fp32 result, u_out = 0): one image of the batch left out is rejected
    ref, A, K = cases.conv_ref64("wgrad", k, 1, 1, False, False, w, x=x, dy=dy)
    assert K == B * H * H
    wr = w.float().clone().requires_grad_(True)
    F.conv2d(x.float(), wr, padding=1).backward(dy.float())
    assert cases.bound_ratio(wr.grad, ref, A, K, 0.0) <= 1.0
    short = cases.conv_ref64("wgrad", k, 1, 1, False, False, w, x=x[1:], dy=dy[1:])[0]
    assert cases.bound_ratio(short, ref, A, K, 0.0) > 1.0
