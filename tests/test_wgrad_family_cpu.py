"""The weight-gradient family (gan_conv_wgrad's generic, range-patch and 7x7 window kernels, gan_wgrad_reduce, gan_bias_grad) without a
GPU: the float64 statements of tests/wgrad_ref64.py against torch's float64 autograd on non-square maps, every case of
tests/wgrad_cases.py planned onto the kernel, split count, path and lane count it names (emulator and library agree), the emulator's
statement of every case inside the derived bounds (which therefore admit an honest implementation), every deliberately wrong reference
outside them, and the refused descriptors.  tests/test_wgrad_family_gpu.py runs the same bodies on the HIP kernels."""
import pytest
import torch
import torch.nn.functional as F

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd.convplan import ConvLayer
from gan_variant_research_amd.runtime import Ctx, HipOps, cpad
from tests import wgrad_cases as W
from tests import wgrad_ref64 as R
from tests.emulator import EmuOps

TOL = dict(rtol=1e-12, atol=1e-12)


def make(dtype):
    return Ctx(EmuOps(), "cpu", dtype)


def make_slabbed(dtype):
    return Ctx(W.SlabEmuOps(), "cpu", dtype)


# ---------------------------------------------------------------------------------------------- the statements against float64 torch
@pytest.mark.parametrize("g", [(5, 7, 3, 1, 1, False, 6, 11, True), (4, 6, 4, 2, 1, False, 6, 10, False), (6, 5, 3, 2, 1, True, 3, 7, False),
                               (3, 4, 7, 1, 3, False, 9, 5, True), (4, 3, 3, 2, 1, False, 7, 13, False)], ids=str)
def test_statements_equal_float64_autograd_on_non_square_maps(g):
    """layer64, the descriptor-level desc64 (through a planned call's tap table, strides and origins; whole and cut into slabs) and bias64
    against the weight and bias gradients of F.conv2d / F.conv_transpose2d in float64 (operands exact in fp32: the views hold them)"""
    cin, cout, k, s, p, tr, H, Wd, reflect = g
    gen = torch.Generator().manual_seed(5)
    w = torch.randn((cin, cout, k, k) if tr else (cout, cin, k, k), generator=gen, dtype=torch.float64).requires_grad_(True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    x = torch.randn(3, cin, H, Wd, generator=gen).double()
    if tr:
        y = F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    else:
        y = F.conv2d(F.pad(x, (p, p, p, p), mode="reflect" if reflect else "constant"), w, b, stride=s)
    dy = torch.randn(y.shape, generator=gen).double()
    y.backward(dy)
    ref, A, K = R.layer64(k, s, p, tr, reflect, x, dy, tuple(w.shape))
    torch.testing.assert_close(ref, w.grad, **TOL)
    assert K == (x if tr else dy).shape[0] * (x if tr else dy).shape[2] * (x if tr else dy).shape[3] and bool((A >= ref.abs() - 1e-9).all())
    # the descriptor-level statement, on the call the planner builds for fp32 views with halos beyond the minimum
    ctx = Ctx(W.Guarding(EmuOps(), None, launch=False), "cpu", F32)
    ctx.ops._ctx = ctx
    layer = ConvLayer(ctx, w.detach().float(), b.detach().float(), torch.zeros_like(w).float(), torch.zeros(cout), k, s, p, tr)
    mode = W.HALO_REFLECT if reflect else W.HALO_ZERO
    xv, dyv = (W.to_view(ctx, x.float(), 2, W.HALO_ZERO), W.to_view(ctx, dy.float(), 2, W.HALO_ZERO)) if tr else \
              (W.to_view(ctx, x.float(), p + 1, mode), W.to_view(ctx, dy.float(), k - 1, W.HALO_ZERO))
    W.nan_halo(xv if tr else dyv)
    layer.wgrad(xv, dyv, False)
    c = ctx.ops.call
    d = R.desc_of(c)
    whole = R.desc64(d, c.x.padded().double(), c.g.padded().double())[0]             # [N][taps][Cx], taps row-major
    n_real, c_real = (cin, cout) if tr else (cout, cin)
    torch.testing.assert_close(whole[:n_real, :, :c_real].permute(0, 2, 1).reshape(n_real, c_real, k, k), w.grad, **TOL)
    assert not whole[n_real:].any() and not whole[:, :, c_real:].any()
    M = d.B * d.Ho * d.Wo
    cuts = [(0, 1), (1, M // 2), (M // 2, M)]
    torch.testing.assert_close(R.desc64(d, c.x.padded().double(), c.g.padded().double(), cuts).sum(0), whole, **TOL)
    rb, Ab, Kb = R.bias64(dyv.padded().double(), dyv.halo, dyv.H, dyv.W, cout)
    torch.testing.assert_close(rb, b.grad, **TOL)
    assert Kb == dy.shape[0] * dy.shape[2] * dy.shape[3]


def test_reduction_statement_is_the_index_formula():
    """reduce64 against a literal loop over (s, n, t, c)"""
    r = W.REDUCE[4]
    gen = torch.Generator().manual_seed(6)
    part = torch.randn(r.nsplit * r.N * r.ntaps * r.Cx, generator=gen)
    n_grad = r.C_real * r.I2 * r.KK
    ref, bound, touched = R.reduce64(part, r.nsplit, r.N, r.ntaps, r.Cx, r.N_real, r.C_real, r.swap, r.I2, r.KK, r.khw, n_grad)
    p = part.double().view(r.nsplit, r.N, r.ntaps, r.Cx)
    want = torch.zeros(n_grad, dtype=torch.float64)
    for n in range(0, r.N_real, 5):
        for t in range(r.ntaps):
            for c in range(r.C_real):
                o = (c * r.I2 + n) * r.KK + r.khw[t]
                want[o] = p[:, n, t, c].sum()
                assert touched[o] and abs(float(ref[o] - want[o])) < 1e-12 and bound[o] > 0
    assert int(touched.sum()) == r.N_real * r.C_real * sum(k >= 0 for k in r.khw)
    assert R.slab_rows(1083, 2) == 576 and R.slab_rows(16896, 27) == 640 and R.slab_rows(16384, 3) == 5504 and R.slab_rows(2178, 4) == 576


# ---------------------------------------------------------------------------------------------- every case plans where it says
@pytest.mark.parametrize("S", W.CASES, ids=W.case_id)
def test_library_plans_the_kernel_the_case_names(S):
    """the library's host functions (no GPU) plan the variant, split count, addressing path and reduction lanes the case names, and the
    emulator's planner statements agree with them"""
    c = W.check_plan(HipOps(torch.device("cpu")), S)
    e = W.check_plan(EmuOps(), S)
    assert (c.variant, c.nsplit) == (e.variant, e.nsplit)


def test_cases_reach_what_the_family_is_about():
    """the list itself: both addressing paths, M < 64, splits that begin mid-image with a ragged tail, skinny tiles, Wo = 1, the persistent
    walk past 256 tiles, every lane count of the reduction"""
    gen = [S for S in W.GENERIC]
    assert {S.fast for S in gen} == {0, 1} and any(S.B * W.out_hw(S.g)[0] * W.out_hw(S.g)[1] < 64 for S in gen)
    assert any(S.nsplit > 1 and R.slab_rows(S.B * S.g.H * S.g.W, S.nsplit) % (S.g.H * S.g.W) and (S.B * S.g.H * S.g.W) % 64 for S in gen)
    assert any(S.g.cout <= 16 for S in gen) and any(W.out_hw(S.g)[1] == 1 for S in gen)
    assert any(S.B * -(-S.g.H // 16) * -(-S.g.W // 16) > 256 for S in W.WINDOW)
    assert {r.lanes for r in W.REDUCE} == {1, 2, 4, 8, 16, 32} and {S.lanes for S in W.CASES} >= {1, 4, 16, 32}
    hip = HipOps(torch.device("cpu"))
    for r in W.REDUCE + W.REDUCE_PAST_THE_GRID:
        assert hip.wgrad_reduce_lanes(r.nsplit, r.N_real, r.ntaps, r.Cx) == r.lanes, r
    r = W.REDUCE_PAST_THE_GRID[1]
    assert r.N_real * r.ntaps * (r.Cx // 4) > 8192 * 256          # more quads than the capped grid has threads: the stride loop runs


# ---------------------------------------------------------------------------------------------- the emulator inside the bounds
@pytest.mark.parametrize("S", W.CASES, ids=W.case_id)
def test_emulated_case_within_the_derived_bounds(S):
    W.check(make, S)


@pytest.mark.parametrize("S", [S for S in W.GENERIC if S.nsplit > 1 and tuple(S.g) not in W.BIG], ids=W.case_id)
def test_emulated_slabs_within_the_derived_bounds(S):
    """the per-slab assertion on the emulator that cuts slabs as gan_conv_wgrad does"""
    W.check(make_slabbed, S)


@pytest.mark.parametrize("S", W.ACCUMULATE, ids=W.case_id)
def test_emulated_accumulate_is_one_fp32_addition(S):
    W.check_accumulate(make, S)


def test_emulated_bias_accumulate_can_differ():
    W.check_accumulate(make, W.BIAS_ACCUMULATE_DIFFERS, bias_differs=True)


@pytest.mark.parametrize("where", ["dy", "x"])
@pytest.mark.parametrize("S", W.NAN_CASES, ids=W.case_id)
def test_emulated_one_nan_stays_in_its_footprint(S, where):
    W.check_nan(make, S, where)


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("r", W.REDUCE + W.REDUCE_PAST_THE_GRID, ids=W.rcase_id)
def test_emulated_reduction_alone(r, accumulate):
    W.body_reduce(make, r, accumulate, lanes_of=HipOps(torch.device("cpu")).wgrad_reduce_lanes)


@pytest.mark.parametrize("halo", [0, 2])
@pytest.mark.parametrize("b", W.BIAS, ids=W.bcase_id)
def test_emulated_bias_gradient_alone(b, halo):
    W.body_bias(make, b, halo)


def test_emulated_family_has_a_figure_for_every_variant():
    W.summary(make)


# ---------------------------------------------------------------------------------------------- the assertions bite
@pytest.mark.parametrize("wrong", W.WRONG, ids=lambda w: w.__name__)
def test_emulated_family_rejects_a_wrong_reference(wrong):
    """The emulator's results held to a deliberately wrong reference: the assertions fail on every named case."""
    W.rejects(make, wrong, make_slabbed)


def test_one_dropped_pixel_shows_at_the_longest_reductions():
    """the bound still sees one pixel left out at K = 34452 (both window cases), K = 16896 and K = 1083"""
    W.rejects(make, W.WRONG[0])


# ---------------------------------------------------------------------------------------------- host side of the library
def test_refused_descriptors_return_their_error():
    assert W.body_refused(HipOps(torch.device("cpu")), "cpu") >= 15
