"""The 256-channel tiles of the range-patch convolution (csrc/conv_patch.hip) after their prologue and epilogues were made to fit in the
register file without scratch: the 3x3 256 -> 256 residual layer at the two shapes of the CUT step, B = 1 and 2, bf16,

  * the 64x64 map on the 256-row tile (conv_patch_kernel<256, 4, 0, false, 7, 256>; forced to 288 rows as well: 15 tiles per image, the
    last one 64 real rows of 288),
  * the 66x66 padded input-gradient domain on the 288-row tile (conv_patch_kernel<288, ...> and conv_patch_bwdchain_kernel<288, 4, 7, 256>:
    16 tiles per image, the last one 36 real rows; the plain epilogue on 256 rows as well: 18 tiles, the last one 4 real rows),

through every epilogue the restructuring touched: the plain store, the fused InstanceNorm partials (two passes over the channel
fragments, the first pass's 16-byte runs kept in registers), the ReLU, the LeakyReLU' mask, and the backward chain (stats_mode 1).

Each case runs through tests/conv_cases.run, which asserts from gan_conv_igemm_variant / gan_conv_patch_variant that the launch is on the
tile the case names, fills the output and the partials (with 128-byte guard zones) with a sentinel, launches twice and requires the same
bits, and requires inputs, weights, mask and operand unchanged; then elements, partials (summed in float64) and chain sums are held to
the float64 statement with the derived bounds of tests/conv_ref64.py -- the numbers of tests/test_conv_family_gpu.py, nothing new.  The
float64 statement itself (unfold + matmul, shared by the epilogue variants of a shape) is held to float64 F.conv2d /
F.conv_transpose2d here.  A forward into a view WITH a halo leaves the halo's sentinel and stores the bits of the halo-free run.

Observed on an MI355X (worst error / bound per case): see profiles/conv_patch_spills.txt."""
import pytest
import torch
import torch.nn.functional as F

from gan_variant_research_amd import BF16
from gan_variant_research_amd.convplan import ConvLayer
from gan_variant_research_amd.runtime import Ctx, HipOps, cpad
from tests import conv_cases as C
from tests import conv_ref64 as R
from tests.cases import to_view
from tests.emulator import HALO_REFLECT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

G_REFLECT = (256, 256, 3, 1, 1, False, 64, 64, True)      # the residual layer: forward on 64x64, input gradient on the 66x66 padded domain
G_ZERO = (256, 256, 3, 1, 1, False, 64, 64, False)        # the same layer zero-padded: its input gradient takes the LeakyReLU' mask
T256 = [("GAN_PATCH_BN", "256"), ("GAN_PATCH_BM", "256")]
T288 = [("GAN_PATCH_BN", "256"), ("GAN_PATCH_BM", "288")]


def make(dtype):
    return Ctx(HipOps(torch.device(DEV)), DEV, dtype)


def _specs():
    out = []
    for B in (1, 2):
        P = lambda g, op, env, **kw: C.Spec(g, B, BF16, op, "patch", env=env, layout=1, cols=256, slices=7, static_taps=0, **kw)
        for env, rows, tiles in ((T256, 256, 16), (T288, 288, 15)):      # the 64x64 map
            out += [P(G_REFLECT, "fwd", env, rows=rows, tiles=B * tiles),
                    P(G_REFLECT, "fwd", env, rows=rows, tiles=B * tiles, stats=True),
                    P(G_REFLECT, "fwd", env, rows=rows, tiles=B * tiles, act=R.ACT_RELU),
                    P(G_ZERO, "dgrad", env, rows=rows, tiles=B * tiles, mask=1)]
        out += [P(G_REFLECT, "dgrad", T288, rows=288, tiles=B * 16),      # the 66x66 padded domain
                P(G_REFLECT, "dgrad", T288, rows=288, tiles=B * 16, chain=True),
                P(G_REFLECT, "dgrad", T256, rows=256, tiles=B * 18)]
    return out


SPECS = _specs()
_shared = {}


@pytest.fixture(autouse=True)
def share_the_float64_convolution(monkeypatch):
    """tests/conv_ref64.layer64 once per (direction, padding, batch): the epilogue variants of a shape hold the same operands (weights and
    images are seeded by the geometry alone), so they share the float64 convolution and its |operand| sum"""
    plain = R.layer64

    def layer64(op, g, w64, b64, src64, padded_domain=False):
        key = (op, g, src64.shape[0], b64 is None, padded_domain)
        if key not in _shared:
            _shared[key] = (plain(op, g, w64, b64, src64, padded_domain), w64, src64)
        val, w0, s0 = _shared[key]
        assert torch.equal(w0, w64) and torch.equal(s0, src64), "the shared float64 convolution was asked for other operands"
        return val
    monkeypatch.setattr(R, "layer64", layer64)


@pytest.mark.parametrize("S", SPECS, ids=C.spec_id)
def test_epilogue_within_the_derived_bounds(S):
    """key, sentinels and guard zones, bit-unchanged inputs and the bit-identical second launch (tests/conv_cases.run); elements, the
    partials summed in float64 and the chain sums against the float64 statement"""
    res = C.result(make, S)
    for k in res["keys"]:
        assert (k["rows_v"], k["cols_v"]) == (dict(S.expect)["rows"], 256), k
    assert (res["stats"] is not None) == (S.stats or S.chain)
    C.check(make, "epilogue", S)


@pytest.mark.parametrize("S", [s for s in SPECS if s.B == 2 and s.act == R.ACT_NONE and not s.stats and not s.chain and s.mask is None
                               and dict(s.env)["GAN_PATCH_BM"] == ("256" if s.op == "fwd" else "288")], ids=C.spec_id)
def test_the_float64_statement_is_float64_conv2d(S):
    """the reference the cases above are held to against torch's own float64 convolution on the CPU: the forward with reflect padding and
    bias, and the padded-domain input gradient (a transposed convolution without padding)"""
    res = C.result(make, S)
    t, A, K, _ = C.reference(res, C.Ref())
    w, x = res["w64"], res["src"]
    if S.op == "fwd":
        want = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, res["b64"])
    else:
        want = F.conv_transpose2d(x, w)
    assert want.shape == t.shape
    # two float64 summations of K terms in different orders: K * 2^-53 * sum |terms|, with the factor 4 of tests/cases.BOUND_C to spare
    assert bool(((t - want).abs() <= 4 * K * 2.0 ** -53 * A).all()), float(((t - want).abs() / A).max())


@pytest.mark.parametrize("rows,tiles", [(256, 16), (288, 15)])
def test_partials_do_not_depend_on_the_tile_width(rows, tiles):
    """the 64x64 forward with fused partials on 128- against 256-channel tiles of the same height: result and partials bit-identical
    (sums of squares are sum + round(t * t) in every instantiation: csrc/conv_patch.hip, sq_rn)"""
    B = 2
    wide = next(s for s in SPECS if s.B == B and s.op == "fwd" and s.stats and dict(s.expect)["rows"] == rows)
    narrow = C.Spec(G_REFLECT, B, BF16, "fwd", "patch", env=[("GAN_PATCH_BN", "128"), ("GAN_PATCH_BM", str(rows))], stats=True,
                    layout=1, rows=rows, cols=128, slices=7, static_taps=9 if rows == 256 else 0, tiles=B * tiles * 2)
    C.check_tile_width_invariance(make, narrow, wide)


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("rows", [256, 288])
def test_forward_into_a_view_with_a_halo_leaves_the_halo(rows, stats):
    """The forward of the step writes into the next layer's padded view.  Output with a one-pixel halo, everything pre-filled with the
    sentinel: the halo, the guard zones and (with partials) the floats behind partials[B][P][C][2] keep it, the interior holds the bits
    of the halo-free run of the same case, and a second launch repeats them."""
    B = 2
    S = next(s for s in SPECS if s.B == B and s.op == "fwd" and s.stats == stats and s.act == R.ACT_NONE and dict(s.expect)["rows"] == rows)
    want = C.result(make, S)
    ctx = make(BF16)
    rec = C.Recorder(ctx.ops)
    ctx.ops = rec
    g = S.g
    w, b = C.make_weights(S)
    w, b = w.to(ctx.device), b.to(ctx.device)
    layer = ConvLayer(ctx, w, b, torch.zeros_like(w), torch.zeros_like(b), g.k, g.s, g.p, g.tr)
    xin = to_view(ctx, C.make_src(S), 1, HALO_REFLECT)
    out, out_big = C.guarded(ctx, B, g.H, g.W, cpad(g.cout), 1, BF16, C.OUT_FILL)
    ws = ws_big = None
    with pytest.MonkeyPatch.context() as mp:
        for k, v in S.env:
            mp.setenv(k, v)
        if stats:
            ws, ws_big = C.guarded_f32(ctx, B * C.MAXP * out.C * 2, C.ST_FILL)
        ops = layer.fwd(xin, out, S.act, None, True, ws)
    keys = C.assert_reached(S, rec, rec.calls)
    assert all(k["rows_v"] == rows and k["cols_v"] == 256 for k in keys), keys
    for o in layer.repack_ops():
        o()
    snaps = []
    for _ in range(2):
        out_big.fill_(C.OUT_FILL)
        if ws_big is not None:
            ws_big.fill_(C.ST_FILL)
        for o in ops:
            o()
        torch.cuda.synchronize()
        snaps.append((C.bits(out_big), None if ws_big is None else C.bits(ws_big)))
    assert torch.equal(snaps[0][0], snaps[1][0]) and (ws_big is None or torch.equal(snaps[0][1], snaps[1][1])), "a repeated launch gave other bits"
    full = out_big.detach().cpu()
    sent = C.bits(torch.full((1,), C.OUT_FILL, dtype=full.dtype))[0]
    fb = C.bits(full)
    assert bool((fb[:C.GUARD] == sent).all() and (fb[-C.GUARD:] == sent).all()), "the guard zone of the output was written"
    pad = fb[C.GUARD:-C.GUARD].view(B, out.Hp, out.Wp, out.C)
    inner = torch.zeros(out.Hp, out.Wp, dtype=torch.bool)
    inner[1:1 + g.H, 1:1 + g.W] = True
    assert bool((pad[:, ~inner] == sent).all()), "the output's halo was written"
    assert torch.equal(pad[:, 1:1 + g.H, 1:1 + g.W].contiguous(), want["got_bits"]), "the interior differs from the halo-free run"
    if stats:
        sb = ws_big.detach().cpu()
        n = B * layer.stats_parts * out.C * 2
        assert bool((sb[:C.GUARD] == C.ST_FILL).all() and (sb[C.GUARD + n:] == C.ST_FILL).all()), "floats outside the partials were written"
        assert torch.equal(C.bits(sb[C.GUARD:C.GUARD + n].view(B, layer.stats_parts, out.C, 2)), want["stats_bits"]), "the partials differ from the halo-free run"
