"""TEST INFRASTRUCTURE: cases, derived bounds and assertions for the convolution launches behind gan_conv_igemm (csrc/conv_igemm.hip,
conv_patch.hip, conv_win7.hip), written against an op layer: tests/test_conv_family_cpu.py runs them on the emulator,
tests/test_conv_family_gpu.py on HipOps, with the same shapes and the same assertions.  The float64 statements and the bounds are in
tests/conv_ref64.py; the weight gradient, its reduction and the bias gradient are held by the family of their own in tests/wgrad_cases.py
(tests/test_wgrad_family_cpu.py, tests/test_wgrad_family_gpu.py).  A `Spec` names the direction in `op`, and `run` dispatches on it.

A `Spec` is one planned request on a ConvLayer (forward or input gradient, with its epilogue); `run` plans it on a recording op layer,
fills every output, partial buffer and guard zone with a sentinel (the views are slices of larger tensors, 128 / 256 bytes in), launches
it twice and returns what it left.  Every run asserts, before any figure is compared:
  * the key of the recording op layer (weight layout; on the library also tile rows and columns, tiles, grid, and the bits of
    gan_conv_patch_variant) names the kernel and branch the case is meant for -- a miss fails;
  * only the documented elements changed: the output's stored pixels (all out_C channels of them), partials [B][P][C][2];
  * inputs, mask, operand and packed weights are bit-unchanged; the repeated launch gave the same bits; pad channels are exactly 0.
"""
import math
from collections import namedtuple

import pytest
import torch

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd.convplan import ConvLayer
from gan_variant_research_amd.runtime import Ctx, View, cpad, torch_dtype
from tests import conv_ref64 as R
from tests.cases import BOUND_C, U_BF16, U_F32, to_view
from tests.emulator import HALO_REFLECT, HALO_ZERO, EmuOps

U = U_F32
NAME = {BF16: "bf16", F32: "fp32"}
TDT = {BF16: torch.bfloat16, F32: torch.float32}
BITS = {BF16: torch.int16, F32: torch.int32}
U_OUT = {BF16: U_BF16, F32: U_F32}
OUT_FILL, ST_FILL = 7.5, -9.0           # exact in bf16 and fp32
GUARD = 64                              # elements before and after every sentinel view: 128 bytes (bf16) / 256 bytes (fp32)
MAXP = 16                               # partials per image the workspaces of these cases leave room for

Geom = namedtuple("Geom", "cin cout k s p tr H W reflect")
_SpecT = namedtuple("Spec", "g B dtype op act bias mask stats chain poison env expect variant")


def Spec(g, B, dtype, op, variant, act=R.ACT_NONE, bias=True, mask=None, stats=False, chain=False, poison=None, env=(), **expect):
    """op: 'fwd' | 'dgrad'; mask: None or the halo of the LeakyReLU' mask view; stats: fused partials (mode 0); chain: backward chain
    (mode 1); poison: None | 'nan' | 'inf'; env: ((name, value), ...) set while the call is planned; variant: the kernel the case is
    meant for ('generic' | 'patch' | 'win7'), expect: what every (or, for a list, some) launch's key must hold."""
    return _SpecT(Geom(*g), B, dtype, op, act, bias and op == "fwd", mask, stats, chain, poison, tuple(env),
                  tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in expect.items())), variant)


def spec_id(S):
    g = S.g
    s = f"{g.cin}-{g.cout}k{g.k}s{g.s}{'T' if g.tr else ''}{'r' if g.reflect else 'z'}-{g.H}x{g.W}-B{S.B}-{NAME[S.dtype]}-{S.op}"
    s += (f"-act{S.act}" if S.act else "") + (f"-mask{S.mask}" if S.mask is not None else "")
    s += "".join(f"-{n}" for n, v in (("nobias", S.op == "fwd" and not S.bias), ("stats", S.stats), ("chain", S.chain), (S.poison, S.poison)) if v)
    return s + "".join(f"-{k[-2:]}{v}" for k, v in S.env)


def out_hw(g):
    return (2 * g.H, 2 * g.W) if g.tr else ((g.H + 2 * g.p - g.k) // g.s + 1, (g.W + 2 * g.p - g.k) // g.s + 1)


# ------------------------------------------------------------------------------------------------ the cases
# The 20 shapes of the geometry group: (cin, cout, k, s, p, transposed, H, W, reflect), then per direction the kernel the bf16 planner
# takes and its launch count, and the launch count in fp32 (always the generic kernel; no paired phases there).  None: no such direction.
TABLE = [
    ((3, 16, 7, 1, 3, False, 5, 23, True), ("generic", 1, 1), ("generic", 1, 1)),
    ((64, 3, 7, 1, 3, False, 17, 33, True), ("win7", 1, 1), ("win7", 1, 1)),
    ((3, 64, 7, 1, 3, False, 33, 4, True), ("win7", 1, 1), ("win7", 1, 1)),
    ((16, 32, 3, 2, 1, False, 6, 14, False), ("generic", 1, 1), ("generic", 4, 4)),
    ((16, 32, 3, 2, 1, False, 7, 13, False), ("generic", 1, 1), ("generic", 4, 4)),     # stride 2 on an odd map: phases of 4x7, 4x6, 3x7, 3x6
    ((3, 16, 4, 2, 1, False, 9, 5, False), ("generic", 1, 1), ("generic", 4, 4)),         # k4 on an odd map: 5x3, 5x2, 4x3, 4x2
    ((128, 256, 4, 2, 1, False, 9, 11, False), ("patch", 1, 1), ("patch", 4, 4)),         # the four 4-tap phases, each with its own extent
    ((64, 128, 3, 2, 1, False, 7, 13, False), ("patch", 1, 1), ("generic", 4, 4)),        # 64 output channels on an odd map: never paired
    ((64, 128, 3, 2, 1, False, 6, 13, False), ("patch", 1, 1), ("generic", 4, 4)),        # even H, odd W: not paired either
    ((16, 32, 3, 2, 1, False, 1, 1, False), ("generic", 1, 1), ("generic", 1, 1)),        # one pixel: phase (0, 0) alone has an extent
    ((128, 128, 3, 1, 1, False, 2, 40, True), ("patch", 1, 1), ("patch", 1, 1)),
    ((128, 128, 3, 1, 1, False, 19, 15, True), ("patch", 1, 1), ("patch", 1, 1)),
    ((128, 64, 3, 2, 1, True, 3, 9, False), ("patch", 2, 4), ("patch", 1, 1)),          # forward: the paired phases
    ((64, 128, 4, 2, 1, False, 6, 10, False), ("patch", 1, 1), ("patch", 2, 4)),        # stride-2 input; input gradient: the paired phases
    ((256, 1, 4, 1, 1, False, 2, 9, False), ("generic", 1, 1), ("generic", 1, 1)),
    ((64, 1, 4, 1, 1, False, 9, 2, False), ("generic", 1, 1), ("generic", 1, 1)),
    ((8, 8, 3, 1, 1, False, 1, 1, False), ("generic", 1, 1), ("generic", 1, 1)),
    ((64, 128, 3, 1, 1, False, 1, 37, False), ("patch", 1, 1), ("generic", 1, 1)),
    ((64, 128, 3, 1, 1, False, 37, 1, False), ("generic", 1, 1), ("generic", 1, 1)),    # Wo = 1 falls to the generic kernel
    ((256, 256, 3, 1, 1, False, 12, 64, True), ("patch", 1, 1), ("patch", 1, 1)),
]
LAYOUT = {"generic": 0, "patch": 1, "win7": 2}


def _geometry_specs():
    out = []
    for g, fwd, dgrad in TABLE:
        for op, plan in (("fwd", fwd), ("dgrad", dgrad)):
            if plan is None:
                continue
            kern, n, n32 = plan
            for B in (1, 3):
                out.append(Spec(g, B, BF16, op, kern, layout=LAYOUT[kern], n=n))
                out.append(Spec(g, B, F32, op, "generic", layout=0, n=n32))
    # ---- generic kernel
    for dt in (BF16, F32):
        out.append(Spec((16, 64, 3, 1, 1, False, 3, 3, False), 20, dt, "fwd", "generic", layout=0, rows=128, tiles=8, grid=8))  # 9-pixel maps: 14 images in a tile
        out.append(Spec((16, 64, 3, 1, 1, False, 8, 16, False), 1, dt, "fwd", "generic", layout=0, rows=128))                    # Ho * Wo = 128
        out.append(Spec((16, 64, 3, 1, 1, False, 3, 43, False), 1, dt, "fwd", "generic", layout=0, rows=128))                    # Ho * Wo = 129
    out.append(Spec((8, 256, 3, 1, 1, False, 105, 105, False), 3, F32, "fwd", "generic", layout=0, rows=128, cols=128, tiles=528, grid=512))       # MT = 259: skipped virtual tiles, a ragged last tile
    out.append(Spec((8, 1, 4, 1, 1, False, 257, 257, False), 1, BF16, "fwd", "generic", layout=0, rows=256, cols=16))
    # ---- range-patch kernel
    P = lambda g, B=3, op="fwd", **kw: Spec(g, B, BF16, op, "patch", layout=1, **kw)
    out += [
        P((64, 128, 3, 1, 1, False, 3, 100, True), slices=9, rows=256, cols=128),                           # 9-slice buffers: a 100-pixel-wide map
        P((128, 128, 3, 1, 1, False, 3, 100, True), op="dgrad", slices=9),
        P((64, 128, 3, 1, 1, False, 2, 129, False), B=1, slices=9),                                          # M_img = 258
        P((128, 128, 3, 1, 1, False, 15, 17, True), slices=7, rows=256, cols=128, static_taps=9),          # M_img = 255: one below a tile
        P((128, 128, 3, 1, 1, False, 16, 16, True), rows=256, static_taps=9, tiles=3),                      # M_img = 256: exactly a tile
        P((128, 128, 3, 1, 1, False, 17, 17, True), env=[("GAN_PATCH_BM", "288")], rows=288, tiles=6, static_taps=0),   # 289 = one above a 288-row tile
        P((128, 128, 3, 1, 1, False, 12, 24, True), env=[("GAN_PATCH_BM", "288")], rows=288, tiles=3),      # 288: exactly a 288-row tile
        P((256, 256, 3, 1, 1, False, 12, 20, True), env=[("GAN_PATCH_BN", "256")], rows=256, cols=256),
        P((256, 256, 3, 1, 1, False, 12, 20, True), env=[("GAN_PATCH_BN", "256"), ("GAN_PATCH_BM", "288")], rows=288, cols=256),
        P((256, 256, 3, 1, 1, False, 12, 20, True), op="dgrad", env=[("GAN_PATCH_BN", "256")], rows=256, cols=256),
        P((128, 256, 4, 2, 1, False, 6, 10, False), op="dgrad", static_taps=4, n=4),                       # the four 4-tap phases of a k4 s2 input gradient
        P((128, 256, 4, 2, 1, False, 9, 11, False), op="dgrad", static_taps=4, n=4, rows=256, cols=128,    # ... on an odd map: 5x6, 5x5, 4x6 and 4x5 pixels,
          some=[(("layout", 1), ("static_taps", 4), ("tiles", 3))]),                                          # none too small for the kernel: one tile per image
        Spec((64, 128, 3, 2, 1, False, 7, 13, False), 3, BF16, "dgrad", "generic", layout=0, n=4, cols=64),  # an odd destination is not viewed as super-pixels
        Spec((128, 256, 3, 2, 1, False, 6, 10, False), 3, BF16, "dgrad", "patch", some=[(("layout", 1), ("static_taps", 2)), (("layout", 1), ("static_taps", 4)), (("layout", 0),)], n=4),
        P((128, 128, 4, 1, 1, False, 6, 10, False), static_taps=16),
        P((64, 128, 7, 1, 3, False, 9, 12, True), static_taps=0, slices=7),                                 # the generic tap loop: 49 taps
        P((64, 128, 3, 1, 1, False, 40, 2, False)),                                                         # Wo = 2
        P((64, 128, 3, 2, 1, False, 6, 10, False), op="dgrad", n=2, cols=128),                              # paired phases: a strided input gradient
        P((128, 64, 3, 2, 1, True, 3, 9, False), op="fwd", n=2, cols=128),                                  # paired phases: a transposed forward
    ]
    # ---- 7x7 window kernels, both, forward and input gradient
    for H, W in ((16, 16), (17, 33), (33, 4), (4, 33)):
        for g in ((64, 3, 7, 1, 3, False, H, W, True), (3, 64, 7, 1, 3, False, H, W, True)):
            for op in ("fwd", "dgrad"):
                out.append(Spec(g, 3, BF16, op, "win7", layout=2, rows=256, tiles=3 * (-(-(H + (6 if op == "dgrad" else 0)) // 16)) * (-(-(W + (6 if op == "dgrad" else 0)) // 16))))
    for g in ((64, 3, 7, 1, 3, False, 1, 9, False), (3, 64, 7, 1, 3, False, 1, 9, False)):
        out += [Spec(g, 3, BF16, "fwd", "win7", layout=2), Spec(g, 3, BF16, "dgrad", "win7", layout=2)]
    return list(dict.fromkeys(out))


E_GEN, E_GEN1, E_GEN3 = (16, 20, 3, 1, 1, False, 5, 7, False), (32, 1, 4, 1, 1, False, 5, 7, False), (16, 3, 3, 1, 1, False, 5, 7, True)
E_PATCH, E_PATCH2 = (64, 128, 3, 1, 1, False, 6, 11, True), (64, 128, 3, 1, 1, False, 20, 20, True)
E_TO3, E_FROM3 = (64, 3, 7, 1, 3, False, 9, 20, True), (3, 64, 7, 1, 3, False, 17, 33, True)
E_CHAIN, E_WIDE = (128, 128, 3, 1, 1, False, 6, 10, True), (256, 256, 3, 1, 1, False, 12, 20, True)
ACTS = (R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU, R.ACT_TANH)


def _epilogue_specs():
    out = []
    for act in ACTS:
        for bias in (True, False):
            out += [Spec(E_GEN, 3, dt, "fwd", "generic", act=act, bias=bias, layout=0) for dt in (BF16, F32)]
            out.append(Spec(E_PATCH, 3, BF16, "fwd", "patch", act=act, bias=bias, layout=1))
            if act in (R.ACT_NONE, R.ACT_TANH):
                out.append(Spec(E_TO3, 3, BF16, "fwd", "win7", act=act, bias=bias, layout=2))
        out += [Spec(gg, 3, dt, "fwd", "generic", act=act, layout=0) for gg in (E_GEN1, E_GEN3) for dt in (BF16, F32)]       # cout 1 and 3 (20: E_GEN)
    out += [Spec(E_FROM3, 3, BF16, "fwd", "win7", bias=b, layout=2) for b in (True, False)]
    for mh in (0, 1):          # the LeakyReLU' mask: stride-1 and phased input gradients, generic and range-patch
        out += [Spec((16, 32, 4, 1, 1, False, 6, 9, False), 3, dt, "dgrad", "generic", mask=mh, layout=0) for dt in (BF16, F32)]
        out += [Spec((16, 32, 3, 2, 1, False, 6, 10, False), 3, dt, "dgrad", "generic", mask=mh, layout=0, n=4) for dt in (BF16, F32)]
        out.append(Spec((128, 64, 4, 1, 1, False, 6, 9, False), 3, BF16, "dgrad", "patch", mask=mh, layout=1))
        out.append(Spec((128, 128, 4, 2, 1, False, 6, 10, False), 3, BF16, "dgrad", "patch", mask=mh, layout=1, n=4))
        out += [Spec((16, 32, 4, 2, 1, False, 9, 7, False), 3, dt, "dgrad", "generic", mask=mh, layout=0, n=4) for dt in (BF16, F32)]       # odd maps: the mask
        out.append(Spec((128, 256, 4, 2, 1, False, 9, 11, False), 3, BF16, "dgrad", "patch", mask=mh, layout=1, n=4, static_taps=4))     # offsets follow the phase
        out.append(Spec((32, 16, 3, 2, 1, True, 3, 5, False), 3, BF16, "dgrad", "generic", mask=mh, layout=0))          # a transposed layer's input gradient
    out += [Spec(E_PATCH, 3, BF16, "fwd", "patch", stats=True, layout=1), Spec(E_PATCH2, 3, BF16, "fwd", "patch", stats=True, layout=1, tiles=6),
            Spec(E_PATCH, 1, BF16, "fwd", "patch", stats=True, layout=1), Spec(E_FROM3, 3, BF16, "fwd", "win7", stats=True, layout=2),
            Spec(E_FROM3, 3, BF16, "fwd", "win7", stats=True, bias=False, layout=2), Spec(E_PATCH2, 3, BF16, "fwd", "patch", stats=True, bias=False, layout=1)]
    out += [Spec(E_CHAIN, B, BF16, "dgrad", "patch", chain=True, layout=1) for B in (1, 3)]
    for bn in ("128", "256"):
        out.append(Spec(E_WIDE, 3, BF16, "fwd", "patch", stats=True, env=[("GAN_PATCH_BN", bn)], layout=1, cols=int(bn)))
        out.append(Spec(E_WIDE, 3, BF16, "dgrad", "patch", chain=True, env=[("GAN_PATCH_BN", bn)], layout=1, cols=int(bn)))
    return list(dict.fromkeys(out))


def _nonfinite_specs():
    out = []
    for poison in ("nan", "inf"):
        for act in ACTS:
            out += [Spec(E_GEN, 3, dt, "fwd", "generic", act=act, poison=poison, layout=0) for dt in (BF16, F32)]
            out.append(Spec(E_PATCH2, 3, BF16, "fwd", "patch", act=act, poison=poison, layout=1, tiles=6))       # 400 pixels: image 0's last tile is ragged
        out += [Spec(E_TO3, 3, BF16, "fwd", "win7", act=R.ACT_TANH, poison=poison, layout=2), Spec(E_FROM3, 3, BF16, "fwd", "win7", poison=poison, stats=True, layout=2),
                Spec(E_PATCH2, 3, BF16, "fwd", "patch", stats=True, poison=poison, layout=1),
                Spec((128, 64, 4, 1, 1, False, 6, 9, False), 3, BF16, "dgrad", "patch", mask=1, poison=poison, layout=1),
                Spec((16, 32, 3, 2, 1, False, 6, 10, False), 3, F32, "dgrad", "generic", mask=0, poison=poison, layout=0, n=4),
                Spec((16, 32, 3, 2, 1, False, 7, 13, False), 3, F32, "dgrad", "generic", mask=0, poison=poison, layout=0, n=4),      # an odd strided input gradient
                Spec((128, 64, 3, 2, 1, True, 6, 10, False), 3, BF16, "fwd", "patch", poison=poison, layout=1, n=2),      # paired: the widened footprint
                Spec((256, 128, 3, 2, 1, True, 6, 10, False), 3, BF16, "fwd", "patch", poison=poison, n=4, some=[(("layout", 1), ("static_taps", 4)), (("layout", 0),)]),     # unpaired
                Spec(E_CHAIN, 3, BF16, "dgrad", "patch", chain=True, poison=poison, layout=1)]
    return list(dict.fromkeys(out))


GEOMETRY, EPILOGUE, NONFINITE = _geometry_specs(), _epilogue_specs(), _nonfinite_specs()
GROUPS = {"geometry": GEOMETRY, "epilogue": EPILOGUE, "nonfinite": NONFINITE}


# ------------------------------------------------------------------------------------------------ recording op layer, keys
class Recorder:
    """an op layer that remembers every ConvCall it is asked to launch"""

    def __init__(self, ops, launch=True):
        self._ops, self.calls, self._launch = ops, [], launch

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def conv_igemm(self, c):
        self.calls.append(c)
        return self._ops.conv_igemm(c) if self._launch else None


def key_of(ops, c):
    k = {"layout": 2 if c.win7 is not None else 1 if c.w_frag else 0}
    if ops.is_hip:
        k.update(ops.conv_igemm_variant(c))
        if c.w_frag:
            v = ops.conv_patch_variant(c)
            k.update(slices=v["slices"], static_taps=v["static_taps"], rows_v=v["rows"], cols_v=v["cols"])
    return k


def assert_reached(S, ops, calls):
    keys = [key_of(ops, c) for c in calls]
    exp = dict(S.expect)
    n, some = exp.pop("n", 1), exp.pop("some", None)
    assert len(keys) == n, f"{spec_id(S)}: {len(keys)} launches, the case names {n}: {keys}"
    for name, want in exp.items():
        for k in keys:
            if name in k:                   # the emulator's key holds the layout only
                assert k[name] == want, f"{spec_id(S)}: did not reach the branch it names: {name} = {k[name]}, wanted {want} ({keys})"
        assert ops.is_hip is False or all(name in k for k in keys), f"{spec_id(S)}: the key has no {name}: {keys}"
    for want in some or ():
        hit = [k for k in keys if all(k.get(a, b) == b for a, b in want)]
        assert hit, f"{spec_id(S)}: no launch with {dict(want)}: {keys}"
    for k in keys:
        if "rows_v" in k:
            assert (k["rows_v"], k["cols_v"]) == (k["rows"], k["cols"]), k
    return keys


# ------------------------------------------------------------------------------------------------ data
def _gen(*seed):
    return torch.Generator().manual_seed(hash(seed) % (2 ** 31))


def make_weights(S):
    g = S.g
    gen = _gen(g.cin, g.cout, g.k, g.s, int(g.tr), 5)
    w = torch.randn((g.cin, g.cout, g.k, g.k) if g.tr else (g.cout, g.cin, g.k, g.k), generator=gen) * (0.5 / (g.cin * g.k * g.k) ** 0.5)
    b = torch.randn(g.cout, generator=gen) * 0.3
    return w, b


def make_src(S):
    """the launch's operand, NCHW, rounded to the dtype, image by image (image b does not depend on B)"""
    g = S.g
    C, (H, W) = (g.cin, (g.H, g.W)) if S.op == "fwd" else (g.cout, out_hw(g))
    v = torch.stack([torch.randn(C, H, W, generator=_gen(g.H, g.W, C, b, 7)) * (1.0 if b != 2 else 2.0 ** -6) for b in range(S.B)])
    v = v.to(TDT[S.dtype]).float()
    if S.poison:
        v[1, min(1, C - 1), min(1, H - 1), min(1, W - 1)] = float("nan") if S.poison == "nan" else float("inf")
    return v


def make_mask(S, Cp, halo):
    """(B, H + 2 halo, W + 2 halo, Cp) in the dtype: mixed signs, exact zeros and -0.0, the halo as busy as the interior"""
    g = S.g
    v = torch.stack([torch.randn(g.H + 2 * halo, g.W + 2 * halo, Cp, generator=_gen(g.H, g.W, Cp, b, halo, 11)) for b in range(S.B)])
    sel = torch.stack([torch.rand(g.H + 2 * halo, g.W + 2 * halo, Cp, generator=_gen(g.H, g.W, Cp, b, halo, 13)) for b in range(S.B)])
    v = torch.where(sel < 0.1, torch.zeros(()), v)
    v = torch.where((sel >= 0.1) & (sel < 0.2), torch.tensor(-0.0), v)
    return v.to(TDT[S.dtype])


def guarded(ctx, B, H, W, C, halo, dtype, fill):
    n = B * (H + 2 * halo) * (W + 2 * halo) * C
    big = torch.full((n + 2 * GUARD,), fill, dtype=torch_dtype(dtype), device=ctx.device)
    v = View(big[GUARD:GUARD + n], B, H, W, C, halo, dtype)
    assert v.ptr() % 16 == 0
    return v, big


def guarded_f32(ctx, n, fill):
    big = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device=ctx.device)
    return big[GUARD:GUARD + n], big


def sync(ctx):
    if ctx.device.type == "cuda":
        torch.cuda.synchronize()


def bits(t):
    t = t.detach().cpu()
    return t.contiguous().view(BITS[BF16] if t.dtype == torch.bfloat16 else torch.int32).clone()


# ------------------------------------------------------------------------------------------------ one planned request, launched
def run(make, S):
    """plans S on make(S.dtype)'s op layer, launches it twice from sentinels and returns what it left (CPU tensors)"""
    ctx = make(S.dtype)
    rec = Recorder(ctx.ops)
    ctx.ops = rec
    g, dev = S.g, ctx.device
    w, b = make_weights(S)
    w, b = w.to(dev), b.to(dev)
    layer = ConvLayer(ctx, w, b, torch.zeros_like(w), torch.zeros_like(b), g.k, g.s, g.p, g.tr)
    src = make_src(S)
    Ho, Wo = out_hw(g)
    res = {"spec": S, "is_hip": rec.is_hip, "src": src.double(), "padded": False, "mask": None, "operand": None, "stats": None}
    with pytest.MonkeyPatch.context() as mp:      # tile forcing is read at planning time only (gan_conv_patch_tile_rows / _cols)
        for k in ("GAN_PATCH_BM", "GAN_PATCH_BN"):
            mp.delenv(k, raising=False)
        for k, v in S.env:
            mp.setenv(k, v)
        stats_ws = stats_big = None
        if S.op == "fwd":
            xin = to_view(ctx, src, max(g.p, 1), HALO_REFLECT if g.reflect else HALO_ZERO)
            out, out_big = guarded(ctx, S.B, Ho, Wo, cpad(g.cout), 0, S.dtype, OUT_FILL)
            if S.stats:
                stats_ws, stats_big = guarded_f32(ctx, S.B * MAXP * out.C * 2, ST_FILL)
            ops = layer.fwd(xin, out, S.act, None, S.bias, stats_ws)
            nparts = layer.stats_parts
            assert not S.stats or nparts > 0, f"{spec_id(S)}: the launch cannot write the fused partials the case is about"
        else:
            out_C = cpad(g.cin)
            mask = opd = None
            if S.mask is not None:
                mask = View(make_mask(S, out_C, S.mask).to(dev).reshape(-1), S.B, g.H, g.W, out_C, S.mask, S.dtype)
                res["mask"] = mask.padded().detach().cpu().double()
            padded = g.s == 1 and not g.tr and g.reflect
            res["padded"] = padded
            if g.tr or g.s == 2:
                xin = to_view(ctx, src, 1, HALO_ZERO)
                out, out_big = guarded(ctx, S.B, g.H, g.W, out_C, 0, S.dtype, OUT_FILL)
                ops = layer.dgrad(xin, out, mask)
            elif padded:
                xin = to_view(ctx, src, g.k - 1, HALO_ZERO)
                out, out_big = guarded(ctx, S.B, g.H, g.W, out_C, g.p, S.dtype, OUT_FILL)
                chain = None
                if S.chain:     # the saved ReLU output with its reflect halo: mixed signs and zeros (a general operand: the sums are linear in it)
                    y = make_mask(S, g.cin, 0).float().permute(0, 3, 1, 2).contiguous()
                    opd = to_view(ctx, y, g.p, HALO_REFLECT)
                    res["operand"] = opd.padded().detach().cpu().double()
                    stats_ws, stats_big = guarded_f32(ctx, S.B * MAXP * out_C * 2, ST_FILL)
                    chain = {"operand": opd, "ws": stats_ws}
                ops = layer.dgrad(xin, out, padded_domain=True, chain=chain)
                nparts = layer.chain_parts
            else:
                xin = to_view(ctx, src, g.k - 1 - g.p, HALO_ZERO)
                out, out_big = guarded(ctx, S.B, g.H, g.W, out_C, 0, S.dtype, OUT_FILL)
                ops = layer.dgrad(xin, out, mask)
            if not S.chain:
                nparts = 0
    res["keys"] = assert_reached(S, rec, rec.calls)
    res["paired"] = any(c.out.C == 128 and c.out is not out for c in rec.calls)
    for o in layer.repack_ops():
        o()
    sync(ctx)
    packs = [t for pk in layer.packs for t in (pk._w, pk._wf) if t is not None]
    before = [bits(t) for t in [xin.t, w, b] + packs + ([mask.t] if S.op == "dgrad" and mask is not None else []) + ([opd.t] if S.op == "dgrad" and opd is not None else [])]
    snaps = []
    for _ in range(2):
        out_big.fill_(OUT_FILL)
        if stats_big is not None:
            stats_big.fill_(ST_FILL)
        for o in ops:
            o()
        sync(ctx)
        snaps.append((bits(out_big), None if stats_big is None else bits(stats_big)))
    after = [bits(t) for t in [xin.t, w, b] + packs + ([mask.t] if S.op == "dgrad" and mask is not None else []) + ([opd.t] if S.op == "dgrad" and opd is not None else [])]
    what = spec_id(S)
    assert all(torch.equal(a, c) for a, c in zip(before, after)), f"{what}: an input, a weight copy, the mask or the operand changed"
    assert torch.equal(snaps[0][0], snaps[1][0]), f"{what}: a repeated launch gave other bits"
    assert stats_big is None or torch.equal(snaps[0][1], snaps[1][1]), f"{what}: a repeated launch gave other partials"
    # ---- only the documented elements changed
    full = out_big.detach().cpu()
    sent = bits(torch.full((1,), OUT_FILL, dtype=full.dtype))[0]
    fb = bits(full)
    assert bool((fb[:GUARD] == sent).all() and (fb[-GUARD:] == sent).all()), f"{what}: the guard zone of the output was written"
    pad = full[GUARD:-GUARD].view(S.B, out.Hp, out.Wp, out.C)
    if not res["padded"] and out.halo:
        inner = torch.zeros(out.Hp, out.Wp, dtype=torch.bool)
        inner[out.halo:out.halo + out.H, out.halo:out.halo + out.W] = True
        assert bool((bits(pad)[:, ~inner] == sent).all()), f"{what}: the output's halo was written"
    region = pad if res["padded"] or not out.halo else pad[:, out.halo:out.halo + out.H, out.halo:out.halo + out.W]
    creal = g.cout if S.op == "fwd" else g.cin
    res["got"] = region[..., :creal].permute(0, 3, 1, 2).double()
    res["got_bits"] = bits(region.contiguous())
    res["padch"] = region[..., creal:].float()
    res["u_out"] = U_OUT[S.dtype]
    res["nparts"] = nparts
    if stats_big is not None:
        sb = stats_big.detach().cpu()
        n = S.B * nparts * out.C * 2
        assert nparts <= MAXP and bool((sb[:GUARD] == ST_FILL).all() and (sb[GUARD + n:] == ST_FILL).all()), f"{what}: floats outside partials[B][{nparts}][C][2] were written"
        res["stats"] = sb[GUARD:GUARD + n].view(S.B, nparts, out.C, 2)[..., :creal, :].double().sum(1)      # summed over an image's partials: (B, C, 2)
        res["stats_bits"] = bits(sb[GUARD:GUARD + n].view(S.B, nparts, out.C, 2))
    w_ref = w.cpu().bfloat16().double() if S.dtype == BF16 else w.cpu().double()
    res["w64"], res["b64"] = w_ref, (b.cpu().double() if S.bias else None)
    return res


_results = {}


def result(make, S):
    k = (make(S.dtype).device.type, S)
    if k not in _results:
        _results[k] = run(make, S)
    return _results[k]


# ------------------------------------------------------------------------------------------------ the reference a result is held to
class Ref:
    drop_tap = swap_taps = zero_pad = bias_after = mask_off = swap_phase = no_outpad = rounded_stats = unrounded_chain = missing_image = False
    even_extent = False
    slope = 0.2


def _wrong(name, **kw):
    return type(name, (Ref,), kw)


WRONG = [_wrong("TapDropped", drop_tap=True), _wrong("TapRowsAndColumnsSwapped", swap_taps=True), _wrong("ZeroPaddingForReflect", zero_pad=True),
         _wrong("BiasAfterActivation", bias_after=True), _wrong("SlopeZero", slope=0.0), _wrong("MaskOnePixelOff", mask_off=True),
         _wrong("PhaseRowAndColumnSwapped", swap_phase=True), _wrong("NoOutputPadding", no_outpad=True), _wrong("StatisticsOfTheRoundedResult", rounded_stats=True),
         _wrong("ChainSumsOfTheUnroundedGradient", unrounded_chain=True), _wrong("OneImageMissing", missing_image=True),
         _wrong("PhasesOfOneExtent", even_extent=True)]

_refs = {}


def reference(res, ref):
    """(t, A, K, mf): pre-activation float64 result, |operand| sum, reduction length and mask factor (or None), as `ref` states them;
    the honest one is computed once per case and shared"""
    S = res["spec"]
    honest = type(ref) is Ref
    if honest and S in _refs:
        return _refs[S]
    g, w64, b64 = S.g, res["w64"], res["b64"]
    if ref.drop_tap:
        w64 = w64.clone()
        w64[:, :, g.k - 1, 0] = 0.0
    if ref.swap_taps:
        w64 = w64.transpose(2, 3).contiguous()
    if ref.zero_pad:
        g = g._replace(reflect=False)
    t, A, K = R.layer64(S.op, g, w64, None if ref.bias_after else b64, res["src"], res["padded"])
    if ref.no_outpad and g.tr and S.op == "fwd":
        t = t.clone()
        fillv = 0.0 if b64 is None else b64.view(1, -1, 1)
        t[:, :, -1, :] = fillv
        t[:, :, :, -1] = fillv
    mf = None
    if res["mask"] is not None:
        m, h = res["mask"], S.mask
        if ref.mask_off:
            m = torch.roll(m, 1, 2)
        mf = R.mask_factor64(m[:, h:h + g.H, h:h + g.W, :g.cin].permute(0, 3, 1, 2), ref.slope)
    out = (t, A, K, mf)
    if honest:
        _refs[S] = out
    return out


def stated(res, ref):
    """the float64 result `ref` states, with its tolerance and the pre-activation error bound"""
    S = res["spec"]
    t, A, K, mf = reference(res, ref)
    val = R.epilogue64(t, S.act, mf, ref.slope)
    if ref.bias_after and res["b64"] is not None:
        val = val + res["b64"].view(1, -1, 1, 1)
    if ref.swap_phase and val.shape[2] % 2 == 0 and val.shape[3] % 2 == 0:
        val = val.clone()
        a, b = val[..., 0::2, 1::2].clone(), val[..., 1::2, 0::2].clone()
        val[..., 0::2, 1::2], val[..., 1::2, 0::2] = b, a
    if ref.missing_image and S.B > 1:
        val = val.clone()
        val[S.B - 1] = val[0]
    if ref.even_extent and S.op == "dgrad" and S.g.s == 2 and not S.g.tr:      # every phase H // 2 x W // 2: the last row / column of an odd map is left out
        val = val.clone()
        val[:, :, 2 * (S.g.H // 2):, :] = 0.0
        val[:, :, :, 2 * (S.g.W // 2):] = 0.0
    tol, et = R.elem_tol(t, A, K, S.act, mf, res["u_out"], res["b64"] is not None)
    return val, tol, t, et


def ratio(got, ref, tol):
    return (got - ref).abs() / (tol + 1e-300)


_worst = {}
_rejecting = []


def report(group, S, what, r, extra="", dev="cpu"):
    if _rejecting:
        print(f"[conv-family] (against the wrong reference {_rejecting[0]}) {group} {spec_id(S)} {what}: {r:.3g}")
        return r
    k = (dev, group, f"{S.variant}-{NAME[S.dtype]}")
    _worst[k] = max(_worst.get(k, 0.0), r)
    print(f"[conv-family] {group:9s} {k[2]:12s} {spec_id(S)} {what}: error / bound = {r:.3g}{extra}   (worst of the variant so far {_worst[k]:.3g})")
    return r


def check(make, group, S, ref=None):
    """the result of S against the float64 statement: elements, pad channels, partials or chain sums.  Returns the worst error / bound."""
    ref = ref or Ref()
    res = result(make, S)
    what = spec_id(S)
    val, tol, t, et = stated(res, ref)
    got = res["got"]
    assert got.shape == val.shape, (got.shape, val.shape)
    if S.poison:
        return check_nonfinite(make, group, S, res, val, tol, t, et)
    assert bool(torch.isfinite(got).all()), f"{what}: a non-finite result from finite operands"
    assert bool((res["padch"] == 0).all()), f"{what}: a pad channel of the output is not exactly zero"
    worst = float(ratio(got, val, tol).max())
    extra = ""
    if res["stats"] is not None:
        st = res["stats"]
        if S.chain:
            # the honest statement sums the gradient the launch itself stored (its elements are held to float64 above): the sums are then
            # independent of the kernel only in the summation
            gs = val if ref.unrounded_chain else got
            y = res["operand"][..., :S.g.cin].permute(0, 3, 1, 2)
            s1, s2, t1, t2 = R.chain_sums64(gs, y)
        else:
            tt = t.to(TDT[S.dtype]).double() if ref.rounded_stats else t
            s1, s2 = tt.sum((2, 3)), (tt * tt).sum((2, 3))
            t1, t2 = R.sums_tol(t, et)
        if ref.missing_image and S.B > 1:
            s1, s2 = s1.clone(), s2.clone()
            s1[S.B - 1], s2[S.B - 1] = s1[0], s2[0]
        rs = max(float(ratio(st[..., 0], s1, t1).max()), float(ratio(st[..., 1], s2, t2).max()))
        extra = f", sums {rs:.3g}"
        worst = max(worst, rs)
    report(group, S, "elements" + (" and sums" if extra else ""), worst, extra, dev=make(S.dtype).device.type)
    assert worst <= 1.0, f"{what}: max error / bound = {worst:.3g}{extra}"
    return worst


_excused = {}


def check_nonfinite(make, group, S, res, val, tol, t, et):
    """one NaN / +Inf in a real channel of one pixel near the top of image 1 of 3"""
    what = spec_id(S)
    clean = result(make, S._replace(poison=None))
    got = res["got"]
    for b in (0, 2):
        assert torch.equal(res["got_bits"][b], clean["got_bits"][b]), f"{what}: image {b} differs from the clean run"
        assert res["stats"] is None or torch.equal(res["stats_bits"][b], clean["stats_bits"][b]), f"{what}: the partials of image {b} differ from the clean run"
    bad = ~torch.isfinite(val[1])
    assert bool((~torch.isfinite(t[1])).any()), f"{what}: the poison reaches nothing"        # (tanh(+-Inf) = +-1: `bad` may then be empty)
    g1 = got[1]
    assert bool((~torch.isfinite(g1[bad])).all()), f"{what}: an element whose reference is not finite came out finite"
    assert bool(torch.isnan(g1[torch.isnan(val[1])]).all()), f"{what}: a NaN of the reference is not a NaN in the result"
    # every other real element: within the bound (where the poison only passed an activation's flat side, the reference value exactly)
    tol1 = torch.where(torch.isfinite(tol[1]), tol[1], res["u_out"] * val[1].abs() + 4 * U)
    rr = ratio(g1, val[1], tol1)
    over = ~bad & ~(rr <= 1.0)
    excused = torch.zeros_like(bad)
    if res["paired"]:      # the union of the two x-phases' footprints minus the reference's: both pixels of a 128-channel super-pixel
        px = bad.any(0)
        pair = px.view(px.shape[0], -1, 2).any(-1, keepdim=True).expand(-1, -1, 2).reshape(px.shape)
        excused = (pair & ~px).unsqueeze(0).expand_as(bad)
    n_exc = int(excused.any(0).sum())
    _excused[(make(S.dtype).device.type, what)] = n_exc
    assert not bool((over & ~excused).any()), f"{what}: {int((over & ~excused).sum())} elements outside the poison's footprint are off ({float(rr[over & ~excused].max()):.3g} of the bound)"
    fin = ~bad & ~excused & torch.isfinite(rr)
    worst = float(rr[fin].max()) if bool(fin.any()) else 0.0
    extra = f", footprint {int(bad.any(0).sum())} pixels, excused {n_exc}"
    if res["stats"] is not None and not S.chain:      # the sums of a poisoned (image, channel) follow the reference's: not finite where its are not
        s1 = t[1].sum((1, 2))
        assert bool((~torch.isfinite(res["stats"][1][..., 0][~torch.isfinite(s1)])).all()), f"{what}: a partial sum over a poisoned plane is finite"
    report(group, S, "clean elements of the poisoned image", worst, extra, dev=make(S.dtype).device.type)
    assert worst <= 1.0
    return worst


# ------------------------------------------------------------------------------------------------ invariances, predicates
def check_batch_invariance(make, S):
    """image 0 at B = 1 is image 0 at B = 3, bit for bit, partials included"""
    a, b = result(make, S._replace(B=1, expect=tuple(e for e in S.expect if e[0] not in ("tiles", "grid")))), result(make, S)
    assert torch.equal(a["got_bits"][0], b["got_bits"][0]), f"{spec_id(S)}: image 0 depends on the batch"
    if a["stats"] is not None:
        assert torch.equal(a["stats_bits"][0], b["stats_bits"][0]), f"{spec_id(S)}: the partials of image 0 depend on the batch"


def check_tile_width_invariance(make, S128, S256):
    a, b = result(make, S128), result(make, S256)
    assert torch.equal(a["got_bits"], b["got_bits"]), "result differs between the 128- and the 256-channel tile"
    assert torch.equal(a["stats_bits"], b["stats_bits"]), "partials differ between the 128- and the 256-channel tile"


def plan_only(ops, S):
    """the ConvCalls of S planned on `ops` with CPU tensors: nothing is launched"""
    rec = Recorder(ops, launch=False)
    return rec, run_plan(Ctx(rec, "cpu", S.dtype), S)


def run_plan(ctx, S):
    g = S.g
    w, b = make_weights(S)
    layer = ConvLayer(ctx, w, b, torch.zeros_like(w), torch.zeros_like(b), g.k, g.s, g.p, g.tr)
    Ho, Wo = out_hw(g)
    if S.op == "fwd":
        layer.fwd(ctx.view(S.B, g.H, g.W, cpad(g.cin), max(g.p, 1)), ctx.view(S.B, Ho, Wo, cpad(g.cout), 0), S.act, None, S.bias,
                  ctx.f32(S.B * MAXP * cpad(g.cout) * 2) if S.stats else None)
    elif g.tr or g.s == 2:
        layer.dgrad(ctx.view(S.B, Ho, Wo, cpad(g.cout), 1), ctx.view(S.B, g.H, g.W, cpad(g.cin), 0), ctx.view(S.B, g.H, g.W, cpad(g.cin), S.mask) if S.mask is not None else None)
    elif g.reflect:
        layer.dgrad(ctx.view(S.B, Ho, Wo, cpad(g.cout), g.k - 1), ctx.view(S.B, g.H, g.W, cpad(g.cin), g.p), padded_domain=True)
    else:
        layer.dgrad(ctx.view(S.B, Ho, Wo, cpad(g.cout), g.k - 1 - g.p), ctx.view(S.B, g.H, g.W, cpad(g.cin), 0), ctx.view(S.B, g.H, g.W, cpad(g.cin), S.mask) if S.mask is not None else None)
    return ctx.ops.calls


def check_predicates(hip_ops, S):
    """EmuOps and the library answer alike on conv_patch_ok, conv_win7_ok and conv_stats_parts > 0 for every call of the case"""
    emu = EmuOps()
    _, calls = plan_only(emu, S)
    assert calls
    for c in calls:
        assert emu.conv_patch_ok(c) == hip_ops.conv_patch_ok(c), f"{spec_id(S)}: conv_patch_ok: emulator {emu.conv_patch_ok(c)}, library {hip_ops.conv_patch_ok(c)}"
        assert emu.conv_win7_ok(c, 0, 0) == hip_ops.conv_win7_ok(c, 0, 0), f"{spec_id(S)}: conv_win7_ok"
        if c.w_frag or c.win7 is not None:
            assert (emu.conv_stats_parts(c) > 0) == (hip_ops.conv_stats_parts(c) > 0), f"{spec_id(S)}: conv_stats_parts"


# ------------------------------------------------------------------------------------------------ wrong references
REJECT_ON = {
    "TapDropped": [Spec(E_GEN, 3, F32, "fwd", "generic", layout=0), Spec((3, 16, 4, 2, 1, False, 9, 5, False), 3, BF16, "dgrad", "generic", layout=0, n=4), Spec(E_PATCH, 3, BF16, "fwd", "patch", layout=1), Spec(E_TO3, 3, BF16, "fwd", "win7", layout=2)],
    "TapRowsAndColumnsSwapped": [Spec(E_GEN, 3, BF16, "fwd", "generic", layout=0), Spec(E_PATCH, 3, BF16, "fwd", "patch", layout=1), Spec(E_FROM3, 3, BF16, "fwd", "win7", layout=2)],
    "ZeroPaddingForReflect": [Spec(E_PATCH, 3, BF16, "fwd", "patch", layout=1), Spec(E_GEN3, 3, F32, "fwd", "generic", layout=0)],
    "BiasAfterActivation": [Spec(E_GEN, 3, BF16, "fwd", "generic", act=R.ACT_RELU, layout=0), Spec(E_PATCH, 3, BF16, "fwd", "patch", act=R.ACT_LRELU, layout=1),
                            Spec(E_TO3, 3, BF16, "fwd", "win7", act=R.ACT_TANH, layout=2)],
    "SlopeZero": [Spec(E_GEN, 3, F32, "fwd", "generic", act=R.ACT_LRELU, layout=0), Spec((128, 64, 4, 1, 1, False, 6, 9, False), 3, BF16, "dgrad", "patch", mask=1, layout=1)],
    "MaskOnePixelOff": [Spec((16, 32, 4, 1, 1, False, 6, 9, False), 3, F32, "dgrad", "generic", mask=1, layout=0),
                        Spec((16, 32, 4, 2, 1, False, 9, 7, False), 3, F32, "dgrad", "generic", mask=1, layout=0, n=4),
                        Spec((128, 256, 4, 2, 1, False, 9, 11, False), 3, BF16, "dgrad", "patch", mask=0, layout=1, n=4, static_taps=4),
                        Spec((128, 128, 4, 2, 1, False, 6, 10, False), 3, BF16, "dgrad", "patch", mask=0, layout=1, n=4)],
    "PhasesOfOneExtent": [Spec((16, 32, 3, 2, 1, False, 7, 13, False), 3, F32, "dgrad", "generic", layout=0, n=4),
                          Spec((64, 128, 3, 2, 1, False, 6, 13, False), 3, BF16, "dgrad", "generic", layout=0, n=4),
                          Spec((128, 256, 4, 2, 1, False, 9, 11, False), 3, BF16, "dgrad", "patch", layout=1, n=4)],
    "PhaseRowAndColumnSwapped": [Spec((16, 32, 3, 2, 1, False, 6, 10, False), 3, F32, "dgrad", "generic", mask=0, layout=0, n=4),
                                 Spec((128, 64, 3, 2, 1, True, 3, 9, False), 3, BF16, "fwd", "patch", layout=1, n=2, cols=128)],
    "NoOutputPadding": [Spec((128, 64, 3, 2, 1, True, 3, 9, False), 3, BF16, "fwd", "patch", layout=1, n=2, cols=128), Spec((128, 64, 3, 2, 1, True, 3, 9, False), 3, F32, "fwd", "generic", layout=0, n=4)],
    "StatisticsOfTheRoundedResult": [Spec(E_PATCH, 3, BF16, "fwd", "patch", stats=True, layout=1), Spec(E_FROM3, 3, BF16, "fwd", "win7", stats=True, bias=False, layout=2)],
    "ChainSumsOfTheUnroundedGradient": [Spec(E_CHAIN, 3, BF16, "dgrad", "patch", chain=True, layout=1)],
    "OneImageMissing": [Spec(E_GEN, 3, F32, "fwd", "generic", layout=0), Spec(E_PATCH2, 3, BF16, "fwd", "patch", stats=True, layout=1, tiles=6)],
}


def rejects(make, wrong):
    failed = []
    _rejecting.append(wrong.__name__)
    try:
        for S in REJECT_ON[wrong.__name__]:
            result(make, S)              # planning, key and contract assertions are not what rejects a reference: they fail here, outside the try
            try:
                check(make, "reject", S, wrong())
            except AssertionError as e:
                failed.append((spec_id(S), str(e)[:100]))
    finally:
        _rejecting.clear()
    print(f"[conv-family] {wrong.__name__} rejected on {failed}")
    assert len(failed) == len(REJECT_ON[wrong.__name__]), f"the assertions accept the wrong reference {wrong.__name__} on a case it was tried on: {failed}"


def summary(make, group):
    """worst error / bound per kernel variant of a group on this device (results are cached: nothing runs twice).  Each case is a test of
    its own: a miss fails there and is only listed here; a variant of the group without a figure of THIS device fails here."""
    dev = make(BF16).device.type
    want = {(dev, group, f"{S.variant}-{NAME[S.dtype]}") for S in GROUPS[group]}
    for S in GROUPS[group]:
        try:
            check(make, group, S)
        except AssertionError as e:
            print(f"[conv-family] SUMMARY {group} MISS {str(e)[:200]}")
    for k in sorted(want):
        assert k in _worst and math.isfinite(_worst[k]), f"no figure for {k}"
        print(f"[conv-family] SUMMARY {k[1]} {k[2]}: worst error / bound = {_worst[k]:.3g}")
    if group == "nonfinite":
        for (d, what), n in sorted(_excused.items()):
            if d == dev:
                print(f"[conv-family] SUMMARY excused footprint {what}: {n} pixels")


def check_plan(hip_ops, S):
    """the library's own plan for S, asked on the host (the queries are pure: no GPU): layout, tile rows and columns, tiles, grid, slices
    and tap schedule are those the case names -- a planner change that moves a case off its branch shows without a GPU"""
    with pytest.MonkeyPatch.context() as mp:
        for k in ("GAN_PATCH_BM", "GAN_PATCH_BN"):
            mp.delenv(k, raising=False)
        for k, v in S.env:
            mp.setenv(k, v)
        _, calls = plan_only(hip_ops, S)
        return assert_reached(S, hip_ops, calls)


# ------------------------------------------------------------------------------------------------ refused descriptors
def body_refused(hip_ops, device):
    """Descriptors the host rejects before any launch: each returns its error and the output keeps its sentinel.  Nothing here would be
    launched: every mutation fails a check of gan_conv_igemm (or of the kernel's own launcher) that precedes the launch."""
    import ctypes
    from gan_variant_research_amd import FP8
    lib = hip_ops.lib
    ctx = Ctx(Recorder(hip_ops, launch=False), device, BF16)

    def planned(g):
        ctx.ops.calls.clear()
        w, b = make_weights(Spec(g, 3, BF16, "fwd", "x"))
        w, b = w.to(ctx.device), b.to(ctx.device)
        layer = ConvLayer(ctx, w, b, torch.zeros_like(w), torch.zeros_like(b), g[2], g[3], g[4], g[5])
        x = ctx.view(3, g[6], g[7], cpad(g[0]), 1)
        out, big = guarded(ctx, 3, g[6], g[7], cpad(g[1]), 0, BF16, OUT_FILL)
        layer.fwd(x, out)
        c, = ctx.ops.calls
        return c, big, (layer, x, out)
    c0, big0, keep0 = planned(E_GEN)
    c1, big1, keep1 = planned(E_PATCH)
    assert not c0.w_frag and c0.win7 is None and c1.w_frag
    stats = ctx.f32(3 * MAXP * 128 * 2, ST_FILL)
    cases = [("Nw", c0, dict(Nw=48), b"must be 16 or a multiple of 64"),
             ("Cin", c0, dict(Cin=24), b"Cin=24"),
             ("ntaps * Cin", c0, dict(ntaps=9), b"not a multiple"),
             ("fp8 on layout 0", c0, dict(dtype=FP8), b"fp8 operands run on the range-patch kernel only"),
             ("statistics on layout 0", c0, dict(stats=stats.data_ptr()), b"fused statistics exist only"),
             ("stats_mode 1 on layout 0", c0, dict(stats_mode=1), b"stats_mode 1 exists only"),
             ("stats_mode 1 without its operand", c1, dict(stats_mode=1, stats=stats.data_ptr(), bias=None, mask=None), b"needs stats and its operand"),
             ("input window above the allocation", c0, dict(in_y0=-1), b"input window outside"),
             ("input window below the allocation", c0, dict(in_y0=c0.x.Hp - c0.Ho + 1), b"input window outside"),
             ("output window outside the allocation", c0, dict(out_x0=1), b"output window outside"),
             ("layout 1 on a descriptor that does not qualify", c0, dict(w_layout=1), b"does not qualify for the range-patch kernel"),
             ("layout 2 on a descriptor that does not qualify", c0, dict(w_layout=2), b"7x7 window kernel does not cover"),
             ("layout 2 on a range-patch descriptor", c1, dict(w_layout=2), b"7x7 window kernel does not cover")]
    for what, c, change, msg in cases:
        d = hip_ops._conv_desc(c)
        for k, v in change.items():
            setattr(d, k, v)
        rc = lib.gan_conv_igemm(ctypes.byref(d), None)
        err = lib.gan_last_error()
        assert rc != 0 and msg in err, f"{what}: rc = {rc}, error {err!r}"
    if ctx.device.type == "cuda":
        torch.cuda.synchronize()
    for big in (big0, big1):
        assert bool((big == OUT_FILL).all()), "a refused descriptor wrote to the output"
    assert bool((stats == ST_FILL).all()), "a refused descriptor wrote partials"
    return len(cases)


# ------------------------------------------------------------------------------------------------ gan_pack_weight, gan_pack_weight_batch
def _pack_batch_op(ops, packs, nblocks_of):
    """HipOps.pack_weight_batch with the block count of each descriptor chosen by the test (any nblocks >= 1 is documented)"""
    from gan_variant_research_amd import _lib
    arr = (_lib.GanPackDesc * len(packs))()
    first, keep = 0, []
    for i, (d, (src, dst, dtype, Nw, ntaps, Cin, N_real, C_real, swap, I2, KK, khw, layout, scale)) in enumerate(zip(arr, packs)):
        keep += [src, dst, khw, scale]
        d.src, d.dst, d.khw = src.data_ptr(), dst.data_ptr(), khw.data_ptr()
        d.scale = scale.data_ptr() if scale is not None else None
        d.dtype, d.Nw, d.ntaps, d.Cin, d.N_real, d.C_real, d.swap, d.I2, d.KK, d.layout = dtype, Nw, ntaps, Cin, N_real, C_real, swap, I2, KK, layout
        d.nblocks = nblocks_of(i, Nw * ntaps * Cin)
        d.first_block, first = first, first + d.nblocks
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(ops.device)
    op = ops._call("gan_pack_weight_batch", ops._p(table), len(packs), first, ops._s())
    op.keep = keep
    return op


def body_pack(make, dtype):
    """gan_pack_weight and gan_pack_weight_batch against tests/conv_ref64.pack64, bit for bit (bf16: round to nearest even of src / scale):
    layouts 0 and 1, swap, khw < 0, N and C padding, the sigma divisor, three descriptors in one launch -- one with a single block on a
    large tensor --, a NaN weight.  The destination sits between guard zones that keep their sentinel."""
    ctx = make(dtype)
    ops, dev = ctx.ops, ctx.device
    gen = _gen(int(dtype), 77)
    # (N_real, C_real, I2, KK, swap, khw, Nw, Cin, layout)
    k9 = list(range(9))
    descs = [(20, 12, 12, 9, False, k9 + [-1, -1, -1], 64, 16, 0),                       # N and C padding, padded taps
             (12, 20, 12, 9, True, [8 - k for k in k9] + [-1] * 3, 64, 32, 0),           # swap: the weight read as [in][out]; flipped taps
             (128, 64, 64, 9, False, [4, -1, 0, 8], 128, 64, 1),                         # fragment-major, a tap list with a hole
             (100, 64, 100, 4, True, [3, 2, 1, 0, -1, -1, -1, -1], 128, 64, 1),          # fragment-major with swap and N padding
             (256, 256, 256, 9, False, k9, 256, 256, 1)]                                  # the large tensor (589,824 elements)
    worst = 0
    singles, batch = [], []
    for i, (N_real, C_real, I2, KK, swap, khw, Nw, Cin, layout) in enumerate(descs):
        n_src = (C_real if swap else N_real) * I2 * KK
        src = torch.randn(n_src, generator=gen) * torch.logspace(-3, 3, n_src)[torch.randperm(n_src, generator=gen)]
        if i in (0, 2):
            src[5] = float("nan")
        src[7], src[9] = 0.0, -0.0
        src = src.to(dev)
        khw_t = ctx.i32(khw)
        for scale in ((None, 1.7) if i in (1, 2, 4) else (None,)):
            dst, big = guarded_f32(ctx, Nw * len(khw) * Cin, ST_FILL) if dtype == F32 else guarded(ctx, 1, 1, Nw * len(khw) * Cin // 8, 8, 0, BF16, OUT_FILL)
            dst = dst if dtype == F32 else dst.t
            sc = None if scale is None else torch.full((1,), scale, dtype=torch.float32, device=dev)
            op = ops.pack_weight(src, dst, dtype, Nw, len(khw), Cin, N_real, C_real, swap, I2, KK, khw_t, layout, sc)
            want = R.pack64(src.cpu(), Nw, len(khw), Cin, N_real, C_real, swap, I2, KK, khw, layout, scale).float().to(TDT[dtype])
            (batch if (scale is not None or i in (3, 4)) else singles).append((op, dst, big, want, (i, scale)))
    for op, *_ in singles:
        op()
    packs = [op.pack_args for op, *_ in batch]
    if ops.is_hip:         # the large tensor's last descriptor walks all its elements with ONE block of 256 threads
        _pack_batch_op(ops, packs, lambda j, total: 1 if j == len(packs) - 1 else max(1, min(512, (total + 1023) // 1024)))()
    else:
        ops.pack_weight_batch(packs)()
    assert len(packs) >= 3
    sync(ctx)
    fill = ST_FILL if dtype == F32 else OUT_FILL
    for op, dst, big, want, tag in singles + batch:
        got = big.detach().cpu()
        assert bool((got[:GUARD] == fill).all() and (got[-GUARD:] == fill).all()), f"pack {tag}: wrote outside dst[Nw][ntaps][Cin]"
        gb, wb = bits(got[GUARD:-GUARD]), bits(want)
        nan_w = torch.isnan(want.float())
        assert bool(torch.isnan(got[GUARD:-GUARD].float())[nan_w].all()), f"pack {tag}: a NaN weight did not stay a NaN"
        diff = int(((gb != wb) & ~nan_w).sum())
        worst = max(worst, diff)
        assert diff == 0, f"pack {tag}: {diff} elements differ from round(src / scale) placed by the layout formula"
    print(f"[conv-family] pack {NAME[dtype]}: {len(singles)} single and {len(batch)} batched copies bit-identical to the float64 statement")
    return worst
