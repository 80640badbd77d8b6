"""Every convolution launch of the benchmark's step, at the benchmark's shapes, against a float64 reference.

The launches bench.py times (CUT 256x256, batch 16, bf16; and BASELINE.json configs[4] at 512x512, batch 8, without fp8) select their
kernels, tiles and persistent grids from the batch and the map size: the range-patch kernel walks several tiles per block only past 256
tiles, the generic kernel past 512 virtual tiles, the 256-row 16-channel generic tile past 65 280 output pixels, and the weight-gradient
splits and reduction lanes follow B * H * W.  Here:
  1. a recording op layer plans the real trainer (one train_step: R1 and the merged identity pass included) and keeps a dispatch key of
     every convolution / weight-gradient launch it plans, and the ConvLayer calls (layer, direction, views) behind them;
  2. every distinct ConvLayer call is replayed on a fresh layer with random operands and checked element by element -- forward, input
     gradient, weight and bias gradient -- against cases.conv_ref64 in float64 on the GPU, within cases.derived_bound;
  3. the bound is shown to reject a reference with one tap dropped (forward, input gradient) and a weight gradient missing one image,
     for every kernel family the step uses;
  4. every key the step planned must be among the keys the replays planned (none is exempt);
  5. the persistent branches named above are reached (reach test), plus one standalone 512 -> 1 layer on the 256-row 16-channel tile;
  6. InstanceNorm and PatchNCE run their parity bodies at the step's shapes."""
import math
import zlib

import pytest
import torch

from gan_variant_research_amd import BF16, F32
from gan_variant_research_amd import cut as C
from gan_variant_research_amd.convplan import ConvLayer
from gan_variant_research_amd.runtime import Ctx, HipOps, cpad
from gan_variant_research_amd._lib import HALO_REFLECT, HALO_ZERO
from tests import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIGS = {"cut256_b16": (256, 16), "cut512_b8": (512, 8)}     # bench.py's headline; BASELINE.json configs[4] per GPU, bf16
# step keys a standalone ConvLayer cannot produce, with the reason: there are none
UNREPLAYABLE = {}


class RecordingOps(HipOps):
    """HipOps that logs a dispatch key for every convolution, weight-gradient and reduction launch it plans (its side / fork streams
    log into the same list).  Epilogue flags (act, bias, mask, statistics, chain) are not part of a key; what they change in the tiling
    (the backward chain's tap loop) shows in the range-patch variant."""

    def __init__(self, device, log, stream=None, torch_stream=None):
        super().__init__(device, stream=stream, torch_stream=torch_stream)
        self.log = log
        self._pending = None

    def _child(self):
        ts = torch.cuda.Stream(device=self.device)
        return RecordingOps(self.device, self.log, stream=ts.cuda_stream, torch_stream=ts)

    def side(self):
        if self._side is None:
            self._side = self._child()
        return self._side

    def fork(self):
        if self._fork is None:
            self._fork = self._child()
        return self._fork

    def conv_key(self, c):
        v = self.conv_igemm_variant(c)
        pv = self.conv_patch_variant(c) if c.w_frag else {}
        layout = 2 if c.win7 is not None else 1 if c.w_frag else 0
        return ("conv", c.x.dtype, layout, c.B, c.Ho, c.Wo, c.Cin, c.Nst, c.ntaps, c.in_sy, c.in_sx, c.out_sy, c.out_sx, c.tile_rows, c.tile_cols,
                pv.get("slices", 0), pv.get("static_taps", 0), v["rows"], v["cols"], v["tiles"], v["grid"])

    def conv_igemm(self, c):
        self.log.append(self.conv_key(c))
        return super().conv_igemm(c)

    def conv_wgrad(self, c):
        self._pending = ("wgrad", c.x.dtype, c.variant, c.nsplit, c.B, c.Ho, c.Wo, c.Cx, c.N, c.ntaps, c.x_sy, c.x_sx, c.g_sy, c.g_sx)
        return super().conv_wgrad(c)

    def wgrad_reduce(self, part, nsplit, N, ntaps, Cx, N_real, C_real, swap, I2, KK, khw, grad, accumulate):
        assert self._pending is not None and self._pending[3] == nsplit
        self.log.append(self._pending + (self.wgrad_reduce_lanes(nsplit, N_real, ntaps, Cx),))
        self._pending = None
        return super().wgrad_reduce(part, nsplit, N, ntaps, Cx, N_real, C_real, swap, I2, KK, khw, grad, accumulate)


def _geom(layer):
    return (int(layer.cin), int(layer.cout), layer.k, layer.s, layer.p, layer.transposed)


def _vg(v):
    return None if v is None else (v.B, v.H, v.W, v.C, v.halo)


def _record_step(S, B, monkeypatch, run_step=True):
    """Builds CutTrainer as bench.py does, runs one train_step; returns (step keys, ConvLayer calls, trainer shapes for the norm / NCE)."""
    import bench
    monkeypatch.delenv("GAN_PATCH_BN", raising=False)
    monkeypatch.delenv("GAN_PATCH_BM", raising=False)
    log, calls = [], {}
    orig = {n: getattr(ConvLayer, n) for n in ("fwd", "dgrad", "wgrad")}

    def fwd(self, x, y, act=0, mask=None, use_bias=True, stats_ws=None):
        calls.setdefault((_geom(self), self.ctx.dtype, "fwd", _vg(x), _vg(y), _vg(mask), False, False), 0)
        return orig["fwd"](self, x, y, act, mask, use_bias, stats_ws)

    def dgrad(self, dy, dx, mask=None, padded_domain=False, chain=None):
        calls.setdefault((_geom(self), self.ctx.dtype, "dgrad", _vg(dy), _vg(dx), _vg(mask), bool(padded_domain), chain is not None), 0)
        return orig["dgrad"](self, dy, dx, mask, padded_domain, chain)

    def wgrad(self, x, dy, accumulate, bias_too=True, ops=None):
        calls.setdefault((_geom(self), self.ctx.dtype, "wgrad", _vg(x), _vg(dy), None, False, False), 0)
        return orig["wgrad"](self, x, dy, accumulate, bias_too, ops)
    monkeypatch.setattr(ConvLayer, "fwd", fwd)
    monkeypatch.setattr(ConvLayer, "dgrad", dgrad)
    monkeypatch.setattr(ConvLayer, "wgrad", wgrad)
    cfg = bench.default_config()
    C.set_seed(42)
    gen, disc = C.build_models(cfg, DEV)
    tr = C.CutTrainer(gen, disc, cfg, B, S, device=DEV, amp=True, ops=RecordingOps(torch.device(DEV), log))
    if run_step:
        g = torch.Generator().manual_seed(3)
        photos, monets = ((torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(DEV) for _ in range(2))
        losses = tr.train_step(0, photos, monets, tr.sample_randomness(torch.Generator().manual_seed(9)))
        torch.cuda.synchronize()
        assert all(math.isfinite(v) for v in losses.values()) and losses["r1"] > 0.0
    for n, f in orig.items():
        monkeypatch.setattr(ConvLayer, n, f)
    nce = [_vg(tr.p2.acts[i]) for i in tr.nce_layers]
    del tr, gen, disc
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return set(log), list(calls), nce


def _filled(ctx, shape, fill):
    B, H, W, Cc, halo = shape
    v = ctx.view(B, H, W, Cc, halo)
    v.t.fill_(fill)
    return v


def _nchw(v, Cr, padded=False):
    t = v.padded() if padded else v.nhwc()
    return t[..., :Cr].permute(0, 3, 1, 2).double()


def _images(B, step=1):
    """Images whose float64 reference is computed for the forward / input gradient: all of them (step 1)."""
    return list(range(0, B, step))


def _replay(call, report, neg):
    """Runs one recorded ConvLayer call on a fresh layer (random operands, same views and flags) and checks it against float64.
    Returns the keys the replay planned."""
    (cin, cout, k, s, p, tr), dtype, op, va, vb, vmask, padded_domain, chain = call
    log = []
    ctx = Ctx(RecordingOps(torch.device(DEV), log), DEV, dtype)
    g = torch.Generator().manual_seed(zlib.crc32(repr(call).encode()))
    wshape = (cin, cout, k, k) if tr else (cout, cin, k, k)
    w = (torch.randn(wshape, generator=g) * (0.5 / (cin * k * k) ** 0.5)).to(DEV)
    b = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    gw, gb = torch.zeros_like(w), torch.zeros_like(b)
    layer = ConvLayer(ctx, w, b, gw, gb, k, s, p, tr)
    reflect = (not tr) and s == 1 and k in (3, 7)       # the generator's stride-1 layers pad by reflection (CUT config), the rest by zeros
    rnd = lambda B_, C_, H_, W_: (torch.randn(B_, C_, H_, W_, generator=g).bfloat16().float() if dtype == BF16 else torch.randn(B_, C_, H_, W_, generator=g))
    mask = _filled(ctx, vmask, 1.0) if vmask is not None else None      # LeakyReLU mask > 0 everywhere: factor 1
    if op == "fwd":
        B, H, W, _, xh = va
        x = rnd(B, cin, H, W)
        xv = cases.to_view(ctx, x, xh, HALO_REFLECT if reflect else HALO_ZERO)
        yv = ctx.view(*vb)
        ops = layer.fwd(xv, yv, mask=mask)
    elif op == "dgrad":
        B, Ho, Wo, _, dyh = va
        dy = rnd(B, cout, Ho, Wo)
        dyv = cases.to_view(ctx, dy, dyh, HALO_ZERO)
        dxv = ctx.view(*vb)
        ch = None
        if chain:
            ch = {"operand": _filled(ctx, vb, 1.0), "ws": ctx.f32(B * 96 * vb[3] * 2)}
        ops = layer.dgrad(dyv, dxv, mask=mask, padded_domain=padded_domain, chain=ch)
    else:
        B, H, W, _, xh = va
        x = rnd(B, cin, H, W)
        Ho, Wo = vb[1], vb[2]
        dy = rnd(B, cout, Ho, Wo)
        xv = cases.to_view(ctx, x, xh, HALO_REFLECT if reflect else HALO_ZERO)
        dyv = cases.to_view(ctx, dy, vb[4], HALO_ZERO)
        ops = layer.wgrad(xv, dyv, accumulate=False)
    if op != "wgrad":         # a weight gradient reads no operand copy of the weight
        ctx.ops.pack_weight_batch([o.pack_args for o in layer.repack_ops()])()
    for o in ops:
        o()
    torch.cuda.synchronize()
    keys = set(log)
    w64 = (w.bfloat16() if dtype == BF16 else w).double()
    u_out = cases.U_BF16 if dtype == BF16 else cases.U_F32
    wdrop = w64.clone()
    wdrop[:, :, k // 2, k // 2] = 0                   # one tap left out: present at every output pixel
    name = f"{op} {(cin, cout, k, s, p, tr)} {'bf16' if dtype == BF16 else 'fp32'} B{va[0]} {va[1]}x{va[2]}" + (" pd" if padded_domain else "") + (" chain" if chain else "")
    worst = 0.0
    if op in ("fwd", "dgrad"):
        got_all = _nchw(dxv, cin, padded_domain) if op == "dgrad" else _nchw(yv, cout)
        src = (dy if op == "dgrad" else x).to(DEV).double()
        x_hw = (vb[1], vb[2]) if op == "dgrad" else None
        for i in _images(src.shape[0]):
            kw = {"dy": src[i:i + 1], "x_hw": x_hw, "padded_domain": padded_domain} if op == "dgrad" else {"x": src[i:i + 1]}
            ref, A, K = cases.conv_ref64(op, k, s, p, tr, reflect, w64, **kw)
            if op == "fwd":
                ref, A = ref + b.double().view(1, -1, 1, 1), A + b.double().abs().view(1, -1, 1, 1)
            worst = max(worst, cases.assert_within_bound(got_all[i:i + 1], ref, A, K, u_out, f"{name} image {i}"))
            if i == 0:
                bad = cases.conv_ref64(op, k, s, p, tr, reflect, wdrop, **kw)[0]
                if op == "fwd":
                    bad = bad + b.double().view(1, -1, 1, 1)
                neg.setdefault(_family(keys), []).append(cases.bound_ratio(got_all[:1], bad, A, K, u_out))
    else:
        x64, dy64 = x.to(DEV).double(), dy.to(DEV).double()
        ref, A, last = 0.0, 0.0, None
        for i in range(x64.shape[0]):       # full batch, image by image; the last image's share kept for the negative control
            r, a_, _ = cases.conv_ref64("wgrad", k, s, p, tr, reflect, w64, x=x64[i:i + 1], dy=dy64[i:i + 1])
            ref, A, last = ref + r, A + a_, r
        K = (x64 if tr else dy64)[:, 0].numel()
        worst = cases.assert_within_bound(gw, ref, A, K, 0.0, f"{name} weight gradient")
        neg.setdefault(_family(keys), []).append(cases.bound_ratio(gw, ref - last, A, K, 0.0))
        Kb = dy64[:, 0].numel()
        worst = max(worst, cases.assert_within_bound(gb, dy64.sum((0, 2, 3)), dy64.abs().sum((0, 2, 3)), Kb, 0.0, f"{name} bias gradient"))
    for key in keys:
        report[key] = max(report.get(key, 0.0), worst)
    del ctx, layer, ops
    torch.cuda.empty_cache()
    return keys


def _family(keys):
    """Kernel family of a replay's launches: ('conv', layout) or ('wgrad', variant); a replay whose launches mix families gets a tuple."""
    fam = sorted({(k[0], k[2]) for k in keys})
    return fam[0] if len(fam) == 1 else tuple(fam)


FAMILY_NAMES = {("conv", 0): "generic", ("conv", 1): "range-patch", ("conv", 2): "7x7 window",
                ("wgrad", 0): "generic wgrad", ("wgrad", 1): "range-patch wgrad", ("wgrad", 2): "7x7 window wgrad"}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_bench_step_launches_match_float64(config, monkeypatch):
    S, B = CONFIGS[config]
    step_keys, calls, _ = _record_step(S, B, monkeypatch)
    report, neg, replay_keys = {}, {}, set()
    for call in calls:
        replay_keys |= _replay(call, report, neg)
    # 4. coverage: every launch of the real step was planned, with the same key, by some replay
    missing = {k for k in step_keys - replay_keys if k not in UNREPLAYABLE}
    assert not missing, f"step launches no replay reproduced: {sorted(missing)}"
    # 3. the bound rejects dropped work, in every kernel family the step uses (fwd / dgrad: a tap; wgrad: an image)
    fams = {(k[0], k[2]) for k in step_keys if k[0] in ("conv", "wgrad")}
    for fam in fams:
        ratios = neg.get(fam, [])
        assert ratios and max(ratios) > 1.0, f"{FAMILY_NAMES[fam]}: no replay where the bound rejects dropped work ({ratios})"
    print(f"\n[{config}] {len(step_keys)} step keys, {len(calls)} replayed layer calls; worst err/bound per key:")
    for key in sorted(step_keys, key=str):
        print(f"  {report.get(key, float('nan')):.3f}  {key}")
    print(f"  negative controls (max err/bound of the broken reference, per family): "
          f"{ {FAMILY_NAMES.get(f, f): round(max(r), 1) for f, r in neg.items()} }")


def test_bench_shapes_reach_every_persistent_branch(monkeypatch):
    """Across both configurations the step plans the branches that only large batches select (planning only, no step)."""
    keys = set()
    for S, B in CONFIGS.values():
        keys |= _record_step(S, B, monkeypatch, run_step=False)[0]
    conv = [k for k in keys if k[0] == "conv"]
    patch = [k for k in conv if k[2] == 1]
    generic = [k for k in conv if k[2] == 0]
    win = [k for k in conv if k[2] == 2]
    wg = [k for k in keys if k[0] == "wgrad"]
    reached = {
        "range-patch launch with > 256 tiles (blocks walk tiles)": any(k[-2] > 256 and k[-1] == 256 for k in patch),
        "generic launch with nvirt > 512 (blocks walk tiles)": any(k[-2] > 512 and k[-1] == 512 for k in generic),
        "range-patch 288-row tile": any(k[13] == 288 for k in patch),
        "range-patch 256-row tile": any(k[13] == 256 for k in patch),
        "range-patch 128-column tile (planner)": any(k[14] == 128 for k in patch),
        "range-patch 256-column tile (planner)": any(k[14] == 256 for k in patch),
        "7x7 window forward, 64 -> 3 and 3 -> 64": {k[6] for k in win} == {8, 64},
        "7x7 window weight gradient walks > 1 tile per block": any(w[2] == 2 and any(c[3] == w[4] and c[4] == w[5] and c[19] > w[3] for c in win) for w in wg),
        "reduce lanes G = 1": any(k[-1] == 1 for k in wg),
        "reduce lanes G >= 2": any(k[-1] >= 2 for k in wg),
    }
    print("\nreached:", reached)
    assert all(reached.values()), {k: v for k, v in reached.items() if not v}
    # the window forward launches one block per 16x16 tile (it is not persistent): grid == tiles
    assert all(k[-1] == k[-2] for k in win)


def test_discriminator_512_to_1_on_the_256_row_16_channel_tile():
    """4x4 512 -> 1 with B * Ho * Wo >= 65 281 (B = 16 at 68x68: 71 824 pixels): the generic kernel's 256-row tile for Nw = 16."""
    call = ((512, 1, 4, 1, 1, False), BF16, "fwd", (16, 68, 68, 512, 1), (16, 67, 67, 8, 0), None, False, False)
    report, neg = {}, {}
    keys = _replay(call, report, neg)
    assert [(k[2], k[17], k[18]) for k in keys] == [(0, 256, 16)], keys
    assert max(neg[("conv", 0)]) > 1.0
    dcall = ((512, 1, 4, 1, 1, False), BF16, "dgrad", (16, 67, 67, 8, 2), (16, 68, 68, 512, 0), None, False, False)
    wcall = ((512, 1, 4, 1, 1, False), BF16, "wgrad", (16, 68, 68, 512, 1), (16, 67, 67, 8, 2), None, False, False)
    _replay(dcall, report, neg)
    _replay(wcall, report, neg)
    print("\nworst err/bound:", {k: round(v, 3) for k, v in report.items()})


NORM_SHAPES = [(16, 256, 256, 64, 1), (16, 128, 128, 128, 1), (32, 64, 64, 256, 1), (16, 31, 31, 512, 1)]


@pytest.mark.parametrize("shape", NORM_SHAPES)
def test_instance_norm_twins_at_bench_shapes(shape):
    from tests import test_gpu_parity as GP
    GP.test_instance_norm_twins(shape, BF16)


def test_patchnce_twins_on_every_nce_map(monkeypatch):
    from tests import test_gpu_parity as GP
    _, _, nce = _record_step(256, 16, monkeypatch, run_step=False)
    assert len(nce) >= 4
    for B, H, W, Cc, halo in sorted(set(nce)):
        GP.test_patchnce_twins((B, H, W, Cc, halo, 256), BF16)
