"""The batched spectral-norm kernels (gan_spectral_norm_batch_fwd / _bwd, the scaled operand pack) and the fused CutTrainer with
several discriminator scales and spectral norm, on the MI355X."""
import pytest
import torch

from gan_variant_research_amd import cut as C
from gan_variant_research_amd._lib import BF16, F32
from tests.spectral_ref64 import module_step64 as _ref64          # the float64 statement lives with the spectral-norm family

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

# the discriminator's matrices at ndf=64 (h x w = Cout x Cin*16), three scales, plus a w that is not a multiple of 256 and a tall one
D_SHAPES = [(64, 48), (128, 1024), (256, 2048), (512, 4096), (1, 8192)]
EXTRA = [(40, 300), (100, 24)]


def _ops():
    from gan_variant_research_amd.runtime import HipOps
    ops = HipOps(torch.device(DEV))
    ops.bind()
    return ops


def _entries(ops, shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in shapes:
        W = torch.randn(h, w, generator=g) * 0.05
        u = torch.nn.functional.normalize(torch.randn(h, generator=g), dim=0, eps=1e-12)
        v = torch.nn.functional.normalize(torch.randn(w, generator=g), dim=0, eps=1e-12)
        G = torch.randn(h, w, generator=g)
        dW0 = torch.randn(h, w, generator=g)
        dev = lambda t: t.to(DEV).contiguous()
        out.append({"W": dev(W), "u": dev(u), "v": dev(v), "sigma": torch.zeros(1, device=DEV), "u_snap": torch.zeros(h, device=DEV),
                    "v_snap": torch.zeros(w, device=DEV), "G": dev(G), "dW": dev(dW0),
                    "ws": torch.zeros(ops.spectral_norm_batch_ws_floats(h, w), device=DEV), "host": (W, u, v, G, dW0)})
    return out


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("power_iter", [True, False])
def test_batched_spectral_norm_vs_float64(power_iter):
    ops = _ops()
    shapes = D_SHAPES * 3 + EXTRA                      # 15 descriptors as at three scales, plus the odd shapes
    es = _entries(ops, shapes)
    fwd = ops.spectral_norm_batch_fwd(es, power_iter, 1e-12)
    bwd = ops.spectral_norm_batch_bwd(es, accumulate=False)
    bwd_acc = ops.spectral_norm_batch_bwd(es, accumulate=True)
    fwd()
    bwd()
    torch.cuda.synchronize()
    for (h, w), e in zip(shapes, es):
        W, u0, v0, G, dW0 = e["host"]
        u, v, sigma, dW = _ref64(W, u0, v0, G, power_iter)
        what = f"{h}x{w}"
        assert _rel(e["u"], u) < 2e-5 and _rel(e["v"], v) < 2e-5, what
        assert torch.equal(e["u_snap"], e["u"]) and torch.equal(e["v_snap"], e["v"]), what
        assert abs(float(e["sigma"]) - float(sigma)) <= 2e-5 * abs(float(sigma)), what
        assert _rel(e["dW"], dW) < 5e-5, what
    first = [e["dW"].clone() for e in es]
    bwd_acc()
    torch.cuda.synchronize()
    for e, f in zip(es, first):
        assert _rel(e["dW"], 2 * f) < 1e-6


def test_batched_spectral_norm_is_deterministic():
    ops = _ops()
    shapes = D_SHAPES * 3 + EXTRA
    runs = []
    for _ in range(2):
        es = _entries(ops, shapes, seed=3)
        f, b = ops.spectral_norm_batch_fwd(es, True, 1e-12), ops.spectral_norm_batch_bwd(es, False)
        f(); b(); f(); b()
        torch.cuda.synchronize()
        runs.append([torch.cat([e[k].reshape(-1) for k in ("u", "v", "sigma", "dW")]).cpu() for e in es])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_pack_with_sigma_equals_pack_of_w_sn():
    """The bf16 operand copy packed from weight_orig with scale = sigma equals the per-layer path's copy packed from W_sn (1 ulp)."""
    from gan_variant_research_amd.convplan import ConvLayer
    from gan_variant_research_amd.runtime import Ctx
    ops = _ops()
    for dtype in (BF16, F32):
        ctx = Ctx(ops, DEV, dtype)
        g = torch.Generator().manual_seed(5)
        for cin, cout in ((3, 64), (256, 512), (512, 1)):
            W = (torch.randn(cout, cin, 4, 4, generator=g) * 0.05).to(DEV)
            b = torch.zeros(cout, device=DEV)
            u = torch.nn.functional.normalize(torch.randn(cout, generator=g), dim=0).to(DEV)
            v = torch.nn.functional.normalize(torch.randn(cin * 16, generator=g), dim=0).to(DEV)
            sigma, Wsn, ws = torch.zeros(1, device=DEV), torch.zeros_like(W), torch.zeros(ops.spectral_norm_ws_floats(cout, cin * 16), device=DEV)
            ops.spectral_norm_fwd(W, u, v, True, 1e-12, sigma, Wsn, ws)()
            layers = []
            for src, scale in ((W, sigma), (Wsn, None)):
                L = ConvLayer(ctx, src, b, torch.zeros_like(W), torch.zeros_like(b), 4, 2, 1)
                L.pack_scale = scale
                x = ctx.view(2, 32, 32, max(8, 1 << (cin - 1).bit_length()), 1)
                y = ctx.view(2, 16, 16, max(8, 1 << (cout - 1).bit_length()), 1)
                L.fwd(x, y)
                dy = ctx.view(2, 16, 16, y.C, 1)
                L.dgrad(dy, ctx.view(2, 32, 32, x.C, 0))
                ops.pack_weight_batch([op.pack_args for op in L.repack_ops()])()
                layers.append(L)
            torch.cuda.synchronize()
            for pa, pb in zip(layers[0].packs, layers[1].packs):
                for a, c in ((pa._w, pb._w), (pa._wf, pb._wf)):
                    if a is None:
                        continue
                    d = (a.view(torch.int16 if dtype == BF16 else torch.int32).long() - c.view(torch.int16 if dtype == BF16 else torch.int32).long()).abs()
                    assert int(d.max()) <= 1, (dtype, cin, cout)


def test_fused_trainer_sn2_golden_hip():
    from tests.test_dfamily_cpu import fused_golden_sn2_case
    fused_golden_sn2_case(DEV, None, 1e-3, 2e-3)


def test_fused_trainer_dfamily_bf16_bench_maps_vs_module_step(monkeypatch):
    """bf16, three scales + spectral norm at 256x256, B=2: one fused step vs module_step.train_step on the same kernels."""
    from gan_variant_research_amd import losses as L
    from tests.test_dfamily_cpu import fused_vs_module_case
    monkeypatch.setattr(L, "_PLANS", {})
    fused_vs_module_case(DEV, 3, True, 256, 1, _ops, amp=True, loss_rtol=4e-2, loss_atol=4e-2, ptol=1e-3, uv_tol=1e-2)


def test_fused_trainer_dfamily_matches_module_step_fp32_hip(monkeypatch):
    from gan_variant_research_amd import losses as L
    from tests.test_dfamily_cpu import fused_vs_module_case
    monkeypatch.setattr(L, "_PLANS", {})
    fused_vs_module_case(DEV, 2, True, 64, 3, _ops)


@pytest.mark.parametrize("num_scales,sn,S", [(2, False, 72), (1, True, 36)])
def test_fused_trainer_dfamily_on_odd_maps_hip(monkeypatch, num_scales, sn, S):
    """9x9 maps under the third 4x4 stride-2 layer of every scale (72 -> 36 -> 18 -> 9; pooled 36 -> 18 -> 9 -> 4), and one spectral-norm
    scale at 36: one fp32 step, fused trainer against module_step.train_step on the same kernels."""
    from gan_variant_research_amd import losses as L
    from tests.test_dfamily_cpu import fused_vs_module_case
    monkeypatch.setattr(L, "_PLANS", {})
    fused_vs_module_case(DEV, num_scales, sn, S, 1, _ops)


def test_multistream_dfamily_step_is_deterministic():
    """Two runs of the multi-stream step (discriminator stream, weight-gradient side stream) give bit-identical losses and parameters."""
    from tests.test_dfamily_cpu import _inputs, dfamily_config
    outs = []
    for _ in range(2):
        cfg = dfamily_config(3, True)
        C.set_seed(42)
        gen, disc = C.build_models(cfg, "cpu")
        tr = C.CutTrainer(gen, disc, cfg, 2, 128, device=DEV, amp=True)
        photos, monets = _inputs(2, 128)
        losses = []
        for step in range(2):
            torch.manual_seed(9000 + step)
            losses.append(tr.train_step(step, photos.to(DEV), monets.to(DEV), tr.sample_randomness()))
        tr._device_sync()
        outs.append((losses, tr.opt_D.flat_p.cpu(), tr.opt_G.flat_p.cpu(), {k: v.cpu() for k, v in tr.d_buffers.items()}))
        del tr
    (la, da, ga, ba), (lb, db, gb, bb) = outs
    assert la == lb
    assert torch.equal(da, db) and torch.equal(ga, gb)
    for k in ba:
        assert torch.equal(ba[k], bb[k]), k
