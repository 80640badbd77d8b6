"""TEST INFRASTRUCTURE: emulator statement of the e4m3 weight gradient (gan_conv_wgrad with dtype GAN_FP8, csrc/wgrad_patch_fp8.hip).

`Fp8WgradEmuOps` is tests.emulator.EmuOps plus
  * gan_wgrad_patch_splits for GAN_FP8 descriptors (never negative: where the bf16 query would group whole images it answers 0),
  * gan_conv_wgrad on e4m3 bytes: part = g_scale[b] * sum_m g8[m][n] * x8[pix(m) + tap][c], summed exactly (float64) per image, so
    what it returns differs from the bf16 path by the number format alone,
  * events that remember who recorded and who waited: every op of a built program carries `.stream` ("main" / "side"), event ops carry
    `.ev_record` / `.ev_wait`, so a test can check the order of a program without running it.
Never imported by the product package.
"""
from __future__ import annotations

import torch

from tests.emulator import EmuOps, _vfloat

FP8 = 2


class _Event:
    pass


class _SideOps:
    """The second stream of Fp8WgradEmuOps: the same statements, ops tagged stream = "side"."""

    def __init__(self, main):
        self._main = main

    def __getattr__(self, name):
        attr = getattr(self._main, name)
        if not callable(attr):
            return attr

        def call(*a, **kw):
            out = attr(*a, **kw)
            if callable(out):
                try:
                    out.stream = "side"
                except AttributeError:      # a bound method cannot carry attributes: wrap it
                    inner = out
                    out = lambda: inner()
                    out.stream = "side"
            return out
        return call


class Fp8WgradEmuOps(EmuOps):
    def side(self):
        return _SideOps(self)

    def new_event(self):
        return _Event()

    def record(self, ev):
        def op():
            return None
        op.ev_record = ev
        return op

    def wait(self, ev):
        def op():
            return None
        op.ev_wait = ev
        return op

    def wgrad_patch_splits(self, c):
        """Statement of gan_wgrad_patch_splits; GAN_FP8 descriptors: csrc/wgrad_patch_fp8.hip."""
        if c.x.dtype != FP8:
            return super().wgrad_patch_splits(c)
        if c.g.dtype != FP8 or c.ntaps != 9 or c.Cx % 64 or c.N % 128 or c.N != c.g.C:
            return 0
        if (c.x_sy, c.x_sx, c.g_sy, c.g_sx) != (1, 1, 1, 1) or c.Ho * c.Wo < 128:
            return 0
        if c.Wo < 16 or c.Wo & (c.Wo - 1) or 128 % c.Wo or c.max_tapoff != (2 * c.x.Wp + 2) * c.Cx:
            return 0
        window = (128 // c.Wo + 2) * ((c.Wo + 2 + 15) // 16 * 16)
        if window > 320 and c.Wo != 128:      # 128-wide maps: the row-ring variant
            return 0
        bps = (c.N // 128) * (c.Cx // 64)
        if c.Ho * c.Wo < 8 * 128 and c.B * bps > 256 and (c.Ho * c.Wo) % 128 == 0 and window <= 320:
            ipb = c.B * bps // 256
            while ipb > 1 and c.B % ipb:
                ipb -= 1
            if ipb > 1:                       # bf16 would put several images into a split; the per-image scale forbids it
                return 0
        if c.Ho * c.Wo < 8 * 128 and c.B > 64:
            return 0
        spi = (256 + c.B * bps - 1) // (c.B * bps)
        return max(1, min(spi, max(1, c.Ho * c.Wo // 256)))

    def conv_wgrad(self, c):
        if c.x.dtype != FP8:
            op = super().conv_wgrad(c)
            op.wgrad = c
            return op
        assert c.variant == 1 and c.g.dtype == FP8, "e4m3 operands exist on the range-patch variant only"
        spi = self.wgrad_patch_splits(c)
        assert spi > 0 and c.nsplit == c.B * spi, (spi, c.nsplit)

        def op():
            x = _vfloat(c.x).double()
            g = _vfloat(c.g).double()
            sc = torch.ones(c.B, dtype=torch.float64) if c.g_scale is None else c.g_scale[:c.B].double()
            ys, xs = c.x_y0 + torch.arange(c.Ho), c.x_x0 + torch.arange(c.Wo)
            gy, gx = c.g_y0 + torch.arange(c.Ho), c.g_x0 + torch.arange(c.Wo)
            gm = g[:, gy][:, :, gx][..., :c.N].reshape(c.B, -1, c.N)
            Wp, Cx = c.x.Wp, c.Cx
            part = torch.zeros(c.B, c.N, c.ntaps, Cx, dtype=torch.float64)
            for t, off in enumerate(c.tapoff.tolist()):
                dy, dx = (off // Cx) // Wp, (off // Cx) % Wp
                xm = x[:, ys + dy][:, :, xs + dx].reshape(c.B, -1, Cx)
                part[:, :, t] = torch.bmm(gm.transpose(1, 2), xm) * sc.view(c.B, 1, 1)
            buf = c.part.view(-1)
            n = c.N * c.ntaps * Cx
            buf[:c.nsplit * n] = 0
            # one slab per image (its first split) carries the image's sum: the scale belongs to the image
            for b in range(c.B):
                buf[b * spi * n:(b * spi + 1) * n] = part[b].reshape(-1).float()
        op.wgrad = c
        return op


# ---------------------------------------------------------------------- step-level helpers shared by the CPU and GPU tests
def run_cut_steps_fp8_wgrad(device, ops, **kw):
    """tests.cases.run_cut_steps with a trainer built as CutTrainer(..., fp8=True, fp8_wgrad=True): same inputs, oracle and tolerances."""
    from tests import cases
    orig = cases.C.CutTrainer

    def make(*a, **k):
        return orig(*a, fp8_wgrad=True, **k)
    cases.C.CutTrainer = make
    try:
        return cases.run_cut_steps(device, ops, True, amp=True, fp8=True, **kw)
    finally:
        cases.C.CutTrainer = orig


def make_trainer(device, ops, S, B, fp8, fp8_wgrad, use_aug=True):
    """The trainer tests.cases.run_cut_steps builds (same seed, same configuration), with the fp8 switches given."""
    from tests import cases
    C = cases.C
    cfg = cases.small_config()
    cfg["diffaugment"]["enable"] = use_aug
    C.set_seed(42)
    gen, disc = C.build_models(cfg, "cpu")
    kw = {"fp8_wgrad": True} if fp8_wgrad else {}
    return C.CutTrainer(gen, disc, cfg, B, S, device=device, amp=True, ops=ops, fp8=fp8, **kw)


def run_steps(tr, S, B, nsteps, device):
    """nsteps training steps on run_cut_steps' inputs and per-step seeds; returns the list of loss dicts."""
    g = torch.Generator().manual_seed(1234)
    photos = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    monets = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    out = []
    for step in range(nsteps):
        torch.manual_seed(9000 + step)
        rnd = tr.sample_randomness()
        out.append({k: float(v) for k, v in tr.train_step(step, photos.to(device), monets.to(device), rnd).items()})
    return out


def block_grads(tr):
    """fp32 weight gradients of the 18 residual convolutions after a step, block order, (first, second) per block."""
    return [conv.grad_w.detach().cpu().double().clone() for pair in tr.G.c_blk for conv in pair]


def rel_frobenius(a, b):
    return float((a - b).norm() / b.norm())


# ---------------------------------------------------------------------- launch recorder
class LaunchLog:
    """What a trainer asks its op layer to launch, in the order it builds its programs: (stream, op name, arguments).  Views and tensors are
    summarised by geometry / size, dtype and an ordinal of first appearance (the log keeps them alive, so an address is never reused);
    descriptor dataclasses field by field (fields that are None are left out, so a new optional field does not change older records)."""

    def __init__(self):
        self.entries, self._ids, self._keep = [], {}, []

    def _id(self, t):
        self._keep.append(t)
        return self._ids.setdefault(t.data_ptr(), len(self._ids))

    def summary(self, a):
        import dataclasses
        from gan_variant_research_amd.runtime import View
        if isinstance(a, View):
            return ["V", a.B, a.H, a.W, a.C, a.halo, a.dtype, self._id(a.t)]
        if torch.is_tensor(a):
            return ["T", a.numel(), str(a.dtype), self._id(a)]
        if dataclasses.is_dataclass(a) and not isinstance(a, type):
            return [type(a).__name__, {f.name: self.summary(getattr(a, f.name)) for f in dataclasses.fields(a) if getattr(a, f.name) is not None}]
        if isinstance(a, (list, tuple)):
            return [self.summary(x) for x in a]
        if isinstance(a, dict):
            return {str(k): self.summary(v) for k, v in a.items()}
        if isinstance(a, (bool, int, float, str)) or a is None:
            return a
        return type(a).__name__

    def hashed(self):
        """[stream, name, 12 hex digits of the arguments' digest] per launch: the form stored under tests/golden/."""
        import hashlib
        import json
        return [[s, n, hashlib.sha1(json.dumps(args, sort_keys=True).encode()).hexdigest()[:12]] for s, n, args in self.entries]


class RecOps:
    """Wraps an op layer: every call that returns launches (a callable or a list of them) is entered into the LaunchLog; side() / fork()
    return wrappers of their own with the stream's name.  Queries (anything returning a number) pass through unrecorded."""

    def __init__(self, inner, log=None, stream="main"):
        self._inner, self.log, self._stream = inner, log if log is not None else LaunchLog(), stream
        self._side = None

    def side(self):
        if self._side is None:
            self._side = RecOps(self._inner.side(), self.log, self._stream + ".side")
        return self._side

    def fork(self):
        return RecOps(self._inner.fork(), self.log, self._stream + ".fork")

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr):
            return attr

        def call(*a, **kw):
            out = attr(*a, **kw)
            if callable(out) or (isinstance(out, list) and out and all(callable(o) for o in out)):
                self.log.entries.append((self._stream, name, self.log.summary([list(a), kw])))
            return out
        return call


def build_step_programs(ops, S, B, fp8, fp8_wgrad=False):
    """Builds the trainer and both of its step-program sets (identity pass merged / separate) on a recording op layer; nothing is stepped."""
    rec = RecOps(ops)
    tr = make_trainer("cpu", rec, S, B, fp8, fp8_wgrad)
    tr._use_mode(True)
    tr._use_mode(False)
    return tr, rec.log
