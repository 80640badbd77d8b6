"""Generator / discriminator execution engines: explicit forward and backward *programs* over halo-NHWC buffers.

The reference builds its networks from torch.nn modules and lets autograd derive the backward pass
(GAN_Variant1/models/generator_resnet_attn.py:74-235, discriminator_patchgan.py:7-128, Basic_GAN/src/models.py:7-107).
Here every network is a fixed, hand-scheduled list of kernel launches: activations are written once in the
layout their consumer wants (reflect / zero halo materialised by the producer), InstanceNorm + ReLU + residual
add + padding are one pass, and gradients of reflection padding are folded by the consumer.
"""
from __future__ import annotations

import os

from typing import Callable, Dict, List, Optional, Sequence

import torch

from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, BF16, F32, FP8, HALO_REFLECT, HALO_ZERO
from .convplan import ConvLayer
from .runtime import IN_WS_CHUNKS, Ctx, Program, View, cpad

IN_EPS = 1e-5


def generator_keys(style: str, n_blocks: int, n_down: int = 2, reflect: bool = True):
    """state_dict key prefixes in execution order: (init, [down], [(blk_a, blk_b)], [up], out).  With zero padding the
    reference builds no pad modules (generator_resnet_attn.py:24-30,43-46,110-113,157-160), which shifts the Sequential indices."""
    if style == "cut":
        i0, ia, ib = (1, 1, 5) if reflect else (0, 0, 3)
        return (f"initial.{i0}", [f"downsample.{3*i}" for i in range(n_down)],
                [(f"res_blocks.{b}.conv_block.{ia}", f"res_blocks.{b}.conv_block.{ib}") for b in range(n_blocks)],
                [f"upsample.{3*i}" for i in range(n_down)], f"output.{i0}")
    assert style == "basic" and n_down == 2
    base = 10
    ups = base + n_blocks
    return ("net.1", ["net.4", "net.7"], [(f"net.{base+b}.block.1", f"net.{base+b}.block.5") for b in range(n_blocks)],
            [f"net.{ups}", f"net.{ups+3}"], f"net.{ups+7}")


class _Net:
    def __init__(self, ctx: Ctx, params: Dict[str, torch.Tensor], grads: Dict[str, torch.Tensor]):
        self.ctx, self.params, self.grads = ctx, params, grads
        self.layers: List[ConvLayer] = []
        self._gbufs = {}

    def _conv(self, key, k, s, p, transposed=False, need_dgrad=True) -> ConvLayer:
        w, b = self.params[key + ".weight"], self.params.get(key + ".bias")
        layer = ConvLayer(self.ctx, w, b, self.grads[key + ".weight"], self.grads.get(key + ".bias"), k, s, p, transposed, need_dgrad)
        self.layers.append(layer)
        return layer

    def repack_program(self) -> Program:
        """Refreshes every operand copy of the network after an optimiser step: ONE batched launch."""
        prog = Program("repack")
        ops = [op for layer in self.layers for op in layer.repack_ops()]
        if ops:
            prog.add(self.ctx.ops.pack_weight_batch([op.pack_args for op in ops]))
        return prog

    def gbuf(self, tag: str, B, H, W, C, halo) -> View:
        """Gradient scratch shared by every pass of this network (launches are stream-ordered)."""
        key = (tag, B, H, W, C, halo)
        v = self._gbufs.get(key)
        if v is None:
            v = self.ctx.view(B, H, W, C, halo)
            self._gbufs[key] = v
        return v

    def in_ws(self, B, C) -> torch.Tensor:
        return self.ctx.scratch("in_ws", B * IN_WS_CHUNKS * C * 2 + B * C * 2 + (B * 1024 + 32) * C)


def fp8_switches(mi_cfg: Optional[dict], amp: bool, fp8: Optional[bool], fp8_wgrad: Optional[bool]):
    """(fp8, fp8_wgrad) of a fused trainer: the keyword where given, else the config's 'mi355x' section, else False.  fp8 needs amp and
    fp8_wgrad needs fp8 (GeneratorNet has what they mean): ValueError otherwise."""
    mi = mi_cfg or {}
    fp8 = bool(mi.get("fp8", False) if fp8 is None else fp8)
    if fp8 and not amp:
        raise ValueError("fp8 convolutions exist in the bf16 (amp) mode only: fp32 is the parity mode")
    fp8_wgrad = bool(mi.get("fp8_wgrad", False) if fp8_wgrad is None else fp8_wgrad)
    if fp8_wgrad and not fp8:
        raise ValueError("fp8_wgrad needs fp8: the e4m3 weight gradient reads the e4m3 operand copies that only the fp8 forward and "
                         "input-gradient passes write")
    return fp8, fp8_wgrad


class GeneratorNet(_Net):
    """9-block ResNet generator of both trainers (CUT: biased convs; Basic_GAN: bias-free but the last)."""

    def __init__(self, ctx, params, grads, style="cut", n_blocks=9, ngf=64, in_c=3, out_c=3, need_input_grad=True, reflect=True,
                 block_act=ACT_RELU, fp8=False, fp8_wgrad=False, fp8_pow2_scales=False):
        """reflect: `padding_type` 'reflect' (the configs' value) or 'zero'; block_act: the residual blocks' activation (ReLU in the
        configs, LeakyReLU(0.2) for activation='leaky_relu', generator_resnet_attn.py:60-66).
        fp8: the residual blocks' 3x3 convolutions (generator_resnet_attn.py:33,48 -- 88 % of the generator's FLOPs) read e4m3 copies of
        their operands in the forward pass and in the input gradient (BASELINE.json configs[4]); weight gradients, InstanceNorm, the
        first / last layers and everything stored stay bf16 / fp32.  bf16 mode with reflect padding only.
        fp8_wgrad (needs fp8): the same convolutions' weight gradients run on those e4m3 copies too (ConvLayer.wgrad8: the layer input's
        copy of the forward pass and the output gradient's copy of the input gradient -- no further quantisation pass); layers whose maps
        the e4m3 weight-gradient kernel does not take (under 128 pixels) keep the bf16 one.  GPass.wgrad8_layers tells which took which.
        fp8_pow2_scales (needs fp8): the per-image scales of the output gradients' e4m3 copies are powers of two (ops.quantize_fp8_pow2)
        and the e4m3 weight gradients are told so: on many small maps (16x16 at batch >= 64) a split then sums over several whole images
        instead of falling back to the bf16 kernel.  The fused CycleGAN trainer sets it; the CUT trainer keeps the amax / 448 scales."""
        super().__init__(ctx, params, grads)
        self.fp8 = bool(fp8)
        self.fp8_wgrad = bool(fp8_wgrad)
        self.fp8_pow2_scales = bool(fp8_pow2_scales)
        assert not self.fp8_pow2_scales or self.fp8, "fp8_pow2_scales is about the e4m3 gradient copies of the fp8 mode: it needs fp8=True"
        self.passes = []
        assert not self.fp8_wgrad or self.fp8, "fp8_wgrad reads the e4m3 operand copies that only the fp8 mode writes: it needs fp8=True"
        assert not self.fp8 or (ctx.dtype == BF16 and reflect and 4 * ngf >= 128 and (4 * ngf) % 128 == 0), "fp8 blocks: bf16 mode, reflect padding, >= 128 channels"
        self.style, self.n_blocks, self.ngf, self.in_c, self.out_c = style, n_blocks, ngf, in_c, out_c
        self.reflect, self.block_act = reflect, block_act
        self.pad_mode = HALO_REFLECT if reflect else HALO_ZERO
        k_init, k_down, k_blk, k_up, k_out = generator_keys(style, n_blocks, reflect=reflect)
        self.c_init = self._conv(k_init, 7, 1, 3, need_dgrad=need_input_grad)
        self.c_down = [self._conv(k, 3, 2, 1) for k in k_down]
        self.c_blk = [(self._conv(a, 3, 1, 1), self._conv(b, 3, 1, 1)) for a, b in k_blk]
        self.c_up = [self._conv(k, 3, 2, 1, transposed=True) for k in k_up]
        self.c_out = self._conv(k_out, 7, 1, 3)
        self.n_layers = 3 + n_blocks + 2  # numbered activations of get_feature_layers

    def new_pass(self, B, H, W, last_layer: Optional[int] = None) -> "GPass":
        p = GPass(self, B, H, W, last_layer)
        self.passes.append(p)      # every pass built on this network (tests read which weight gradients took which path)
        return p


class GPass:
    """Buffers of one generator forward (+ its backward).  last_layer=None runs to the output image; otherwise the
    pass stops after that numbered activation (get_feature_layers numbering, generator_resnet_attn.py:204-233)."""

    def __init__(self, net: GeneratorNet, B, H, W, last_layer):
        assert H % 4 == 0 and W % 4 == 0
        self.net, self.B, self.H, self.W = net, B, H, W
        ctx, g, nb = net.ctx, net.ngf, net.n_blocks
        self.full = last_layer is None
        self.last = net.n_layers - 1 if self.full else last_layer
        v = ctx.view
        self.x0 = v(B, H, W, cpad(net.in_c), 3)
        # raw conv outputs, statistics and normalised activations; acts[i] = numbered activation i
        self.raw, self.stats, self.acts = [], [], []
        dims = [(H, W, g, 1)]                                   # H0: zero halo 1 (stride-2 conv, pad 1)
        dims += [(H // 2, W // 2, 2 * g, 1), (H // 4, W // 4, 4 * g, 1)]   # H1 (zero), R0 (reflect)
        dims += [(H // 4, W // 4, 4 * g, 1)] * nb               # block outputs (reflect; the last feeds ConvT: zero)
        dims += [(H // 2, W // 2, 2 * g, 1), (H, W, g, 3)]      # H3 (zero, feeds ConvT), H4 (reflect 3)
        for i, (h, w, c, halo) in enumerate(dims):
            if i > self.last:
                break
            self.acts.append(v(B, h, w, c, halo))
        n_raw = 0
        for i in range(self.last + 1):
            if 3 <= i < 3 + nb:
                h, w, c, _ = dims[i]
                self.raw.append((v(B, h, w, c, 0), v(B, h, w, c, 0)))
                self.stats.append((ctx.f32(B * c * 2), ctx.f32(B * c * 2)))
                n_raw += 1
            else:
                h, w, c, _ = dims[i]
                self.raw.append(v(B, h, w, c, 0))
                self.stats.append(ctx.f32(B * c * 2))
        self.mid = [v(B, H // 4, W // 4, 4 * g, 1) for _ in range(min(nb, max(0, self.last - 2)))]  # T_k: reflect halo 1
        if net.fp8:      # e4m3 copies of the residual convolutions' inputs (block input, T_k); gradients: see bwd_program
            self.in8 = [v(B, H // 4, W // 4, 4 * g, 1, dtype=FP8) for _ in self.mid]
            self.mid8 = [v(B, H // 4, W // 4, 4 * g, 1, dtype=FP8) for _ in self.mid]
        self.img = v(B, H, W, cpad(net.out_c), 0) if self.full else None

    def _fp8_grad_bufs(self, B, h, w, c, tag=None):
        """e4m3 copy of a residual convolution's output gradient (zero halo 2) with its per-image amax / scale: one set per network and
        shape (producer and consumer are neighbours on the main stream).  With e4m3 weight gradients the side stream reads the copy and
        its scales one block late: then `tag` names one of the alternating sets (a0 / a1 / b0 / b1, as the dy_blk_* buffers)."""
        net = self.net
        key = ("fp8g", B, h, w, c) if tag is None else ("fp8g", B, h, w, c, tag)
        bufs = net._gbufs.get(key)
        if bufs is None:
            bufs = net._gbufs[key] = (net.ctx.view(B, h, w, c, 2, dtype=FP8), net.ctx.f32(B), net.ctx.f32(B, 1.0))
        return bufs

    def halo_mode(self, i: int) -> int:
        nb = self.net.n_blocks
        if i == 2 or (3 <= i < 3 + nb - 1) or i == 4 + nb:
            return self.net.pad_mode
        return HALO_ZERO

    # ------------------------------------------------------------------ forward
    def fwd_program(self, src) -> Program:
        """src: contiguous NCHW fp32 tensor (the reference's input) or a plain C=8 image View."""
        net, ops, nb = self.net, self.net.ctx.ops, self.net.n_blocks
        prog = Program("G.fwd")
        if isinstance(src, View):
            prog.add(ops.view_copy(src, self.x0, net.pad_mode))
        else:
            prog.add(ops.nchw_to_view(src, net.in_c, self.x0, net.pad_mode))

        def norm(i, raw, stats, act, residual=None, out=None, conv=None, out8=None):
            out = self.acts[i] if out is None else out
            halo = self.halo_mode(i) if out is self.acts[i] else net.pad_mode
            ws = net.in_ws(self.B, raw.C)
            parts = conv.stats_parts if conv is not None else 0     # per-tile (sum, sum of squares) the convolution's epilogue already wrote
            if 0 < parts <= 16:      # few tiles: the apply pass adds them up itself (no statistics launch at all)
                prog.add(ops.in_apply_parts(raw, ws, parts, IN_EPS, stats, act, residual, out, halo, out8))
            elif parts > 16:
                prog.add(ops.in_stats_from_parts(ws, parts, self.B, raw.C, raw.H * raw.W, IN_EPS, stats))
                prog.add(ops.in_apply(raw, stats, act, residual, out, halo))
                if out8 is not None:
                    prog.add(ops.quantize_fp8(out, out8))
            else:                    # no fused partials: a partial pass of its own
                prog.add(ops.in_partial(raw, ws))
                prog.add(ops.in_apply_parts(raw, ws, ops.in_partial_count(raw), IN_EPS, stats, act, residual, out, halo, out8))

        prog.add(net.c_init.fwd(self.x0, self.raw[0], stats_ws=net.in_ws(self.B, self.raw[0].C)))
        norm(0, self.raw[0], self.stats[0], ACT_RELU, conv=net.c_init)
        for i in (1, 2):
            if i > self.last:
                return prog
            prog.add(net.c_down[i - 1].fwd(self.acts[i - 1], self.raw[i]))
            norm(i, self.raw[i], self.stats[i], ACT_RELU, out8=self.in8[0] if (net.fp8 and i == 2 and self.last > 2) else None)
        for k in range(nb):
            i = 3 + k
            if i > self.last:
                return prog
            (ca, cb), (ra, rb), (sa, sb) = net.c_blk[k], self.raw[i], self.stats[i]
            # fp8: the convolutions read the e4m3 operand copies, which come out of the InstanceNorm passes that produce the bf16 tensors
            f8 = net.fp8
            conv_fwd = lambda conv, x, y: (conv.fwd8 if f8 else conv.fwd)(x, y, stats_ws=net.in_ws(self.B, y.C))
            prog.add(conv_fwd(ca, self.in8[k] if f8 else self.acts[i - 1], ra))
            norm(i, ra, sa, net.block_act, out=self.mid[k], conv=ca, out8=self.mid8[k] if f8 else None)
            prog.add(conv_fwd(cb, self.mid8[k] if f8 else self.mid[k], rb))
            nxt8 = self.in8[k + 1] if (f8 and k + 1 < nb and i + 1 <= self.last) else None
            norm(i, rb, sb, ACT_NONE, residual=self.acts[i - 1], conv=cb, out8=nxt8)
        for j in range(2):
            i = 3 + nb + j
            if i > self.last:
                return prog
            prog.add(net.c_up[j].fwd(self.acts[i - 1], self.raw[i]))
            norm(i, self.raw[i], self.stats[i], ACT_RELU)
        if self.full:
            prog.add(net.c_out.fwd(self.acts[-1], self.img, ACT_TANH))
        return prog

    # ------------------------------------------------------------------ backward
    def bwd_program(self, g_img: Optional[View] = None, g_img_fold: bool = False, g_img2: Optional[View] = None,
                    hooks: Optional[Dict[int, Callable[[View], list]]] = None, accumulate: bool = False,
                    need_input_grad: bool = False, bucket: Optional[tuple] = None) -> Program:
        """Backward of this pass.  g_img (+ g_img2): gradient wrt the output image (folded over a reflect halo if
        g_img_fold).  hooks[i](g_view) returns ops that add extra gradient into activation i's gradient before it
        is consumed (PatchNCE).  Weight gradients are written (accumulate=False) or added into net.grads."""
        net, ctx, ops, nb, B = self.net, self.net.ctx, self.net.ctx.ops, self.net.n_blocks, self.B
        hooks = hooks or {}
        rf = net.reflect      # reflection padding: input gradients are produced on the padded domain and folded by their consumer
        prog = Program("G.bwd")
        H, W, g = self.H, self.W, net.ngf
        acc = accumulate

        def hook(i, gv):
            if i in hooks:
                prog.add(hooks[i](gv))

        # Weight gradients go to a second HIP stream: they are MFMA-bound and nothing on the backward chain waits for them, so
        # they overlap with the HBM-bound part of the chain (InstanceNorm backward, reflection folds: 63 % of its time hidden in a
        # two-kernel probe).  An event after the producer of dy orders the side stream; before the main stream rewrites a dy buffer
        # it waits for the side launches that read it; the program ends with a join.
        side = ops.side()
        readers = {}     # id(dy buffer) -> event recorded on the side stream after its last reader
        # power-of-two scales of the e4m3 gradient copies (GeneratorNet.fp8_pow2_scales): their quantiser, and the promise to the weight gradient
        quantize_grad = ops.quantize_fp8_pow2 if net.fp8_pow2_scales else ops.quantize_fp8
        pow2_kw = {"pow2": True} if net.fp8_pow2_scales else {}

        def wgrad_side(conv, x, dy, bias_too, g_scale=None):
            ev = ops.new_event()
            prog.add(ops.record(ev))
            prog.add(side.wait(ev))
            if dy.dtype == FP8:      # e4m3 operands (fp8_wgrad): x is the layer input's e4m3 copy, dy the scaled copy of the output gradient
                w8ops = conv.wgrad8(x, dy, g_scale, acc, ops=side, **pow2_kw)
                self.wgrad8_calls.append(w8ops[0].wgrad)
                prog.add(w8ops)
            else:
                prog.add(conv.wgrad(x, dy, acc, bias_too=bias_too, ops=side))
            done = ops.new_event()
            prog.add(side.record(done))
            readers[id(dy.t)] = done

        # fp8_wgrad: which residual convolutions' weight gradients run on e4m3 operands -- (block, "a" | "b") -> True (e4m3 kernel) / False
        # (bf16 kernel: the e4m3 one does not take the layer's maps)
        self.wgrad8_layers = {}
        self.wgrad8_calls = []      # the e4m3 weight-gradient calls of this program (runtime.WgradCall), in launch order

        def use_wgrad8(k, which, conv, x8, dy8, sc8):
            if not net.fp8_wgrad:
                return False
            ok = conv.wgrad8_call(x8, dy8, sc8, ops=side, **pow2_kw) is not None
            self.wgrad8_layers[(k, which)] = ok
            return ok

        def before_write(buf: View):
            ev = readers.pop(id(buf.t), None)
            if ev is not None:
                prog.add(ops.wait(ev))

        # bias gradients in front of a norm are column sums of dx: the norm backward leaves per-block partials in a buffer of the
        # layer's own and ONE launch at the end of the program sums them for every layer (two tiny launches per layer less on the chain)
        bias_items = []
        if not hasattr(self, "_bias_parts"):
            self._bias_parts = {}

        def bias_part(conv, raw):
            """The layer's own buffer of per-block bias partials (listed for the summing launch), or None when `conv` has no bias."""
            if conv is None or conv.grad_b is None:
                return None
            nparts = ops.in_bwd_bias_parts(raw)
            part = self._bias_parts.get(id(conv))
            if part is None:
                part = self._bias_parts[id(conv)] = ctx.f32(nparts * raw.C)
            bias_items.append((part, nparts, raw.C, conv.grad_b, conv.cout, acc))
            return part

        def inbwd(raw, stats, act, gy, fold, dx, conv=None, amax=None, parts=None):
            """InstanceNorm backward; with `conv`, its bias gradient (column sums of dx) comes out of the same pass; with `amax`, max|dx|
            per image too (the scale of dx's e4m3 copy); with `parts` = (ws, nparts, mode) the two sums were written by the producer of gy
            (an input-gradient epilogue, ConvLayer.dgrad(chain=...)) and only the apply half runs."""
            part = bias_part(conv, raw)
            if parts is not None:
                prog.add(ops.in_bwd_parts(raw, stats, act, gy, fold, dx, parts[0], parts[1], parts[2], part))
            elif amax is not None:
                prog.add(ops.in_bwd_amax(raw, stats, act, gy, fold, dx, net.in_ws(B, raw.C), part, amax))
            elif part is not None:
                prog.add(ops.in_bwd_bias_deferred(raw, stats, act, gy, fold, None, dx, net.in_ws(B, raw.C), part))
            else:
                prog.add(ops.in_bwd(raw, stats, act, gy, fold, None, dx, net.in_ws(B, raw.C)))

        i = self.last
        g_cur: Optional[View] = None   # gradient wrt acts[i]
        g_fold = False
        # Backward chain of the residual blocks (bf16, reflect padding, ReLU blocks): the input gradient of a block's second convolution
        # leaves the two sums of the ReLU'd norm's backward in its epilogue (ConvLayer.dgrad(chain=...)); gan_in_bwd_parts then applies
        # with x and g read once -- one of the five HBM-bound passes per block is gone (DESIGN 3.6 has what else was built and measured).
        use_chain = False
        if self.last >= 3 and ctx.dtype == BF16 and rf and not net.fp8 and net.block_act == ACT_RELU and not os.environ.get("GAN_NO_BWD_CHAIN"):
            r0 = self.raw[3][0]
            use_chain = net.c_blk[0][1].can_chain(net.gbuf("dy_blk_b0", B, r0.H, r0.W, r0.C, 2), net.gbuf("g_blk_p", B, r0.H, r0.W, r0.C, 1))
        self.bwd_chain = use_chain
        if self.full:
            assert g_img is not None
            dyo = net.gbuf("dy_out", B, H, W, self.img.C, 6)
            prog.add(ops.act_bwd(self.img, ACT_TANH, g_img, g_img_fold, g_img2, dyo))
            wgrad_side(net.c_out, self.acts[-1], dyo, True)
            g_cur = net.gbuf("g_h4", B, H, W, g, 3)
            prog.add(net.c_out.dgrad(dyo, g_cur, padded_domain=rf))
            g_fold = rf
        else:
            a = self.acts[i]
            g_cur = net.gbuf(f"g_act{a.H}x{a.C}", B, a.H, a.W, a.C, 0)
            prog.add(ops.zero_(g_cur.t))
        # ---- upsampling layers
        while i >= 3 + nb:
            j = i - (3 + nb)
            hook(i, g_cur)
            a_in = self.acts[i - 1]
            dy = net.gbuf(f"dy_up{j}", B, self.raw[i].H, self.raw[i].W, self.raw[i].C, 1)
            inbwd(self.raw[i], self.stats[i], ACT_RELU, g_cur, g_fold, dy, net.c_up[j])
            wgrad_side(net.c_up[j], a_in, dy, False)
            g_cur = net.gbuf(f"g_act{a_in.H}x{a_in.C}", B, a_in.H, a_in.W, a_in.C, 0)
            prog.add(net.c_up[j].dgrad(dy, g_cur))
            g_fold = False
            i -= 1
        def block_conv_bwd(k, which, conv, raw, stats, act, gy, fold, chain=False, parts=None):
            """Backward of convolution `which` ("a": first, "b": second) of residual block k behind its InstanceNorm: the norm's backward of
            gy into the convolution's output gradient dy, the weight gradient on the side stream, the input gradient dx on the (padded)
            domain.  parts: see inbwd.  chain: dx's epilogue also sums for the ReLU'd norm in front of the convolution, whose saved output
            (the convolution's input) carries the reflect halo.  -> (dx, `parts` for that norm's backward or None)."""
            x = self.mid[k] if which == "b" else self.acts[2 + k]
            dy = net.gbuf(f"dy_blk_{which}{k % 2}", B, raw.H, raw.W, raw.C, 2)   # two sets, alternating: the side stream reads them one block late
            before_write(dy)
            dx = net.gbuf("g_blk_p", B, raw.H, raw.W, raw.C, 1)
            x8 = dy8 = am8 = sc8 = chained = None
            if net.fp8:
                # input gradients on e4m3 operands: the norm backward leaves max|dY| per image, the copy is scaled by it.  With fp8_wgrad the
                # side stream reads the copy and its scales one block late as well: then the sets alternate like the dy buffers
                x8 = (self.mid8 if which == "b" else self.in8)[k]
                dy8, am8, sc8 = self._fp8_grad_bufs(B, raw.H, raw.W, raw.C, f"{which}{k % 2}" if net.fp8_wgrad else None)
            w8 = use_wgrad8(k, which, conv, x8, dy8, sc8)
            inbwd(raw, stats, act, gy, fold, dy, conv, amax=am8, parts=parts)
            if not w8:                 # the bf16 weight gradient reads dy: it goes before the quantiser
                wgrad_side(conv, x, dy, False)
            if net.fp8:
                before_write(dy8)      # fp8_wgrad: the side stream may still read this set (copy and scales) for block k + 2
                prog.add(quantize_grad(dy, dy8, am8, sc8))
                if w8:                 # after the copy exists: the e4m3 weight gradient reads it, not dy
                    wgrad_side(conv, x8, dy8, False, g_scale=sc8)
                prog.add(conv.dgrad8(dy8, dx, sc8, padded_domain=rf))
            elif chain:
                pa = ctx.scratch("bwd_parts_a", B * IN_WS_CHUNKS * raw.C * 2)
                prog.add(conv.dgrad(dy, dx, padded_domain=True, chain={"operand": x, "ws": pa}))
                chained = (pa, conv.chain_parts, 1)
            else:
                prog.add(conv.dgrad(dy, dx, padded_domain=rf))
            return dx, chained

        # ---- residual blocks
        while i >= 3:
            k = i - 3
            hook(i, g_cur)
            (ca, cb), (ra, rb), (sa, sb) = net.c_blk[k], self.raw[i], self.stats[i]
            g_mid, a_parts = block_conv_bwd(k, "b", cb, rb, sb, ACT_NONE, g_cur, False, chain=use_chain)
            g_in_p, _ = block_conv_bwd(k, "a", ca, ra, sa, net.block_act, g_mid, rf, parts=a_parts)
            g_next = net.gbuf(f"g_res{k % 2}", B, ra.H, ra.W, ra.C, 0)
            prog.add(ops.fold_add(g_cur, g_in_p, rf, g_next))
            g_cur = g_next
            if bucket is not None and k == bucket[0]:
                # Gradient bucket for data parallelism: every layer from residual block k to the output has its final gradient once
                # the launches queued so far have run -- weight gradients on the side stream, bias sums on this one.  The callback
                # (the trainer's) starts the all-reduce of that slice of the flat gradient behind BOTH, so that it overlaps the rest
                # of this backward; the side stream is only used to carry the two conditions, it does not wait for the collective.
                if bias_items:
                    prog.add(ops.bias_finalize_batch(list(bias_items)))
                    del bias_items[:]
                ev_b = ops.new_event()
                prog.add(ops.record(ev_b))
                prog.add(side.wait(ev_b))
                prog.add(bucket[1])
            i -= 1
        # ---- downsampling layers
        while i >= 1:
            hook(i, g_cur)
            a_in = self.acts[i - 1]
            dy = net.gbuf(f"dy_down{i}", B, self.raw[i].H, self.raw[i].W, self.raw[i].C, 1)
            inbwd(self.raw[i], self.stats[i], ACT_RELU, g_cur, False, dy, net.c_down[i - 1])
            wgrad_side(net.c_down[i - 1], a_in, dy, False)
            g_cur = net.gbuf(f"g_act{a_in.H}x{a_in.C}", B, a_in.H, a_in.W, a_in.C, 0)
            prog.add(net.c_down[i - 1].dgrad(dy, g_cur))
            i -= 1
        hook(0, g_cur)
        dy0 = net.gbuf("dy_init", B, H, W, g, 6 if need_input_grad else 0)
        inbwd(self.raw[0], self.stats[0], ACT_RELU, g_cur, False, dy0, net.c_init)
        wgrad_side(net.c_init, self.x0, dy0, False)
        self.g_input = None
        if need_input_grad:
            self.g_input = net.gbuf("g_x0", B, H, W, self.x0.C, 3)   # reflect: padded domain, the consumer folds (g_input_fold)
            prog.add(net.c_init.dgrad(dy0, self.g_input, padded_domain=rf))
        self.g_input_fold = rf
        if bias_items:
            prog.add(ops.bias_finalize_batch(bias_items))
        join = ops.new_event()       # everything after this program (next pass, all-reduce, optimiser) sees complete gradients
        prog.add(side.record(join))
        prog.add(ops.wait(join))
        return prog


class DiscriminatorNet(_Net):
    """PatchGAN discriminator: CUT (conv+bias+LeakyReLU, no norm) or Basic_GAN (InstanceNorm after convs 2-4)."""

    def __init__(self, ctx, params, grads, style="cut", prefix="discriminators.0.model.", ndf=64, n_layers=3, in_c=3):
        super().__init__(ctx, params, grads)
        self.style, self.in_c = style, in_c
        nconv = n_layers + 2
        if style == "cut":
            keys = [f"{prefix}{2*i}" for i in range(nconv)]
        else:
            keys = ["net.0"] + [f"net.{2+3*i}" for i in range(n_layers)] + [f"net.{2+3*n_layers}"]
        self.keys = keys
        self.chans = [in_c, ndf] + [ndf * min(2**n, 8) for n in range(1, n_layers)] + [ndf * min(2**n_layers, 8), 1]
        self.strides = [2] * n_layers + [1, 1]
        self.convs = [self._conv(k, 4, s, 1) for k, s in zip(keys, self.strides)]
        self.nconv = nconv

    def new_pass(self, B, H, W) -> "DPass":
        return DPass(self, B, H, W)


class DPass:
    def __init__(self, net: DiscriminatorNet, B, H, W):
        self.net, self.B, self.H, self.W = net, B, H, W
        ctx = net.ctx
        self.x = ctx.view(B, H, W, cpad(net.in_c), 1)     # zero halo 1; filled by DiffAugment / layout conversion
        self.acts, self.raw, self.stats = [], [], []
        h, w = H, W
        for li in range(net.nconv):
            s = net.strides[li]
            h, w = (h + 2 - 4) // s + 1, (w + 2 - 4) // s + 1
            c = cpad(net.chans[li + 1])
            last = li == net.nconv - 1
            self.acts.append(ctx.view(B, h, w, c, 0 if last else 1))
            normed = net.style == "basic" and 0 < li < net.nconv - 1
            self.raw.append(ctx.view(B, h, w, c, 0) if normed else None)
            self.stats.append(ctx.f32(B * c * 2) if normed else None)
        self.logits = self.acts[-1]

    def fwd_program(self) -> Program:
        net, ops = self.net, self.net.ctx.ops
        prog = Program("D.fwd")
        xin = self.x
        for li, conv in enumerate(net.convs):
            last = li == net.nconv - 1
            if self.raw[li] is not None:
                prog.add(conv.fwd(xin, self.raw[li]))
                prog.add(ops.in_stats(self.raw[li], IN_EPS, self.stats[li], net.in_ws(self.B, self.raw[li].C)))
                prog.add(ops.in_apply(self.raw[li], self.stats[li], ACT_LRELU, None, self.acts[li], HALO_ZERO))
            else:
                prog.add(conv.fwd(xin, self.acts[li], ACT_NONE if last else ACT_LRELU))
            xin = self.acts[li]
        return prog

    def r1_first(self, scratch: torch.Tensor) -> Program:
        """First-order half of R1 (DFamilyPass.r1_program) after this pass's forward: g = d sum D(x) / dx into self.g_input with the LeakyReLU
        masks fused in the dgrad epilogues, the per-layer output gradients (delta_i) kept for r1_second."""
        net, ops, B = self.net, self.net.ctx.ops, self.B
        assert net.style == "cut", "R1 is part of the CUT trainer (no norm layers in its discriminator)"
        pr = Program("R1.first")
        lg = self.logits
        ones = net.gbuf("r1_ones", B, lg.H, lg.W, lg.C, 2)
        pr.add(ops.patch_loss(lg, 2, 0.0, -float(B * lg.H * lg.W), scratch, ones))   # d(sum D)/dlogits = 1
        self._r1_deltas: List[View] = []
        pr.add(self.bwd_program(ones, wgrad=False, need_input_grad=True, keep=self._r1_deltas))
        return pr

    def r1_second(self, u: View) -> Program:
        """Second-order half: the weight gradients of <u_0, g(theta)> by the linearised forward u_i = mask_i * (W_i * u_{i-1}) from
        u_0 = `u` (zero halo 1), with dW_i = wgrad(u_{i-1}, delta_i).  Bias gradients are zero except the last bias, whose gradient is None
        in the reference (the caller skips it)."""
        net, ctx, B = self.net, self.net.ctx, self.B
        pr = Program("R1.second")
        deltas = self._r1_deltas
        for li, conv in enumerate(net.convs):
            delta = deltas[len(deltas) - 1 - li]
            pr.add(conv.wgrad(u, delta, accumulate=False, bias_too=False))
            if li == net.nconv - 1:
                break
            a = self.acts[li]
            nxt = ctx.view(B, a.H, a.W, a.C, 1)
            pr.add(conv.fwd(u, nxt, ACT_NONE, mask=a, use_bias=False))
            u = nxt
        return pr

    def grad_logits_view(self) -> View:
        """Where the loss writes dL/dlogits: zero halo 2 (= k-1-p of the last 4x4 s1 p1 conv's input gradient)."""
        lg = self.logits
        return self.net.gbuf("g_logits", self.B, lg.H, lg.W, lg.C, 2)

    def bwd_program(self, g_logits: View, wgrad: bool = True, accumulate: bool = False, need_input_grad: bool = False,
                    keep: Optional[list] = None, write_only: Sequence[int] = (),
                    hooks: Optional[Dict[int, Callable[[View], list]]] = None) -> Program:
        """Backward from dL/dlogits.  keep: if a list, the per-layer output gradients (delta_i) are appended to it and
        live in dedicated buffers (R1's second-order pass needs them).  write_only: indices of convolutions whose weight gradient is
        written even when `accumulate` (spectral norm's dL/dW_sn scratch); their bias gradients still follow `accumulate`.
        hooks[i](g_view) returns ops queued right after the launch that wrote g_view, the gradient of activation i BEFORE its LeakyReLU
        (the input gradient with the mask fused), and before the next layer's weight or input gradient reads it: a loss on acts[i] adds
        its gradient, times LeakyReLU'(acts[i]), there (feature matching) -- GPass.bwd_program's contract.  Style "cut" only."""
        net, ops, B = self.net, self.net.ctx.ops, self.B
        hooks = hooks or {}
        assert not hooks or net.style == "cut", "hooks sit behind a fused LeakyReLU mask: Basic_GAN's activations pass through InstanceNorm"
        assert all(0 <= i < net.nconv - 1 for i in hooks), "hooks: the logits are no feature"
        prog = Program("D.bwd")
        dy = g_logits
        self.g_input = None
        # The discriminator's weight gradients stay on its own stream: they are 2 % of the step, and a fourth compute stream would
        # share a hardware queue with another one as soon as RCCL adds its stream (HIP multiplexes streams onto four queues;
        # measured: the discriminator's stream landed on the main stream's queue and the step lost 1.1 ms)
        for li in range(net.nconv - 1, -1, -1):
            conv = net.convs[li]
            xin = self.acts[li - 1] if li > 0 else self.x
            if keep is not None:
                keep.append(dy)
            if wgrad:
                if li in write_only:
                    prog.add(conv.wgrad(xin, dy, False, bias_accumulate=accumulate))
                else:
                    prog.add(conv.wgrad(xin, dy, accumulate))
            if li == 0:
                if need_input_grad:
                    self.g_input = net.gbuf("g_dx", B, self.H, self.W, self.x.C, 0)
                    prog.add(conv.dgrad(dy, self.g_input))
                break
            prev = net.convs[li - 1]
            halo = 2 if prev.s == 1 else 1   # what the previous conv's input gradient needs from its dY
            a = self.acts[li - 1]
            tag = f"d_act{li-1}" + ("_keep" if keep is not None else "")
            if self.raw[li - 1] is None:
                nxt = net.gbuf(tag, B, a.H, a.W, a.C, halo)
                prog.add(conv.dgrad(dy, nxt, mask=a))             # LeakyReLU' fused in the epilogue
            else:
                g_a = net.gbuf(f"g_dact{li-1}", B, a.H, a.W, a.C, 0)
                prog.add(conv.dgrad(dy, g_a))
                nxt = net.gbuf(tag, B, a.H, a.W, a.C, halo)
                prog.add(ops.in_bwd(self.raw[li - 1], self.stats[li - 1], ACT_LRELU, g_a, False, None, nxt, net.in_ws(B, a.C)))
            if li - 1 in hooks:
                prog.add(hooks[li - 1](nxt))
            dy = nxt
        return prog


# ------------------------------------------------------------------------------------------------ multiscale / spectral norm
SN_EPS = 1e-12          # torch.nn.utils.spectral_norm default


class SpectralNorm:
    """(u, v, sigma) of every spectral-norm convolution of a discriminator, all scales (discriminator_patchgan.py:21-23), for the fused
    trainer: one gan_spectral_norm_batch_fwd per D forward (a power iteration, sigma and the snapshots its backward reads) and one
    gan_spectral_norm_batch_bwd per weight-gradient pass.  The convolutions' weight gradients (dL/dW_sn) land in the per-layer
    scratch `G`; the backward turns them into dL/dweight_orig in the optimiser's block.  W_sn itself is never formed: the operand
    copies are packed from weight_orig with scale = sigma (ConvLayer.pack_scale)."""

    def __init__(self, ctx: Ctx, keys: Sequence[str], params: Dict[str, torch.Tensor], grads: Dict[str, torch.Tensor],
                 buffers: Dict[str, torch.Tensor]):
        """keys: convolution prefixes; params / grads hold `<key>.weight_orig`, buffers `<key>.weight_u` / `<key>.weight_v` (device
        fp32, updated in place)."""
        self.ctx, self.keys = ctx, list(keys)
        ops = ctx.ops
        self.entries, self.G, self.sigma = [], {}, {}
        for k in self.keys:
            W = params[k + ".weight_orig"]
            h, w = W.shape[0], W.numel() // W.shape[0]
            e = {"W": W, "u": buffers[k + ".weight_u"], "v": buffers[k + ".weight_v"], "sigma": ctx.f32(1, 1.0), "u_snap": ctx.f32(h),
                 "v_snap": ctx.f32(w), "G": torch.zeros_like(W), "dW": grads[k + ".weight_orig"],
                 "ws": ctx.f32(ops.spectral_norm_batch_ws_floats(h, w))}
            self.entries.append(e)
            self.G[k], self.sigma[k] = e["G"], e["sigma"]
        self._fwd = ops.spectral_norm_batch_fwd(self.entries, True, SN_EPS)
        self._bwd = {a: ops.spectral_norm_batch_bwd(self.entries, a) for a in (False, True)}

    def fwd_op(self):
        return self._fwd

    def bwd_op(self, accumulate: bool):
        return self._bwd[bool(accumulate)]




class DiscriminatorFamilyNet:
    """The discriminator family of both trainers and of the module API: one PatchGAN net per key prefix, scale s on the input
    average-pooled s times -- MultiscaleDiscriminator's `num_scales` CUT nets (discriminator_patchgan.py:75-116, prefixes
    discriminators.{s}.model.) or Basic_GAN's single NLayerDiscriminator (Basic_GAN/src/models.py:67-101, one prefix).  A convolution is
    spectral-normalised exactly when its key is in `sn.keys`: all of them in the CUT family, the bias-free middle ones (net.2 / net.5 /
    net.8) in Basic_GAN's.  Those read weight_orig packed with scale sigma and write dL/dW_sn into `sn.G`; every forward packs their operand
    copies itself after its power iteration, the repack after an optimiser step covers the plain ones.  With one scale and no spectral norm
    every program is the single DiscriminatorNet's."""

    def __init__(self, ctx: Ctx, params: Dict[str, torch.Tensor], grads: Dict[str, torch.Tensor], style: str, prefixes: Sequence[str],
                 ndf=64, n_layers=3, in_c=3, sn: Optional[SpectralNorm] = None):
        self.ctx, self.sn, self.in_c = ctx, sn, in_c
        sn_keys = sn.keys if sn is not None else []
        if sn_keys:
            params, grads = dict(params), dict(grads)
            for k in sn_keys:
                params[k + ".weight"], grads[k + ".weight"] = params[k + ".weight_orig"], sn.G[k]
        self.nets = [DiscriminatorNet(ctx, params, grads, style, p, ndf, n_layers, in_c) for p in prefixes]
        self.nconv = self.nets[0].nconv
        self.sn_layers = [[i for i, k in enumerate(net.keys) if k in sn_keys] for net in self.nets]      # per scale
        assert sum(len(idx) for idx in self.sn_layers) == len(sn_keys), ([net.keys for net in self.nets], sn_keys)
        for net, idx in zip(self.nets, self.sn_layers):
            for i in idx:
                net.convs[i].pack_scale = sn.sigma[net.keys[i]]
        self._pack = None

    def _copies(self, spectral: bool):
        return [op.pack_args for net, idx in zip(self.nets, self.sn_layers) for i, conv in enumerate(net.convs) if (i in idx) == spectral
                for op in conv.repack_ops()]

    def repack_program(self) -> Program:
        """Operand copies of the plain convolutions after an optimiser step: one batched launch (none when every convolution is
        normalised: those copies depend on the sigma of the next forward, which packs them itself)."""
        prog = Program("repack")
        copies = self._copies(False)
        if copies:
            prog.add(self.ctx.ops.pack_weight_batch(copies))
        return prog

    def refresh_pack(self):
        """(Re)builds the pack every forward runs over the normalised convolutions' copies planned so far; call after planning passes."""
        if self.sn is not None:
            self._pack = self.ctx.ops.pack_weight_batch(self._copies(True))

    def new_pass(self, B, H, W) -> "DFamilyPass":
        return DFamilyPass(self, B, H, W)


class DFamilyPass:
    """Buffers of one forward (+ backward) of the family: one DPass per scale."""

    def __init__(self, net: DiscriminatorFamilyNet, B, H, W):
        self.net, self.B, self.H, self.W = net, B, H, W
        self.dps = []
        for n in net.nets:
            self.dps.append(n.new_pass(B, H, W))
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1       # AvgPool2d(3, 2, 1)
        self.x = self.dps[0].x
        self.logits = [dp.logits for dp in self.dps]
        self.g_input = None

    def fwd_program(self, spectral: bool = True) -> Program:
        """With spectral norm: one power iteration over every normalised convolution, the pack of their operand copies with
        scale = sigma, then the scales.  spectral=False: the pools and the scales only, on the operand copies the last pack filled (a second
        forward through the same weights, e.g. the real branch of feature matching: one power iteration per step, not two)."""
        net, ops = self.net, self.net.ctx.ops
        prog = Program("D.family.fwd")
        if net.sn is not None and spectral:
            prog.add(net.sn.fwd_op())
            prog.add(lambda: net._pack())
        for s, dp in enumerate(self.dps):
            if s > 0:
                prog.add(ops.avgpool_fwd(self.dps[s - 1].x, dp.x))
            prog.add(dp.fwd_program())
        return prog

    def grad_logits_views(self) -> List[View]:
        return [dp.grad_logits_view() for dp in self.dps]

    def _pool_input_grads(self) -> list:
        """dL/dx_i += pool^T dL/dx_{i+1}, down to scale 0."""
        ops = self.net.ctx.ops
        return [ops.avgpool_bwd(self.dps[i + 1].g_input, self.dps[i].g_input, True) for i in range(len(self.dps) - 2, -1, -1)]

    def bwd_program(self, g_logits: Sequence[View], wgrad: bool = True, accumulate: bool = False, need_input_grad: bool = False,
                    hooks: Optional[Sequence[dict]] = None) -> Program:
        """Per-scale backward; input gradients summed down to scale 0 through the pools (self.g_input).  The normalised convolutions'
        weight gradients (dL/dW_sn) overwrite the scratch and one batched spectral-norm backward adds / writes dL/dweight_orig (it reads
        the snapshots of this pass's own forward: run it before the next); biases and plain weights take theirs directly.
        hooks: one dict per scale, DPass.bwd_program's."""
        sn = self.net.sn
        prog = Program("D.family.bwd")
        assert hooks is None or len(hooks) == len(self.dps)
        for s, (dp, gl, idx) in enumerate(zip(self.dps, g_logits, self.net.sn_layers)):
            prog.add(dp.bwd_program(gl, wgrad=wgrad, accumulate=accumulate, need_input_grad=need_input_grad, write_only=idx,
                                    hooks=None if hooks is None else hooks[s]))
        if need_input_grad:
            prog.add(self._pool_input_grads())
            self.g_input = self.dps[0].g_input
        if wgrad and sn is not None:
            prog.add(sn.bwd_op(accumulate))
        return prog

    def r1_program(self, scale: float, loss: torch.Tensor, scratch: torch.Tensor) -> Program:
        """R1 penalty (train_cutpp.py:165-203) once this pass's input is in place: *loss = mean_b sum_chw (d sum D(x) / dx)^2 and the weight
        gradients of scale * r1, as an explicit second-order program (no autograd graph).  With K scales D_total(x) = sum_i sum D_i(P^i x)
        (P = the average pool), so g = sum_i (P^i)^T g_i and d r1 / d theta_i = <(2 / B) P^i g, d g_i / d theta_i>: the forward (with its
        power iteration and pack), every scale's first-order half, the input gradients folded back through the pools into g and reduced
        (u_0 = scale * 2 g / B), then each scale's second-order half seeded with u_0 pooled down to its resolution; with spectral norm one
        batched backward."""
        net, ctx, ops = self.net, self.net.ctx, self.net.ctx.ops
        pr = Program("R1")
        pr.add(self.fwd_program())
        for dp in self.dps:
            pr.add(dp.r1_first(scratch))
        pr.add(self._pool_input_grads())
        us = [ctx.view(self.B, dp.H, dp.W, dp.x.C, 1) for dp in self.dps]
        pr.add(ops.r1_reduce(self.dps[0].g_input, net.in_c, scale, loss, us[0], ctx.scratch("r1_ws", 1024)))
        for i, dp in enumerate(self.dps):
            if i > 0:
                pr.add(ops.avgpool_fwd(us[i - 1], us[i]))
            pr.add(dp.r1_second(us[i]))
        if net.sn is not None:
            pr.add(net.sn.bwd_op(False))
        return pr
