"""Forward-only generator inference (GAN_Variant1/generate_folder.py:112-252) on the HIP kernels.

`load_generator` takes the reference's checkpoints (or this package's: same layout) and prefers the EMA weights exactly as
generate_folder.py:125-170 does; `stylize` is the tensor-level body of `stylize_folder` (:207-252): G(x) then
clamp -> *0.5 + 0.5 -> *255 -> round -> uint8 (:183-185).  `stylize_hwc` is the same with the conversion and the HWC turn PIL needs
fused into one kernel after the generator's last layer (gan_view_to_u8_hwc), `stylize_images` puts the device input pipeline with
Pillow's BILINEAR taps (:175-180) in front of it.  JPEG / PNG decoding and JPEG encoding stay in PIL on the host; `stylize_folder`
walks a PIL-readable folder, with the resize and both conversions on the host (the default) or on the device (`device_io=True`).
The command line is generate_folder.py next to this file.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Iterable, Optional, Sequence

import torch

from ._lib import BF16, F32
from .cut import ResNetGenerator

_LEGACY_KEYS = ("ema_state_dict", "G_ema", "G_state_dict", "state_dict")


def pick_state_dict(ckpt: Dict) -> Dict[str, torch.Tensor]:
    """generate_folder.py:125-170: EMA shadow, then 'generator', then legacy names, then a raw / nested state dict."""
    ema = ckpt.get("ema_G")
    if isinstance(ema, dict) and isinstance(ema.get("shadow"), dict):
        return ema["shadow"]
    if isinstance(ckpt.get("generator"), dict):
        return ckpt["generator"]
    for k in _LEGACY_KEYS:
        if isinstance(ckpt.get(k), dict):
            return ckpt[k]
    if ckpt and all(isinstance(v, torch.Tensor) for v in ckpt.values()):
        return ckpt
    for v in ckpt.values():
        if isinstance(v, dict) and v and all(isinstance(x, torch.Tensor) for x in v.values()):
            return v
    raise KeyError(f"no generator state_dict in checkpoint (keys: {list(ckpt)[:10]})")


def is_cyclegan_checkpoint(ckpt: Dict) -> bool:
    """The dict Basic_GAN/src/train.py:127-137 saves (basic.CycleGANTrainer.save_checkpoint): both generators under their names."""
    return isinstance(ckpt.get("G_A2B"), dict) and isinstance(ckpt.get("G_B2A"), dict)


def _basic_generator(sd: Dict[str, torch.Tensor], device):
    """basic.ResnetGenerator of the architecture the keys tell (models.py:23-65): the residual blocks are net.10 .. net.{9+n}, the
    first convolution net.1 has ngf output channels.  The state dict is loaded strictly."""
    from .basic import ResnetGenerator
    n_blocks = sum(1 for k in sd if k.startswith("net.") and k.endswith(".block.1.weight"))
    G = ResnetGenerator(3, 3, int(sd["net.1.weight"].shape[0]), n_blocks).to(device)
    G.load_state_dict(sd, strict=True)
    return G


def load_generator(ckpt_path: str, device: str = "cuda", ngf: int = 64, n_blocks: int = 9, bf16: bool = True, use_graph: bool = False,
                   which: str = "G_A2B"):
    """generate_folder.py:189-205.  The file is read with weights_only=True (tensors and plain containers; nothing is unpickled).
    A CycleGAN checkpoint (keys G_A2B and G_B2A) yields `basic.ResnetGenerator` holding `ckpt[which]`, its width and depth read from the
    keys (`ngf` / `n_blocks` are not consulted); every other checkpoint yields the CUT `ResNetGenerator` as the reference loads it."""
    ckpt = torch.load(ckpt_path, map_location=device, weights_only=True)
    if not isinstance(ckpt, dict):
        raise ValueError(f"Checkpoint {ckpt_path} is not a dict; got {type(ckpt)}")
    if is_cyclegan_checkpoint(ckpt):
        if which not in ("G_A2B", "G_B2A"):
            raise ValueError(f"which = {which!r}: a CycleGAN checkpoint holds G_A2B and G_B2A")
        G = _basic_generator(ckpt[which], device)
    else:
        G = ResNetGenerator(3, 3, ngf, n_blocks).to(device)
        missing, unexpected = G.load_state_dict(pick_state_dict(ckpt), strict=False)
        if missing or unexpected:
            print(f"[WARN] generator state_dict: {len(missing)} missing, {len(unexpected)} unexpected keys (e.g. {(list(missing) + list(unexpected))[:4]})")
    G.eval()
    for p in G.parameters():
        p.requires_grad_(False)
    G.compute_dtype = BF16 if bf16 else F32      # the reference runs inference under autocast (:237)
    # use_graph: forward-only passes replay one hipGraph per input shape (autograd._GenBridge.forward).  Off by default: on ROCm 7.2 the
    # replay of the ~110-node graph is slower than the eager launches at small batch (1.70 vs 1.14 ms at B=1, equal at B=16; tools/bench_infer.py)
    G.use_graph = use_graph
    return G


def to_uint8(y: torch.Tensor) -> torch.Tensor:
    """[-1,1] -> uint8, generate_folder.py:183-185 (stays on the device; the caller moves it)."""
    return y.clamp(-1, 1).mul(0.5).add(0.5).mul(255).round().byte()


@torch.inference_mode()
def stylize(G: ResNetGenerator, x: torch.Tensor) -> torch.Tensor:
    """(B,3,H,W) fp32 in [-1,1] on the GPU -> (B,3,H,W) uint8 on the GPU."""
    return to_uint8(G(x))


@torch.inference_mode()
def stylize_hwc(G: ResNetGenerator, x: torch.Tensor) -> torch.Tensor:
    """(B,3,H,W) fp32 in [-1,1] on the GPU -> (B,H,W,3) uint8 on the GPU: `stylize(G, x).permute(0, 2, 3, 1)`, bit for bit, without
    the fp32 NCHW tensor, its clone and the elementwise launches in between."""
    return G.forward_u8(x)


@torch.inference_mode()
def stylize_images(G: ResNetGenerator, images: Sequence[torch.Tensor], img_size: int = 256) -> torch.Tensor:
    """Decoded uint8 (H, W, 3) device tensors of any sizes -> (B, S, S, 3) uint8 on the device: Resize((S, S), BILINEAR) -> ToTensor ->
    Normalize(0.5, 0.5) (generate_folder.py:175-180) on the device, bit-identical to Pillow, then the generator and its uint8 epilogue."""
    from . import dataio
    dev = images[0].device
    pipe = getattr(G, "_infer_pipe", None)
    if pipe is None or pipe.S != img_size or pipe.device != dev or pipe.max_batch < len(images):
        pipe = dataio.InputPipeline(img_size, dev, max_batch=max(16, len(images)), filter=dataio.BILINEAR)
        object.__setattr__(G, "_infer_pipe", pipe)            # plain attribute, like the module's bridge
    x = pipe.run(images, [dataio.infer_job(int(im.shape[0]), int(im.shape[1]), img_size) for im in images])
    return stylize_hwc(G, x)


@torch.inference_mode()
def stylize_folder(G, src_dir: str, out_dir: str, device: str = "cuda", img_size: int = 256, batch: int = 16, limit: Optional[int] = None,
                   device_io: bool = False) -> int:
    """generate_folder.py:207-252 with PIL doing what torchvision's Resize(BILINEAR) / ToTensor / Normalize / ToPILImage do there.
    device_io: PIL only decodes and encodes; each photo is uploaded as uint8 HWC, `stylize_images` resizes, normalises, runs the
    generator and converts on the device, and one contiguous HWC download feeds PIL.  The files written are byte-identical."""
    import numpy as np
    from PIL import Image
    exts = {".jpg", ".jpeg", ".png", ".bmp", ".webp", ".tif", ".tiff"}
    src_root, out_root = Path(src_dir), Path(out_dir)
    paths = sorted(p for p in src_root.rglob("*") if p.suffix.lower() in exts)
    if limit is not None:
        paths = paths[:limit]
    if not paths:
        raise FileNotFoundError(f"No images found under: {src_dir}")
    out_root.mkdir(parents=True, exist_ok=True)
    for i in range(0, len(paths), batch):
        chunk = paths[i:i + batch]
        if device_io:
            imgs = [torch.from_numpy(np.array(Image.open(p).convert("RGB"))).to(device) for p in chunk]
            y = stylize_images(G, imgs, img_size).cpu().numpy()
        else:
            arr = np.stack([np.asarray(Image.open(p).convert("RGB").resize((img_size, img_size), Image.BILINEAR), dtype=np.float32) for p in chunk])
            x = torch.from_numpy(arr).permute(0, 3, 1, 2).div(255.0).sub(0.5).div(0.5).contiguous().to(device)
            y = stylize(G, x).cpu().permute(0, 2, 3, 1).numpy()
        for p, img in zip(chunk, y):
            save = (out_root / p.relative_to(src_root)).with_suffix(".jpg")
            save.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(img).save(save, format="JPEG", quality=95, subsampling=0, optimize=True)
    return len(paths)
