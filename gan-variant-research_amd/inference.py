"""Forward-only generator inference (GAN_Variant1/generate_folder.py:112-252) on the HIP kernels.

`load_generator` takes the reference's checkpoints (or this package's: same layout) and prefers the EMA weights exactly as
generate_folder.py:125-170 does; `stylize` is the tensor-level body of `stylize_folder` (:207-252): G(x) then
clamp -> *0.5 + 0.5 -> *255 -> round -> uint8 (:183-185).  `stylize_hwc` is the same with the conversion and the HWC turn PIL needs
fused into one kernel after the generator's last layer (gan_view_to_u8_hwc), `stylize_images` puts the device input pipeline with
Pillow's BILINEAR taps (:175-180) in front of it.  JPEG / PNG decoding is PIL's on the host by default and, for baseline JPEGs,
`dataio.JpegDecoder`'s on the device with `device_decode=True` (the same pixels); JPEG encoding (:252) is PIL's by
default and `JpegEncoder`'s on the device with `device_jpeg=True`, byte for byte the same files.  `stylize_folder` walks a
PIL-readable folder, with the resize and both conversions on the host (the default) or on the device (`device_io=True`).
`zip_path` makes the files the stored entries of one archive (`ZipWriter`, byte-identical to Python's zipfile); with the device
encoder, `JpegEncoder.encode_block` hands over whole files and their CRC-32 from the device (csrc/zip.hip).
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


_JPEG_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_JPEG_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
_JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def _segment(marker: int, body: bytes) -> bytes:
    return bytes((0xFF, marker)) + (len(body) + 2).to_bytes(2, "big") + body


class JpegEncoder:
    """Baseline JPEG files from packed uint8 (B, H, W, 3) device batches, byte-identical to the reference's
    pil.save(..., format="JPEG", quality=95, subsampling=0, optimize=True) (generate_folder.py:252).  Colour conversion, DCT,
    quantisation, the optimal Huffman tables and the stuffed scan are made on the device (csrc/jpeg.hip); the host downloads B + 1
    offsets, the tables and one contiguous block of scan bytes, and writes the headers around them.  Owns its buffers, like
    dataio.InputPipeline; one encoder serves batches of up to `max_batch` images of one size."""

    def __init__(self, device, max_batch: int, H: int, W: int, quality: int = 95, ops=None):
        from . import autograd as AG
        from ._lib import GanError
        self.device, self.max_batch, self.H, self.W, self.quality = torch.device(device), int(max_batch), int(H), int(W), int(quality)
        if not 1 <= self.quality <= 100:
            raise ValueError(f"quality = {quality}: 1 .. 100")
        if not (self.max_batch >= 1 and 1 <= self.H <= 65535 and 1 <= self.W <= 65535):
            raise ValueError(f"JpegEncoder: max_batch = {max_batch}, H = {H}, W = {W}: max_batch >= 1 and 1 <= H, W <= 65535")
        self.ops = AG._OPS_FACTORY(self.device) if ops is None else ops
        if getattr(self.ops, "is_hip", False) and self.device.type != "cuda":
            raise GanError("the MI355X path needs tensors on a GPU (there is no CPU fallback)")
        ws_bytes, out_bytes = self.ops.jpeg_bounds(self.max_batch, self.H, self.W)
        new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)
        self.rgb = new((self.max_batch, self.H, self.W, 3), torch.uint8)
        self.ws, self.out = new(ws_bytes, torch.uint8), new(out_bytes, torch.uint8)
        self.hist, self.codes = new((self.max_batch, 4, 256), torch.int32), new((self.max_batch, 4, 256), torch.int32)
        self.dht, self.offsets = new((self.max_batch, 4, 272), torch.uint8), new(self.max_batch + 1, torch.int64)
        self._programs, self._file_programs, self._files = {}, {}, None
        s = 5000 // self.quality if self.quality < 50 else 200 - 2 * self.quality
        head = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00" + bytes((1, 1, 0, 0, 1, 0, 1, 0, 0)))
        for i, base in enumerate((_JPEG_LUMA, _JPEG_CHROMA)):
            q = [min(max((v * s + 50) // 100, 1), 255) for v in base]
            head += _segment(0xDB, bytes([i]) + bytes(q[k] for k in _JPEG_ZIGZAG))
        self._head = head + _segment(0xC0, bytes([8]) + self.H.to_bytes(2, "big") + self.W.to_bytes(2, "big") + bytes((3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1)))
        self._sos = _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0)))

    def _program(self, B: int):
        prog = self._programs.get(B)
        if prog is None:
            o = self.ops
            prog = self._programs[B] = [o.jpeg_blocks(self.rgb[:B], self.quality, self.ws, self.hist), o.jpeg_tables(self.hist, 4 * B, self.dht, self.codes),
                                        o.jpeg_scan(self.ws, B, self.H, self.W, self.codes, self.out, self.offsets)]
        return prog

    @torch.inference_mode()
    def encode(self, batch: torch.Tensor) -> list:
        """(B, H, W, 3) uint8 on the encoder's device, B <= max_batch -> B complete JPEG files as bytes."""
        B = int(batch.shape[0])
        if batch.dtype != torch.uint8 or tuple(batch.shape[1:]) != (self.H, self.W, 3) or not 1 <= B <= self.max_batch or batch.device != self.rgb.device:
            raise ValueError(f"JpegEncoder.encode: expected uint8 (1 .. {self.max_batch}, {self.H}, {self.W}, 3) on {self.rgb.device}, "
                             f"got {batch.dtype} {tuple(batch.shape)} on {batch.device}")
        self.rgb[:B].copy_(batch)
        for op in self._program(B):
            op()
        off = self.offsets[:B + 1].cpu().tolist()
        dht = self.dht[:B].cpu().numpy()
        scan = self.out[:off[B]].cpu().numpy().tobytes()
        files = []
        for b in range(B):
            tables = b""
            for t, tc in enumerate((0x00, 0x10, 0x01, 0x11)):          # DC0, AC0, DC1, AC1
                n = int(dht[b, t, :16].sum())
                tables += _segment(0xC4, bytes([tc]) + dht[b, t, :16 + n].tobytes())
            files.append(self._head + tables + self._sos + scan[off[b]:off[b + 1]] + b"\xff\xd9")
        return files

    def _file_program(self, B: int):
        """The buffers of `encode_block`, made at its first call (an encoder that only serves `encode` never holds them), and the launch
        sequence for a batch of B."""
        if self._files is None:
            o, mb = self.ops, self.max_batch
            as_dev = lambda data: torch.frombuffer(bytearray(data), dtype=torch.uint8).to(self.device)
            self._head_dev, self._sos_dev = as_dev(self._head), as_dev(self._sos)
            self._files = torch.zeros(o.jpeg_files_bounds(mb, self.H, self.W, len(self._head), len(self._sos)), dtype=torch.uint8, device=self.device)
            # one block for everything that comes back beside the files: int64 offsets [mb + 1] | int32 crc [mb] | int32 flag
            self._meta = torch.zeros(8 * (mb + 1) + 4 * mb + 4, dtype=torch.uint8, device=self.device)
            self.file_offsets = self._meta[:8 * (mb + 1)].view(torch.int64)
            self.crc, self.flag = self._meta[8 * (mb + 1):8 * (mb + 1) + 4 * mb].view(torch.int32), self._meta[8 * (mb + 1) + 4 * mb:].view(torch.int32)
        prog = self._file_programs.get(B)
        if prog is None:
            prog = self._file_programs[B] = self._program(B) + [self.ops.jpeg_files(self._head_dev, self._sos_dev, self.dht, self.out, self.offsets, B, self._files,
                                                                                    self.file_offsets, self.crc, self.flag)]
        return prog

    @torch.inference_mode()
    def encode_block(self, batch: torch.Tensor):
        """`encode` for a consumer that wants the files as they lie in memory: (block, offsets, crcs) with block a bytes-like object
        (a memoryview), `block[offsets[b]:offsets[b + 1]]` the file `encode(batch)[b]`, and crcs[b] its CRC-32 (zlib.crc32).  The files are
        put together and checksummed on the device (csrc/zip.hip); two downloads: offsets, CRCs and the flag word in one small copy, the
        files in one contiguous copy."""
        from ._lib import GanError
        B = int(batch.shape[0])
        if batch.dtype != torch.uint8 or tuple(batch.shape[1:]) != (self.H, self.W, 3) or not 1 <= B <= self.max_batch or batch.device != self.rgb.device:
            raise ValueError(f"JpegEncoder.encode_block: expected uint8 (1 .. {self.max_batch}, {self.H}, {self.W}, 3) on {self.rgb.device}, "
                             f"got {batch.dtype} {tuple(batch.shape)} on {batch.device}")
        prog = self._file_program(B)
        self.rgb[:B].copy_(batch)
        for op in prog:
            op()
        mb = self.max_batch
        meta = self._meta.cpu().numpy()
        off = meta[:8 * (B + 1)].view("<i8").tolist()
        crcs = meta[8 * (mb + 1):8 * (mb + 1) + 4 * B].view("<u4").tolist()
        flag = int(meta[8 * (mb + 1) + 4 * mb:].view("<u4")[0])
        if flag:
            raise GanError(f"JpegEncoder.encode_block: the device flagged the batch (flag = {flag}: 1 = inconsistent scan offsets, 2 = the files buffer is too small)")
        return memoryview(self._files[:off[B]].cpu().numpy()), off, crcs


class ZipWriter:
    """A ZIP archive of stored (uncompressed) entries, byte-identical to Python's zipfile for
    `ZipFile(path, "w", ZIP_STORED)` with `writestr(ZipInfo(name, date_time=date_time), data)` per entry in the same order: version 20,
    no data descriptor, external attributes 0o600 << 16, flag 0x800 for a name that is not ASCII.  An entry needs its name, its bytes and
    their CRC-32; `add_block` takes the CRCs from whoever has them already (JpegEncoder.encode_block: the device).  The archive is
    written to path + ".part" and renamed by a clean close; an exception inside `with` removes the part file.  No ZIP64: more than
    MAX_ENTRIES entries, or a size or an offset of MAX_BYTES or more, is a ValueError, and so is a repeated name."""
    MAX_ENTRIES = 65535
    MAX_BYTES = 1 << 32

    def __init__(self, path, date_time=(1980, 1, 1, 0, 0, 0)):
        import struct
        import sys
        self._struct = struct
        self.path, self._part = str(path), str(path) + ".part"
        y, mo, d, h, mi, sec = date_time
        if not (1980 <= y <= 2107 and 1 <= mo <= 12 and 1 <= d <= 31 and 0 <= h <= 23 and 0 <= mi <= 59 and 0 <= sec <= 59):
            raise ValueError(f"ZipWriter: date_time = {date_time}: a ZIP holds 1980-01-01 .. 2107-12-31")
        self._date, self._time = (y - 1980) << 9 | mo << 5 | d, h << 11 | mi << 5 | sec // 2
        self._system = 0 if sys.platform == "win32" else 3              # zipfile.ZipInfo.create_system
        self._entries, self._names, self._pos = [], set(), 0
        self._f = open(self._part, "wb")

    def __len__(self):
        return len(self._entries)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.abort()
        return False

    def abort(self):
        """Drop the archive: the part file goes, nothing appears at `path`."""
        import os
        if self._f is not None:
            self._f.close()
            self._f = None
            if os.path.exists(self._part):
                os.remove(self._part)

    def _local(self, name: str, size: int, crc: int) -> bytes:
        """The local header of the next entry, recorded for the central directory."""
        if self._f is None:
            raise ValueError("ZipWriter: the archive is closed")
        if name in self._names:
            raise ValueError(f"ZipWriter: the name {name!r} is in the archive already")
        if len(self._entries) >= self.MAX_ENTRIES:
            raise ValueError(f"ZipWriter: more than {self.MAX_ENTRIES} entries need ZIP64, which is not written")
        try:
            raw, flags = name.encode("ascii"), 0
        except UnicodeEncodeError:
            raw, flags = name.encode("utf-8"), 0x800
        if len(raw) > 65535:
            raise ValueError("ZipWriter: a name of more than 65535 bytes")
        if size >= self.MAX_BYTES or self._pos >= self.MAX_BYTES or self._pos + 30 + len(raw) + size >= self.MAX_BYTES:
            raise ValueError(f"ZipWriter: a size or an offset of {self.MAX_BYTES} or more needs ZIP64, which is not written")
        self._names.add(name)
        self._entries.append((raw, flags, crc, size, self._pos))
        self._pos += 30 + len(raw) + size
        return self._struct.pack("<4s2B4HL2L2H", b"PK\x03\x04", 20, 0, flags, 0, self._time, self._date, crc, size, size, len(raw), 0) + raw

    def add(self, name: str, data, crc=None):
        """One entry; crc: the CRC-32 of data when the caller has it, else zlib.crc32 computes it here."""
        import zlib
        data = memoryview(data).cast("B")
        head = self._local(name, len(data), (zlib.crc32(data) if crc is None else int(crc)) & 0xFFFFFFFF)
        self._f.write(head)
        self._f.write(data)

    def add_block(self, names, block, offsets, crcs=None):
        """len(names) entries from one block: entry b is block[offsets[b]:offsets[b + 1]] with CRC-32 crcs[b] (crcs None: computed
        here).  Headers and data go out in one write."""
        import zlib
        block = memoryview(block).cast("B")
        if len(offsets) != len(names) + 1 or (crcs is not None and len(crcs) != len(names)):
            raise ValueError(f"ZipWriter.add_block: {len(names)} names, {len(offsets)} offsets, {None if crcs is None else len(crcs)} CRCs")
        if any(not 0 <= offsets[b] <= offsets[b + 1] <= len(block) for b in range(len(names))):
            raise ValueError("ZipWriter.add_block: offsets that do not lie in the block in order")
        parts = []
        for b, name in enumerate(names):
            data = block[offsets[b]:offsets[b + 1]]
            parts.append(self._local(name, len(data), (zlib.crc32(data) if crcs is None else int(crcs[b])) & 0xFFFFFFFF))
            parts.append(data)
        self._f.write(b"".join(parts))

    def close(self):
        """Central directory and end record, then the rename to `path`.  A second close does nothing."""
        import os
        if self._f is None:
            return
        try:
            start, pack = self._pos, self._struct.pack
            out = []
            for raw, flags, crc, size, offset in self._entries:
                out.append(pack("<4s4B4HL2L5H2L", b"PK\x01\x02", 20, self._system, 20, 0, flags, 0, self._time, self._date, crc, size, size, len(raw), 0, 0,
                                0, 0, 0o600 << 16, offset) + raw)
            cd = b"".join(out)
            if start + len(cd) >= self.MAX_BYTES:
                raise ValueError(f"ZipWriter: a central directory that ends at {self.MAX_BYTES} or beyond needs ZIP64, which is not written")
            self._f.write(cd + pack("<4s4H2LH", b"PK\x05\x06", 0, 0, len(self._entries), len(self._entries), len(cd), start, 0))
        except BaseException:
            self.abort()
            raise
        self._f.close()
        self._f = None
        os.replace(self._part, self.path)


def _jpeg_encoder(G, device, batch: int, H: int, W: int) -> JpegEncoder:
    """The encoder cached on the generator, like `_infer_pipe`."""
    enc = getattr(G, "_jpeg_enc", None)
    if enc is None or (enc.H, enc.W) != (H, W) or enc.device != device or enc.max_batch < batch:
        enc = JpegEncoder(device, max(16, batch), H, W, quality=95)
        object.__setattr__(G, "_jpeg_enc", enc)
    return enc


def _jpeg_decoder(G, device, progressive: bool = False):
    """The decoder cached on the generator, like `_infer_pipe`."""
    from . import dataio
    dev = dataio.normalize_device(device)
    dec = getattr(G, "_jpeg_dec", None)
    if dec is None or dec.device != dev or dec.progressive != bool(progressive):
        dec = dataio.JpegDecoder(dev, progressive=progressive)
        object.__setattr__(G, "_jpeg_dec", dec)
    return dec


def _folder_decoder(G, device, jpeg: bool, png: bool, progressive: bool = False):
    """The decoder of the folder path for the switches that are on, cached on the generator: a JpegDecoder, a PngDecoder, or one
    DeviceDecoder for both formats."""
    from . import dataio
    if not png:
        return _jpeg_decoder(G, device, progressive)
    dev = dataio.normalize_device(device)
    name, make = ("_device_dec", lambda d: dataio.DeviceDecoder(d, progressive=progressive)) if jpeg else ("_png_dec", dataio.PngDecoder)
    dec = getattr(G, name, None)
    if dec is None or dec.device != dev or getattr(dec, "progressive", False) != bool(progressive and jpeg):
        dec = make(dev)
        object.__setattr__(G, name, dec)
    return dec


@torch.inference_mode()
def stylize_folder(G, src_dir: str, out_dir: Optional[str] = None, device: str = "cuda", img_size: int = 256, batch: int = 16, limit: Optional[int] = None,
                   device_io: bool = False, device_jpeg: bool = False, io_threads: int = 1, device_decode: bool = False, decode_chunk: int = 256,
                   device_png: bool = False, device_progressive: bool = False, zip_path: Optional[str] = None) -> int:
    """generate_folder.py:207-252 with PIL doing what torchvision's Resize(BILINEAR) / ToTensor / Normalize / ToPILImage do there.
    device_io: PIL only decodes and encodes; each photo is uploaded as uint8 HWC, `stylize_images` resizes, normalises, runs the
    generator and converts on the device, and one contiguous HWC download feeds PIL.  The files written are byte-identical.
    device_jpeg (needs device_io): the batch never comes back as pixels; `JpegEncoder` makes the files on the device and the host
    writes their bytes.  io_threads > 1: the PIL decodes of a chunk (and, without device_jpeg, the PIL saves) run on a thread pool of
    at most 16 workers, as dataio.ImageStore's does.  device_decode (needs device_io): `dataio.JpegDecoder` decodes the baseline JPEGs
    on the device, `decode_chunk` files per call whatever `batch` is (its entropy stage has one lane per restart segment: many files in
    flight are its throughput), one chunk ahead on a side stream while the generator works on the previous one; other files, and files
    the decoder flags, still go through PIL.  device_png (needs device_io; independent of device_decode): the same for the PNGs, with
    `dataio.PngDecoder` (one workgroup per file: again the files in flight are its throughput); with both switches one
    `dataio.DeviceDecoder` reads every file once and sends it by its content.  device_progressive (needs device_decode): the
    progressive JPEGs `dataio.parse_jpeg_progressive` accepts are decoded on the device too, in the same calls.  Same files either way.
    zip_path: the files also (or, without out_dir, only) become the stored entries of one archive, written by `ZipWriter` in the order
    of the sorted paths; an entry is named like the file, relative to the output root with `/` separators.  With device_jpeg the
    entries come from `JpegEncoder.encode_block`: whole files and their CRC-32 from the device, no per-file assembly and no checksum
    on the host; otherwise PIL saves into memory and the writer checksums.  Two sources that map to one output name (a.png beside
    a.jpg) are a ValueError there, where the folder keeps the later file.  At least one of out_dir and zip_path is required."""
    import contextlib
    import io
    import numpy as np
    from PIL import Image
    if out_dir is None and zip_path is None:
        raise ValueError("stylize_folder: give out_dir, zip_path or both: there is nowhere to write")
    if device_jpeg and not device_io:
        raise ValueError("device_jpeg=True needs device_io=True: the encoder reads the uint8 batch the device epilogue leaves")
    if device_decode and not device_io:
        raise ValueError("device_decode=True needs device_io=True: the decoder leaves the uint8 images the device input pipeline reads")
    if device_progressive and not device_decode:
        raise ValueError("device_progressive=True needs device_decode=True: it widens the class of JPEGs the device decoder takes")
    if device_png and not device_io:
        raise ValueError("device_png=True needs device_io=True: the decoder leaves the uint8 images the device input pipeline reads")
    if decode_chunk < 1:
        raise ValueError(f"decode_chunk = {decode_chunk}: at least 1")
    if io_threads < 1:
        raise ValueError(f"io_threads = {io_threads}: at least 1")
    exts = {".jpg", ".jpeg", ".png", ".bmp", ".webp", ".tif", ".tiff"}
    src_root, out_root = Path(src_dir), None if out_dir is None else Path(out_dir)
    paths = sorted(p for p in src_root.rglob("*") if p.suffix.lower() in exts)
    if limit is not None:
        paths = paths[:limit]
    if not paths:
        raise FileNotFoundError(f"No images found under: {src_dir}")
    if out_root is not None:
        out_root.mkdir(parents=True, exist_ok=True)
    pool = None
    if io_threads > 1:
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(min(io_threads, 16))
    each = (lambda fn, *its: list(pool.map(fn, *its))) if pool is not None else (lambda fn, *its: [fn(*a) for a in zip(*its)])

    def decode(p):
        return np.array(Image.open(p).convert("RGB"))

    def decode_resized(p):
        return np.asarray(Image.open(p).convert("RGB").resize((img_size, img_size), Image.BILINEAR), dtype=np.float32)

    def target(p):
        save = (out_root / p.relative_to(src_root)).with_suffix(".jpg")
        save.parent.mkdir(parents=True, exist_ok=True)
        return save

    def save_pil(p, img):
        Image.fromarray(img).save(target(p), format="JPEG", quality=95, subsampling=0, optimize=True)

    def save_bytes(p, data):
        target(p).write_bytes(data)

    def pil_bytes(img):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=95, subsampling=0, optimize=True)
        return buf.getvalue()

    def entry(p):
        return p.relative_to(src_root).with_suffix(".jpg").as_posix()

    def decoded_ahead():
        """The images of `paths` in chunks of decode_chunk files, the next chunk being decoded while the caller works on this one."""
        from concurrent.futures import ThreadPoolExecutor
        dec = _folder_decoder(G, device, device_decode, device_png, device_progressive)
        cuda = dec.device.type == "cuda"
        side = torch.cuda.Stream(dec.device) if cuda else None
        main = torch.cuda.current_stream(dec.device) if cuda else None

        def job(s):
            if not cuda:
                return dec.decode(paths[s:s + decode_chunk], each=each)
            with torch.cuda.stream(side):
                return dec.decode(paths[s:s + decode_chunk], each=each)      # returns after its error words came back: the pixels are there
        with ThreadPoolExecutor(1) as ahead:
            fut = ahead.submit(job, 0)
            for s in range(0, len(paths), decode_chunk):
                imgs = fut.result()
                if s + decode_chunk < len(paths):
                    fut = ahead.submit(job, s + decode_chunk)
                if cuda:
                    imgs[0].record_stream(main)      # one buffer behind all views; allocated on the side stream, read on this one
                yield imgs

    with contextlib.ExitStack() as stack:
        # one writer, on this thread, in the order of `paths`: the pool only ever encodes and writes files of the folder
        zw = stack.enter_context(ZipWriter(zip_path)) if zip_path is not None else None
        try:
            on_device = device_decode or device_png
            ready, chunks = [], decoded_ahead() if on_device else None
            for i in range(0, len(paths), batch):
                chunk = paths[i:i + batch]
                if device_io:
                    if on_device:
                        while len(ready) < min(i + batch, len(paths)):
                            ready.extend(next(chunks))
                        imgs, ready[i:i + batch] = ready[i:i + batch], [None] * len(chunk)
                    else:
                        imgs = [torch.from_numpy(a).to(device) for a in each(decode, chunk)]
                    y = stylize_images(G, imgs, img_size)
                    if device_jpeg:
                        enc = _jpeg_encoder(G, y.device, len(chunk), img_size, img_size)
                        if zw is None:
                            each(save_bytes, chunk, enc.encode(y))
                            continue
                        block, off, crcs = enc.encode_block(y)
                        zw.add_block([entry(p) for p in chunk], block, off, crcs)
                        if out_root is not None:
                            each(save_bytes, chunk, [block[off[b]:off[b + 1]] for b in range(len(chunk))])
                        continue
                    y = y.cpu().numpy()
                else:
                    arr = np.stack(each(decode_resized, chunk))
                    x = torch.from_numpy(arr).permute(0, 3, 1, 2).div(255.0).sub(0.5).div(0.5).contiguous().to(device)
                    y = stylize(G, x).cpu().permute(0, 2, 3, 1).numpy()
                if zw is None:
                    each(save_pil, chunk, y)
                    continue
                files = each(pil_bytes, y)
                if out_root is not None:
                    each(save_bytes, chunk, files)
                for p, data in zip(chunk, files):
                    zw.add(entry(p), data)
        finally:
            if chunks is not None:
                chunks.close()
            if pool is not None:
                pool.shutdown()
    return len(paths)
