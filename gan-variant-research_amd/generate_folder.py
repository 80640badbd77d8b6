"""Inference driver with the reference's command line (GAN_Variant1/generate_folder.py:255-292):

    python -m gan_variant_research_amd.generate_folder --ckpt CKPT --photos DIR --out DIR [--batch 16] [--size 256] [--device cuda|cpu] [--limit N]
    python -m gan_variant_research_amd.generate_folder --ckpt CKPT --photos DIR --zip images.zip [--out DIR] --device-jpeg

Same flags, defaults and messages; the checkpoint is chosen as the reference chooses it (EMA shadow first, inference.pick_state_dict);
the output tree mirrors the input tree as JPEGs (quality 95, 4:4:4).  What differs is what runs underneath: the generator is the HIP
engine, and on the GPU the resize, the normalisation and the uint8 conversion run there as well (inference.stylize_images).
Build-only flags: --ngf / --n-blocks (the reference reads the architecture from its own module), --fp32 (bf16 operands stand in for the
reference's autocast by default), --graph (one hipGraph replay per batch shape), --host-io (resize and convert with PIL / torch on the host),
--device-jpeg (the JPEG files are encoded on the device as well, byte-identical to PIL's), --io-threads N (PIL decodes / saves on a thread pool),
--device-decode [--decode-chunk N] (baseline JPEGs are decoded on the device, N files at a time ahead of the generator, pixel-identical to PIL's),
--device-progressive (with --device-decode, progressive JPEGs are decoded on the device too),
--device-png (PNGs are decoded on the device the same way, --decode-chunk files at a time; with --device-decode one decoder takes both formats),
--zip PATH (the files become the stored entries of one archive, the competition's images.zip; --out is then optional, and with
--device-jpeg the files and their CRC-32 come from the device in one block per batch),
--which G_A2B|G_B2A (a CycleGAN checkpoint of train_basic is recognised by its keys; this picks the generator, architecture read from the keys).
"""
from __future__ import annotations

import argparse

import torch

from . import inference as I


def parse_args(argv=None) -> argparse.Namespace:
    """generate_folder.py:255-264, plus the build-only flags."""
    ap = argparse.ArgumentParser(description="Stylize a folder of photos with a trained CUT++ generator (MI355X-native).")
    ap.add_argument("--ckpt", required=True, help="Path to ckpt_final.pt or ckpt_stepXXXX.pt")
    ap.add_argument("--photos", required=True, help="Path to source photos folder (e.g., Kaggle photo_jpg)")
    ap.add_argument("--out", default=None, help="Output folder for generated JPGs (optional with --zip)")
    ap.add_argument("--batch", type=int, default=16, help="Batch size for inference")
    ap.add_argument("--size", type=int, default=256, help="Output resolution (and input resize)")
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"], help="Device")
    ap.add_argument("--limit", type=int, default=None, help="Optionally limit number of images for quick tests")
    ap.add_argument("--ngf", type=int, default=64, help="generator width of the checkpoint (build-only flag)")
    ap.add_argument("--n-blocks", type=int, default=9, help="residual blocks of the checkpoint (build-only flag)")
    ap.add_argument("--fp32", action="store_true", help="fp32 operands instead of bf16 (build-only flag)")
    ap.add_argument("--graph", action="store_true", help="replay the generator pass as one hipGraph per batch shape (build-only flag)")
    ap.add_argument("--host-io", action="store_true", help="resize / normalise / convert on the host instead of the device (build-only flag)")
    ap.add_argument("--which", default="G_A2B", choices=["G_A2B", "G_B2A"], help="generator of a CycleGAN checkpoint (train_basic's ckpt_e*.pt) to run (build-only flag)")
    ap.add_argument("--device-jpeg", action="store_true", help="encode the JPEGs on the device, byte-identical to PIL's (build-only flag)")
    ap.add_argument("--io-threads", type=int, default=1, help="threads for the PIL decodes (and the PIL saves without --device-jpeg), at most 16 (build-only flag)")
    ap.add_argument("--device-decode", action="store_true", help="decode baseline JPEGs on the device, pixel-identical to PIL's (build-only flag)")
    ap.add_argument("--device-progressive", action="store_true", help="with --device-decode: decode progressive JPEGs on the device too (build-only flag)")
    ap.add_argument("--decode-chunk", type=int, default=256, help="files per device decode, independent of --batch (build-only flag)")
    ap.add_argument("--device-png", action="store_true", help="decode PNGs on the device, pixel-identical to PIL's (build-only flag)")
    ap.add_argument("--zip", default=None, metavar="PATH", help="write the JPGs as stored entries of this archive, with or without --out (build-only flag)")
    args = ap.parse_args(argv)
    if args.out is None and args.zip is None:
        ap.error("one of --out and --zip is required")
    if args.device_png and (args.host_io or args.device == "cpu"):
        ap.error("--device-png feeds the device I/O path on the GPU: not with --host-io or --device cpu")
    if args.device_progressive and not args.device_decode:
        ap.error("--device-progressive widens what --device-decode takes: it needs --device-decode")
    if args.device_decode and (args.host_io or args.device == "cpu"):
        ap.error("--device-decode feeds the device I/O path on the GPU: not with --host-io or --device cpu")
    if args.decode_chunk < 1:
        ap.error("--decode-chunk must be at least 1")
    if args.device_jpeg and (args.host_io or args.device == "cpu"):
        ap.error("--device-jpeg encodes what the device I/O path leaves on the GPU: not with --host-io or --device cpu")
    if args.io_threads < 1:
        ap.error("--io-threads must be at least 1")
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    if args.device == "cuda" and not torch.cuda.is_available():
        if args.device_jpeg:
            raise SystemExit("--device-jpeg needs the GPU: there is no host fallback for the device encoder")
        if args.device_decode:
            raise SystemExit("--device-decode needs the GPU: there is no host fallback for the device decoder")
        if args.device_png:
            raise SystemExit("--device-png needs the GPU: there is no host fallback for the device decoder")
        print("[WARN] CUDA not available. Falling back to CPU.")
        args.device = "cpu"

    print(f"Loading generator from: {args.ckpt}")
    G = I.load_generator(args.ckpt, device=args.device, ngf=args.ngf, n_blocks=args.n_blocks, bf16=not args.fp32, use_graph=args.graph, which=args.which)
    n_params = sum(p.numel() for p in G.parameters())
    print(f"Generator parameters: {n_params:,}")

    print(f"Stylizing from '{args.photos}' -> '{args.out if args.out is not None else args.zip}' "
          f"(size={args.size}, batch={args.batch}, device={args.device})")
    # the device input pipeline and the uint8 epilogue are HIP kernels: they run exactly when the generator runs on the HIP library
    n = I.stylize_folder(G, src_dir=args.photos, out_dir=args.out, device=args.device, img_size=args.size, batch=args.batch, limit=args.limit,
                         device_io=args.device == "cuda" and not args.host_io, device_jpeg=args.device_jpeg,
                         io_threads=args.io_threads, **(dict(decode_chunk=args.decode_chunk) if args.device_decode or args.device_png else {}),
                         **(dict(device_decode=True) if args.device_decode else {}), **(dict(device_png=True) if args.device_png else {}),
                         **(dict(device_progressive=True) if args.device_progressive else {}), **(dict(zip_path=args.zip) if args.zip is not None else {}))
    print("Done.")
    return n


if __name__ == "__main__":
    main()
