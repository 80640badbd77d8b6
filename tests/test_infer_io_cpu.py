"""Inference I/O, the parts that need no GPU: Pillow's BILINEAR tap tables from the library (host code), the BICUBIC tables through the
new entries, `stylize_hwc` on the emulator, and the command line (gan_variant_research_amd.generate_folder) on the CPU."""
import math

import numpy as np
import pytest
import torch

from gan_variant_research_amd import _lib, autograd as AG, cut as C, dataio, inference as I
from oracle import input_ref as R
from tests.emulator_infer import InferEmuOps

BILINEAR, BICUBIC = 2, 3
PAIRS = [(20, 16), (24, 16), (53, 16), (300, 16), (9, 16), (5, 16), (16, 16), (1, 8), (513, 32), (217, 32), (100, 64), (67, 64)]
BICUBIC_PAIRS = [(217, 256), (256, 256), (256, 286), (1024, 256), (50, 96), (513, 256), (300, 72), (8, 64), (64, 8)]


def _tables(lib, i, o, flt):
    k = lib.gan_resize_ksize_filter(i, o, flt)
    assert k > 0, lib.gan_last_error()
    bounds, kk = np.zeros((o, 2), np.int32), np.zeros((o, k), np.int32)
    assert lib.gan_resize_coeffs_filter(i, o, flt, bounds.ctypes.data, kk.ctypes.data, k) == 0, lib.gan_last_error()
    return bounds, kk, k


def test_constants_are_pillows():
    from PIL import Image
    assert (dataio.BILINEAR, dataio.BICUBIC) == (int(Image.BILINEAR), int(Image.BICUBIC)) == (BILINEAR, BICUBIC)
    assert (_lib.RESIZE_BILINEAR, _lib.RESIZE_BICUBIC) == (BILINEAR, BICUBIC)


def test_bilinear_tables_equal_pillow():
    """Every pair serves once as the horizontal and once as the vertical pass of an Image.resize(BILINEAR)."""
    from PIL import Image
    lib = _lib.load()
    rng = np.random.default_rng(0)
    for n, (w, ow) in enumerate(PAIRS):
        h, oh = PAIRS[(n + 1) % len(PAIRS)]
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        x = im
        if ow != w:
            b, kk, _ = _tables(lib, w, ow, BILINEAR)
            x = R._resample_axis(x, b, kk, axis=1)
        if oh != h:
            b, kk, _ = _tables(lib, h, oh, BILINEAR)
            x = R._resample_axis(x, b, kk, axis=0)
        want = np.asarray(Image.fromarray(im).resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(x, want), ((h, w), (oh, ow), int(np.abs(x.astype(int) - want.astype(int)).max()))
    # the pass Pillow skips: the table of an unchanged size is the identity, so the device pipeline (which always runs both) is exact too
    b, kk, _ = _tables(lib, 16, 16, BILINEAR)
    im = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    assert np.array_equal(R._resample_axis(im, b, kk, axis=1), im)


def test_bilinear_ksize_and_errors():
    lib = _lib.load()
    for i, o in PAIRS + BICUBIC_PAIRS:
        assert lib.gan_resize_ksize_filter(i, o, BILINEAR) == math.ceil(max(i / o, 1.0)) * 2 + 1, (i, o)
    b2, k2 = np.zeros((20, 2), np.int32), np.zeros((20, 16), np.int32)
    for flt in (0, 1, 4, -1):
        assert lib.gan_resize_ksize_filter(10, 20, flt) < 0 and b"filter" in lib.gan_last_error()
        assert lib.gan_resize_coeffs_filter(10, 20, flt, b2.ctypes.data, k2.ctypes.data, 3) != 0 and b"filter" in lib.gan_last_error()
    assert lib.gan_resize_coeffs_filter(10, 20, BILINEAR, b2.ctypes.data, k2.ctypes.data, 5) != 0 and b"ksize" in lib.gan_last_error()
    assert lib.gan_resize_coeffs_filter(10, 20, BICUBIC, b2.ctypes.data, k2.ctypes.data, 3) != 0 and b"ksize" in lib.gan_last_error()
    assert lib.gan_resize_ksize_filter(0, 20, BILINEAR) < 0 and b"positive" in lib.gan_last_error()
    assert lib.gan_input_pipeline_filter(None, None, 0, None, 16, 7, None, 0, None, None, None, None) != 0 and b"filter" in lib.gan_last_error()


def test_bicubic_tables_are_untouched():
    """The _filter entries with BICUBIC are the existing entries byte for byte (and those still equal the restatement of Pillow)."""
    lib = _lib.load()
    for i, o in BICUBIC_PAIRS:
        k = lib.gan_resize_ksize(i, o)
        assert lib.gan_resize_ksize_filter(i, o, BICUBIC) == k
        b0, k0 = np.zeros((o, 2), np.int32), np.zeros((o, k), np.int32)
        assert lib.gan_resize_coeffs(i, o, b0.ctypes.data, k0.ctypes.data, k) == 0
        b1, k1, _ = _tables(lib, i, o, BICUBIC)
        assert b0.tobytes() == b1.tobytes() and k0.tobytes() == k1.tobytes(), (i, o)
        rb, rk = R.resize_coeffs(i, 0, i, o)
        assert np.array_equal(b1, rb) and np.array_equal(k1, rk), (i, o)


def test_stylize_hwc_on_emulator(monkeypatch):
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: InferEmuOps())
    torch.manual_seed(5)
    G = C.ResNetGenerator(3, 3, ngf=8, n_blocks=2).eval()
    x = torch.rand(2, 3, 16, 16) * 2 - 1
    with torch.no_grad():
        want = I.to_uint8(G(x)).permute(0, 2, 3, 1)
    got = I.stylize_hwc(G, x)
    assert got.dtype == torch.uint8 and got.shape == (2, 16, 16, 3) and got.is_contiguous()
    assert torch.equal(got, want)
    assert torch.equal(G.forward_u8(x), want)                 # the slot's epilogue is reused
    assert len(set(want.flatten().tolist())) > 8              # not a constant image


def test_slot_planned_under_inference_mode_serves_later_callers(monkeypatch):
    """The pass slot is pooled: one planned by an inference_mode caller must still take the input of a caller outside it."""
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: InferEmuOps())
    torch.manual_seed(6)
    G = C.ResNetGenerator(3, 3, ngf=8, n_blocks=2).eval()
    for p in G.parameters():
        p.requires_grad_(False)
    x = torch.rand(1, 3, 16, 16) * 2 - 1
    with torch.inference_mode():
        want = I.to_uint8(G(x)).permute(0, 2, 3, 1)
    assert torch.equal(G.forward_u8(x), want)                 # outside inference_mode, same slot
    with torch.no_grad():
        assert torch.equal(I.to_uint8(G(x)).permute(0, 2, 3, 1), want)
    assert torch.equal(I.stylize_hwc(G, x), want)


def test_command_on_the_cpu(monkeypatch, tmp_path, capsys):
    from PIL import Image
    from gan_variant_research_amd import generate_folder as GF
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: InferEmuOps())
    torch.manual_seed(3)
    G = C.ResNetGenerator(3, 3, ngf=8, n_blocks=2)
    shadow = {k: v.detach() * 0.5 for k, v in G.state_dict().items()}
    ck = tmp_path / "ckpt_final.pt"
    torch.save({"step": 7, "generator": G.state_dict(), "ema_G": {"decay": 0.999, "shadow": shadow}, "config": {}}, ck)
    photos = tmp_path / "photos"
    (photos / "sub").mkdir(parents=True)
    rng = np.random.default_rng(1)
    for name, (h, w) in (("a.png", (20, 24)), ("sub/b.png", (33, 17)), ("sub/c.png", (16, 16))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(photos / name)
    base = ["--ckpt", str(ck), "--photos", str(photos), "--device", "cpu", "--size", "16", "--batch", "2", "--ngf", "8", "--n-blocks", "2", "--fp32"]
    n = GF.main(base + ["--out", str(tmp_path / "out")])
    text = capsys.readouterr().out
    assert n == 3
    assert f"Loading generator from: {ck}" in text and "Generator parameters: " in text and text.rstrip().endswith("Done.")
    assert f"Stylizing from '{photos}' -> '{tmp_path / 'out'}' (size=16, batch=2, device=cpu)" in text
    got = sorted(p.relative_to(tmp_path / "out").as_posix() for p in (tmp_path / "out").rglob("*") if p.is_file())
    assert got == ["a.jpg", "sub/b.jpg", "sub/c.jpg"]
    for rel in got:
        assert Image.open(tmp_path / "out" / rel).size == (16, 16)
    # the EMA shadow was loaded: the files are what a generator holding the shadow writes, not what the raw weights write
    G.eval()
    I.stylize_folder(G, str(photos), str(tmp_path / "raw"), device="cpu", img_size=16, batch=2)
    G.load_state_dict(shadow)
    I.stylize_folder(G, str(photos), str(tmp_path / "ema"), device="cpu", img_size=16, batch=2)
    for rel in got:
        out = (tmp_path / "out" / rel).read_bytes()
        assert out == (tmp_path / "ema" / rel).read_bytes() and out != (tmp_path / "raw" / rel).read_bytes(), rel
    assert GF.main(base + ["--out", str(tmp_path / "lim"), "--limit", "2"]) == 2
    assert sorted(p.name for p in (tmp_path / "lim").rglob("*.jpg")) == ["a.jpg", "b.jpg"]
    a = GF.parse_args(["--ckpt", "c", "--photos", "p", "--out", "o"])
    assert (a.batch, a.size, a.device, a.limit, a.ngf, a.n_blocks, a.fp32, a.graph, a.host_io) == (16, 256, "cuda", None, 64, 9, False, False, False)


def test_command_falls_back_to_the_cpu_with_the_reference_warning(monkeypatch, tmp_path, capsys):
    from gan_variant_research_amd import generate_folder as GF
    seen = {}
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(I, "load_generator", lambda ckpt, device, **kw: seen.update(device=device, **kw) or torch.nn.Linear(1, 1))
    monkeypatch.setattr(I, "stylize_folder", lambda G, **kw: seen.update(kw) or 0)
    GF.main(["--ckpt", "c", "--photos", "p", "--out", "o", "--graph"])
    assert "[WARN] CUDA not available. Falling back to CPU." in capsys.readouterr().out
    assert seen["device"] == "cpu" and seen["device_io"] is False and seen["use_graph"] is True and seen["bf16"] is True


def test_pipeline_still_needs_the_gpu():
    with pytest.raises(_lib.GanError):
        dataio.InputPipeline(16, "cpu")
    with pytest.raises(_lib.GanError):
        dataio.InputPipeline(16, "cpu", filter=dataio.BILINEAR)
    assert dataio.infer_job(20, 24, 16) == dataio.eval_job(20, 24, 16)
