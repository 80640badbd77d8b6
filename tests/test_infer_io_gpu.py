"""Inference I/O on the device: the fused uint8 HWC epilogue (gan_view_to_u8_hwc), `forward_u8` / `stylize_hwc`, the input pipeline with
Pillow's BILINEAR taps, and the folder path with device I/O -- all exact: the epilogue against `inference.to_uint8` of what
gan_view_to_nchw writes, the pipeline against Pillow itself, the folder against the files the host path writes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gan_variant_research_amd import BF16, F32, cut as C, dataio, inference as I
from gan_variant_research_amd.runtime import HipOps, View, torch_dtype
from oracle import input_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
GUARD = 64
SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), 1.0, -1.0]


def _pool(dtype) -> torch.Tensor:
    """The value sweep (fp32 tensor on the host; for bf16 views every entry is a bf16 value).
    bf16: every bf16 value in [-1.5, 1.5].  fp32: a 2^16-point grid over [-1.5, 1.5]; each (2k + 1) / 510 - 1, k = 0 .. 254, with its
    two fp32 neighbours; and the inputs whose scaled value is an exact half, (2k + 1) / 255 - 1 -- where round-half-to-even decides --
    with their two neighbours.  Both: +-0, +-inf, +-1."""
    if dtype == BF16:
        v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
        vals = v[v.abs() <= 1.5]                      # drops NaN and everything outside
    else:
        k = np.arange(255, dtype=np.float64)
        pts = np.concatenate([(2 * k + 1) / 510 - 1, (2 * k + 1) / 255 - 1]).astype(np.float32)
        pts = np.concatenate([pts, np.nextafter(pts, np.float32(2)), np.nextafter(pts, np.float32(-2))])
        vals = torch.from_numpy(np.concatenate([np.linspace(-1.5, 1.5, 1 << 16).astype(np.float32), pts]))
    return torch.cat([torch.tensor(SPECIALS), vals])


def _poisoned_view(dtype, B, H, W, halo, Cr, values: torch.Tensor) -> View:
    """A view of 8 channels whose halo pixels and pad channels Cr .. 8 hold NaN and 1e30, its interior `values` (B, H, W, Cr)."""
    Cv = 8
    n = B * (H + 2 * halo) * (W + 2 * halo) * Cv
    t = torch.where(torch.arange(n) % 2 == 0, torch.tensor(float("nan")), torch.tensor(1e30)).to(torch_dtype(dtype)).to(DEV)
    v = View(t, B, H, W, Cv, halo, dtype)
    v.nhwc()[..., :Cr] = values.to(torch_dtype(dtype)).to(DEV)
    return v


def _run_epilogue(ops, view, Cr, misalign=0):
    """dst inside a guard band; returns (dst, reference) -- the reference is to_uint8 of gan_view_to_nchw's output, permuted to HWC."""
    B, H, W = view.B, view.H, view.W
    n = B * H * W * Cr
    buf = torch.full((n + 2 * GUARD + misalign,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = buf[GUARD + misalign:GUARD + misalign + n].view(B, H, W, Cr)
    ops.view_to_u8_hwc(view, Cr, dst)()
    nchw = torch.zeros(B, Cr, H, W, dtype=torch.float32, device=DEV)
    ops.view_to_nchw(view, Cr, nchw)()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD + misalign] == 0xA5).all()) and bool((buf[GUARD + misalign + n:] == 0xA5).all()), "guard band written"
    return dst, nchw


def _fill(dtype, B, H, W, Cr, seed) -> torch.Tensor:
    pool = _pool(dtype)
    n = B * H * W * Cr
    g = torch.Generator().manual_seed(seed)
    pick = torch.cat([torch.arange(len(SPECIALS)), torch.randint(0, len(pool), (n,), generator=g)])[:n]
    return pool[pick[torch.randperm(n, generator=g)]].view(B, H, W, Cr)


@pytest.fixture(scope="module")
def ops():
    return HipOps(DEV)


@pytest.mark.parametrize("shape", [(1, 1, 4), (3, 3, 5), (2, 4, 7), (2, 4, 8), (1, 3, 13), (2, 8, 12)])
@pytest.mark.parametrize("Cr", [1, 3, 4])
@pytest.mark.parametrize("halo", [0, 3])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_epilogue_equals_to_uint8(ops, dtype, halo, Cr, shape):
    B, H, W = shape
    vals = _fill(dtype, B, H, W, Cr, seed=B * 1000 + H * 100 + W * 10 + Cr)
    dst, nchw = _run_epilogue(ops, _poisoned_view(dtype, B, H, W, halo, Cr, vals), Cr)
    assert not bool(torch.isnan(nchw).any())
    want = I.to_uint8(nchw).permute(0, 2, 3, 1)
    assert torch.equal(dst, want), (dst.cpu() != want.cpu()).nonzero()[:4]


@pytest.mark.parametrize("W", [64, 61])          # dword path, byte path with a row tail
@pytest.mark.parametrize("halo", [0, 3])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_epilogue_value_sweep(ops, dtype, halo, W):
    """Every value of the sweep, on both store paths (the small shapes above draw samples of it)."""
    pool = _pool(dtype)
    B, Cr = 2, 3
    H = -(-len(pool) // (B * W * Cr))
    n = B * H * W * Cr
    vals = pool[torch.arange(n) % len(pool)].view(B, H, W, Cr)
    dst, nchw = _run_epilogue(ops, _poisoned_view(dtype, B, H, W, halo, Cr, vals), Cr)
    assert torch.equal(nchw.permute(0, 2, 3, 1).cpu(), vals)
    want = I.to_uint8(nchw).permute(0, 2, 3, 1)
    assert torch.equal(dst, want), (dst.cpu() != want.cpu()).nonzero()[:4]
    # and against the statement itself, in float64 with an explicit half-to-even: the products above are exact or far from a half
    # except at the tie inputs, where fp32 rounding of each step is part of the contract -- so only the monotone envelope is checked
    d = dst.cpu().double()
    exact = (vals.double().clamp(-1, 1) * 0.5 + 0.5) * 255
    assert float((d - exact).abs().max()) <= 0.5 + 1e-4


def test_epilogue_unaligned_destination_takes_the_byte_path(ops):
    B, H, W, Cr = 2, 4, 8, 3
    vals = _fill(F32, B, H, W, Cr, seed=7)
    for mis in (1, 2, 3):
        dst, nchw = _run_epilogue(ops, _poisoned_view(F32, B, H, W, 3, Cr, vals), Cr, misalign=mis)
        assert torch.equal(dst, I.to_uint8(nchw).permute(0, 2, 3, 1))


@pytest.mark.parametrize("shape", [(2, 4, 8), (2, 4, 7)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_epilogue_nan_reads_zero(ops, dtype, shape):
    """Exactly four NaN inputs: they read 0 (torch leaves that conversion undefined, so these four are exempt from the comparison);
    every other element, their neighbours included, still equals torch."""
    B, H, W = shape
    Cr = 3
    vals = _fill(dtype, B, H, W, Cr, seed=11)
    where = [(0, 0, 0, 0), (0, 1, W - 1, 2), (1, 2, 3, 1), (1, H - 1, W - 2, 0)]
    for p in where:
        vals[p] = float("nan")
    dst, nchw = _run_epilogue(ops, _poisoned_view(dtype, B, H, W, 3, Cr, vals), Cr)
    assert int(torch.isnan(nchw).sum()) == 4
    mask = torch.isnan(nchw).permute(0, 2, 3, 1)
    want = I.to_uint8(torch.nan_to_num(nchw, nan=-1.0)).permute(0, 2, 3, 1)
    assert bool((dst[mask] == 0).all())
    assert torch.equal(dst[~mask], want[~mask])


def test_epilogue_argument_checks(ops):
    v = _poisoned_view(F32, 1, 2, 4, 0, 3, torch.zeros(1, 2, 4, 3))
    for Cr in (0, 5):
        with pytest.raises(Exception, match="bad C"):
            ops._call("gan_view_to_u8_hwc", ops._v(v), Cr, ops._p(torch.zeros(64, dtype=torch.uint8, device=DEV)), ops._s())()


# ---------------------------------------------------------------------------------------------- forward_u8 / stylize_hwc
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("hw", [(16, 16), (16, 24)])
@pytest.mark.parametrize("B", [1, 3])
def test_forward_u8_equals_to_uint8_of_forward(B, hw, dtype, graph):
    torch.manual_seed(B * 100 + hw[1])
    G = C.ResNetGenerator(3, 3, ngf=8, n_blocks=2).to(DEV).eval()
    for p in G.parameters():
        p.requires_grad_(False)
    G.compute_dtype, G.use_graph = dtype, graph
    x = (torch.rand(B, 3, *hw) * 2 - 1).to(DEV)
    with torch.inference_mode():
        want = I.to_uint8(G(x)).permute(0, 2, 3, 1)
    a = I.stylize_hwc(G, x)
    b = G.forward_u8(x)
    torch.cuda.synchronize()
    assert a.dtype == torch.uint8 and a.shape == (B, hw[0], hw[1], 3) and a.is_contiguous() and a.data_ptr() != b.data_ptr()
    assert torch.equal(a, want) and torch.equal(b, want)
    assert torch.equal(I.stylize(G, x).permute(0, 2, 3, 1), want)          # the fp32 path of the same slot is unchanged
    assert int(want.max()) - int(want.min()) > 8                           # not a constant image


# ---------------------------------------------------------------------------------------------- input pipeline, BILINEAR
def _rand_image(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _host_bilinear(im, S):
    """What stylize_folder's host path feeds the generator for one photo (generate_folder.py:175-180), torch fp32 ops on the CPU."""
    from PIL import Image
    arr = np.asarray(Image.fromarray(im).resize((S, S), Image.BILINEAR), dtype=np.float32)
    return torch.from_numpy(arr)[None].permute(0, 3, 1, 2).div(255.0).sub(0.5).div(0.5).contiguous()[0]


def test_device_bilinear_pipeline_equals_pillow():
    rng = np.random.default_rng(13)
    S = 16
    sizes = [(20, 24), (37, 53), (16, 16), (9, 300), (300, 9), (7, 5)]
    imgs = [_rand_image(rng, h, w) for h, w in sizes]
    pipe = dataio.InputPipeline(S, DEV, max_batch=8, max_rows=64, filter=dataio.BILINEAR)
    cub = dataio.InputPipeline(S, DEV, max_batch=8, max_rows=64)
    low = [i for i, (h, _) in enumerate(sizes) if h <= 64]
    for batch in (low, list(range(len(sizes)))):          # the second batch holds a 300-row image: the buffer between the passes grows
        dev = [torch.from_numpy(imgs[i]).to(DEV) for i in batch]
        jobs = [dataio.infer_job(*sizes[i], S) for i in batch]
        out, out3 = pipe.run(dev, jobs), cub.run(dev, jobs)
        torch.cuda.synchronize()
        for n, i in enumerate(batch):
            assert torch.equal(out[n].cpu(), _host_bilinear(imgs[i], S)), ("bilinear", sizes[i])
            assert np.array_equal(out3[n].cpu().numpy(), R.apply_pil(imgs[i], jobs[n])), ("bicubic", sizes[i])
    assert pipe.max_rows >= 300 and cub.max_rows >= 300
    with pytest.raises(dataio.GanError):
        dataio.InputPipeline(S, DEV, filter=1)


# ---------------------------------------------------------------------------------------------- folder and command
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Five PNGs of mixed sizes with one sub-directory, a checkpoint, and the files the host path writes for it."""
    from PIL import Image
    root = tmp_path_factory.mktemp("infer_io")
    photos = root / "photos"
    (photos / "sub").mkdir(parents=True)
    rng = np.random.default_rng(17)
    for name, (h, w) in (("a.png", (20, 24)), ("b.png", (16, 16)), ("c.png", (45, 31)), ("sub/d.png", (9, 70)), ("sub/e.png", (64, 12))):
        Image.fromarray(_rand_image(rng, h, w)).save(photos / name)
    torch.manual_seed(19)
    G = C.ResNetGenerator(3, 3, ngf=8, n_blocks=2)
    ck = root / "ckpt_final.pt"
    torch.save({"generator": G.state_dict()}, ck)
    G = I.load_generator(str(ck), device="cuda:0", ngf=8, n_blocks=2)
    assert I.stylize_folder(G, str(photos), str(root / "host"), device="cuda:0", img_size=16, batch=2) == 5
    want = {p.relative_to(root / "host").as_posix(): p.read_bytes() for p in sorted((root / "host").rglob("*.jpg"))}
    assert sorted(want) == ["a.jpg", "b.jpg", "c.jpg", "sub/d.jpg", "sub/e.jpg"]
    return root, photos, ck, G, want


def _files(d):
    return {p.relative_to(d).as_posix(): p.read_bytes() for p in sorted(d.rglob("*")) if p.is_file()}


def test_folder_device_io_writes_the_same_files(folder):
    root, photos, ck, G, want = folder
    assert I.stylize_folder(G, str(photos), str(root / "dev"), device="cuda:0", img_size=16, batch=2, device_io=True) == 5
    assert _files(root / "dev") == want


def test_command_on_the_gpu(folder):
    root, photos, ck, G, want = folder
    cmd = [sys.executable, "-m", "gan_variant_research_amd.generate_folder", "--ckpt", str(ck), "--photos", str(photos), "--out", str(root / "cmd"),
           "--device", "cuda", "--size", "16", "--batch", "2", "--ngf", "8", "--n-blocks", "2"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device=cuda" in out.stdout and out.stdout.rstrip().endswith("Done.")
    assert _files(root / "cmd") == want
