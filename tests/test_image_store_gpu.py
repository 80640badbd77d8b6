"""dataio.ImageStore on the device, built with the index-less `torch.device("cuda")`: the four reference transforms fed from `store[i]`
(views into the arena; odd widths put rows and image ends at odd byte offsets) equal the Pillow restatement bit for bit -- the contract of
test_input_pipeline.test_device_pipeline_equals_pillow -- and the resident and the streaming store give identical batches."""
import numpy as np
import pytest
import torch
from PIL import Image

from gan_variant_research_amd import dataio
from oracle import input_ref as R

SIZES = [(5, 7), (33, 130), (64, 64), (70, 41)]
TRANSFORMS = {"train": lambda dev: dataio.get_train_transforms(32, device=dev), "eval": lambda dev: dataio.get_eval_transforms(32, device=dev),
              "basic_train": lambda dev: dataio.basic_image_tf(36, 32, True, device=dev), "basic_eval": lambda dev: dataio.basic_image_tf(36, 32, False, device=dev)}


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """PNGs of SIZES (photo-like content, so that saturation and hue see chroma) -> (sorted paths, decoded arrays)."""
    root = tmp_path_factory.mktemp("store")
    rng = np.random.default_rng(5)
    for n, (h, w) in enumerate(SIZES):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([127 + 120 * np.sin(yy / 17.0 + c) * np.cos(xx / 23.0 - c) for c in range(3)], -1)
        Image.fromarray(np.clip(base + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)).save(root / f"img_{n}.png")
    paths = sorted(root.iterdir())
    return paths, [np.array(Image.open(p).convert("RGB")) for p in paths]


@pytest.fixture(scope="module")
def stores(folder):
    dev = torch.device("cuda")
    resident, streaming = dataio.ImageStore(folder[0], dev), dataio.ImageStore(folder[0], dev, budget_bytes=1)
    assert resident.resident and not streaming.resident
    yield resident, streaming
    streaming.close()


@pytest.mark.gpu
def test_store_on_an_index_less_device_holds_pillows_pixels(folder, stores):
    paths, want = folder
    for store in stores:
        assert store.device == torch.device("cuda", torch.cuda.current_device()) and len(store) == 4 and store.sizes == SIZES
        for i, (t, f) in enumerate(zip(store.fetch(range(4)), [store[i] for i in range(4)])):
            for x in (t, f):
                assert x.device == store.device and x.dtype == torch.uint8 and x.stride() == (3 * SIZES[i][1], 3, 1)
                assert np.array_equal(x.cpu().numpy(), want[i]), i
    res = stores[0]
    assert all(o % 256 == 0 for o in res.offsets) and res.arena.data_ptr() % 256 == 0
    assert [res[i].data_ptr() - res.arena.data_ptr() for i in range(4)] == res.offsets


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(TRANSFORMS))
def test_transforms_fed_from_the_store_equal_pillow(folder, stores, kind):
    _, want = folder
    tf = TRANSFORMS[kind](torch.device("cuda"))             # index-less, as the drivers build it
    outs = []
    for store in stores:
        np.random.seed(31); torch.manual_seed(31)
        out = tf([store[i] for i in range(4)])
        torch.cuda.synchronize()
        assert out.shape == (4, 3, 32, 32) and out.dtype == torch.float32
        for b, (img, job) in enumerate(zip(want, tf.last_jobs)):
            ref = R.apply(img, job)
            assert np.array_equal(out[b].cpu().numpy(), ref), (kind, store.resident, b, job, float(np.abs(out[b].cpu().numpy() - ref).max()))
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    np.random.seed(31); torch.manual_seed(31)
    assert torch.equal(tf(stores[1].fetch(range(4))), outs[0])          # the pool's batch upload: the same images again
