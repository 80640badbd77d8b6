"""dataio.ImageStore on a CPU device: a folder decoded once with Pillow, resident (one arena, every image at a multiple of 256 bytes) or
streaming (decoded per call), the same tensors either way; an empty list and an unreadable file are errors that name the place."""
import numpy as np
import pytest
import torch
from PIL import Image

from gan_variant_research_amd import dataio

RGB_SIZES = [(1, 1), (5, 7), (33, 130), (64, 64)]


def _write_folder(root):
    """RGB PNGs of RGB_SIZES plus one image each of mode L, RGBA and P; returns the sorted paths."""
    rng = np.random.default_rng(11)
    root.mkdir()
    for n, (h, w) in enumerate(RGB_SIZES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / f"rgb{n}.png")
    Image.fromarray(rng.integers(0, 256, (9, 12), dtype=np.uint8), "L").save(root / "grey.png")
    Image.fromarray(rng.integers(0, 256, (10, 6, 4), dtype=np.uint8), "RGBA").save(root / "alpha.png")
    pal = Image.fromarray(rng.integers(0, 256, (7, 11), dtype=np.uint8), "P")
    pal.putpalette([int(v) for v in rng.integers(0, 256, 768)])
    pal.save(root / "palette.png")
    return sorted(root.iterdir())


def _expect(paths):
    return [np.array(Image.open(p).convert("RGB")) for p in paths]


def _check(t, want):
    assert t.dtype == torch.uint8 and t.device.type == "cpu" and tuple(t.shape) == want.shape
    assert t.stride(2) == 1 and t.stride(1) == 3 and t.stride(0) == 3 * want.shape[1]
    assert np.array_equal(t.numpy(), want)


@pytest.mark.parametrize("workers", [None, 1, 64])
def test_resident_store_holds_pillows_pixels(tmp_path, workers):
    paths = _write_folder(tmp_path / "imgs")
    want = _expect(paths)
    store = dataio.ImageStore(paths, torch.device("cpu"), workers=workers)
    assert store.resident and len(store) == len(paths) == 7 and 1 <= store.workers <= 16
    assert store.sizes == [w.shape[:2] for w in want] and store.nbytes == sum(w.size for w in want)
    assert all(o % 256 == 0 for o in store.offsets) and store.offsets == sorted(set(store.offsets))
    for i, w in enumerate(want):
        _check(store[i], w)
        assert store[i].data_ptr() == store.arena.data_ptr() + store.offsets[i]          # a view into the arena
        assert store.offsets[i] + w.size <= store.arena.numel()
    _check(store[-1], want[-1])
    for t, w in zip(store.fetch([3, 0, 3]), [want[3], want[0], want[3]]):
        _check(t, w)
    with pytest.raises(IndexError):
        store[len(paths)]


def test_streaming_store_hands_out_the_same_tensors(tmp_path):
    paths = _write_folder(tmp_path / "imgs")
    want = _expect(paths)
    store = dataio.ImageStore(paths, "cpu", budget_bytes=1)
    assert not store.resident and store.arena is None and store.sizes == [w.shape[:2] for w in want]
    order = [6, 0, 2, 2, 5, 1, 3, 4]
    for i, t in zip(order, store.fetch(order)):
        _check(t, want[i])
        _check(store[i], want[i])
    store[0][0, 0, 0] += 1            # writable, and nothing is kept: the next read decodes again
    _check(store[0], want[0])
    store.close()
    # the budget is compared with the arena's size
    exact = dataio.ImageStore(paths, "cpu")
    assert dataio.ImageStore(paths, "cpu", budget_bytes=exact.arena.numel()).resident
    assert not dataio.ImageStore(paths, "cpu", budget_bytes=exact.arena.numel() - 1).resident


def test_errors_name_the_place(tmp_path):
    with pytest.raises(FileNotFoundError, match="some/folder"):
        dataio.ImageStore([], "cpu", folder="some/folder")
    with pytest.raises(FileNotFoundError):
        dataio.ImageStore([], "cpu")
    paths = _write_folder(tmp_path / "imgs")
    whole = paths[5].read_bytes()          # the 33 x 130 image
    for cut, name in ((len(whole) // 2, "half.png"), (6, "stub.png")):       # pixel data cut short; not even a header
        bad = tmp_path / "imgs" / name
        bad.write_bytes(whole[:cut])
        for budget in (None, 1):
            with pytest.raises(OSError, match=name):
                store = dataio.ImageStore(paths + [bad], "cpu", budget_bytes=budget)
                store.fetch(range(len(store)))
