"""gan_variant_research_amd.select_7k without a GPU: the host-layer bodies of tests/select_cases.py on the emulator of
tests/emulator_select.py, held to scikit-learn's recorded results (tests/golden/select_kmeans.npz; and to live scikit-learn where it
imports) and to the float64 statement of tests/select_ref64.py; the command line on a temporary folder tree; the C entries'
validation.  tests/test_select_gpu.py runs the same bodies on the HIP kernels."""
import csv
import json

import numpy as np
import pytest
import torch

from tests import select_cases as N
from tests.emulator_select import EmuU8Pipeline, SelectEmuOps


def make():
    return SelectEmuOps(), "cpu"


@pytest.mark.parametrize("name", list(N.KM_FIXTURES))
def test_kmeans_equals_scikit_learn(name):
    N.body_kmeans_fixture(make, name)


def test_kmeans_relocates_an_empty_cluster_as_scikit_learn_does():
    N.body_kmeans_empty_cluster(make)


def test_kmeans_refuses_more_clusters_than_rows():
    N.body_kmeans_refuses(make)


def test_golden_file_is_small_and_holds_no_centres():
    import os
    g = N.golden()
    assert os.path.getsize(N.GOLDEN) < 100_000 and not any("center" in k for k in g) and str(g["sklearn_version"])
    assert {f"{n}_{p}" for n in N.KM_FIXTURES for p in ("labels", "inertia", "n_iter")} | {"empty_labels"} <= set(g)


def test_selection_order_equals_the_statement():
    N.body_select(make)


def test_selection_with_fewer_kept_than_target(capsys):
    from gan_variant_research_amd import select_7k as S
    N.body_select(make, tau=0.22, target=480, short=True)
    real, cands = N.select_fixture()
    S.select(real, cands, k=16, target=480, device="cpu", ops=SelectEmuOps())
    assert "fewer than the target 480" in capsys.readouterr().out


def test_min_cos_dists_and_nearest_centre():
    from gan_variant_research_amd import evaluate as E, select_7k as S
    from tests import select_ref64 as R
    real, cands = N.select_fixture()
    ops = SelectEmuOps()
    assert np.array_equal(S.min_cos_dists(cands[0], real, "cpu", ops), E.cosine_min_distances(cands[0], real, "cpu", ops)[0])
    g = np.random.default_rng(3)
    cen, mean, scale = g.standard_normal((9, 96)), g.standard_normal(96), g.random(96) + 0.5
    d, idx = S.nearest_center_sqdist(cands[0], cen, mean, scale, "cpu", ops)
    ref, bound = R.sqdist(cands[0], cen, mean, scale)
    assert np.array_equal(idx, ref.argmin(1)) and np.all(np.abs(d - ref.min(1)) <= bound[np.arange(len(d)), idx])


def _image(i, h=24, w=20):
    g = np.random.default_rng(900 + i)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // w), (y * 255 // h), ((x + y) * 255 // (h + w))], -1).astype(np.float64)
    return np.clip(base * (0.3 + 0.05 * (i % 13)) + g.normal(0, 30, (h, w, 3)) + 5 * (i % 7), 0, 255).astype(np.uint8)


def test_command_line_on_a_folder_tree(tmp_path, monkeypatch, capsys):
    """Files are copied, a basename collision is counted, the reference's meta keys are present, --no-copy copies nothing,
    --cand-features gives the same selection as the folders."""
    from PIL import Image
    from gan_variant_research_amd import autograd as AG, dataio, evaluate as E, select_7k as S
    from tests import eval_extractor
    monkeypatch.setattr(AG, "_OPS_FACTORY", lambda device: SelectEmuOps())
    monkeypatch.setattr(dataio, "InputPipeline", EmuU8Pipeline)
    real, a, b = tmp_path / "real", tmp_path / "cand_a", tmp_path / "cand_b"
    for d in (real, a, b):
        d.mkdir()
    for i in range(8):
        Image.fromarray(_image(i)).save(real / f"r{i}.png")
    for i in range(10):
        Image.fromarray(_image(20 + i)).save(a / f"img_{i}.png")
        Image.fromarray(_image(40 + i)).save(b / f"img_{i}.png" if i < 4 else b / f"other_{i}.png")         # img_0..3 exist in both roots
    common = ["--real", str(real), "--cand_roots", str(a), str(b), "--tau", "0.0", "--k", "3", "--target", "17", "--device", "cpu", "--img-size", "32",
              "--batch", "4", "--extractor", "tests.eval_extractor:make"]
    out = tmp_path / "out"
    assert S.main([*common, "--outdir", str(out)]) == 0
    said = capsys.readouterr().out
    meta = json.load(open(out / "selection_meta.json"))
    assert {"real", "cand_roots", "tau", "k", "selected"} <= set(meta)
    assert meta["real"] == str(real) and meta["cand_roots"] == [str(a), str(b)] and meta["tau"] == 0.0 and meta["k"] == 3
    assert meta["selected"] == 17 and meta["candidates"] == 20 and meta["kept"] == 20 and meta["kmeans_n_iter"] >= 1 and meta["kmeans_inertia"] > 0
    rows = list(csv.DictReader(open(out / "selection.csv")))
    assert len(rows) == 17 and [int(r["rank"]) for r in rows] == list(range(1, 18))
    assert [float(r["score"]) for r in rows] == sorted(float(r["score"]) for r in rows)
    names = [p.rsplit("/", 1)[-1] for p in (r["path"] for r in rows)]
    assert meta["collisions"] == len(names) - len(set(names)) >= 1, "17 of 20 candidates with 4 shared names: at least one collision"
    assert sorted(p.name for p in (out / "images").iterdir()) == sorted(set(names))
    assert f"Selected 17 images into {out / 'images'}" in said and "share a file name" in said
    ext = eval_extractor.make("cpu")
    kw = dict(device="cpu", batch=4, img_size=32, io_threads=2)
    cp = E.enumerate_images(a) + E.enumerate_images(b)
    feats = [E.extract_features(E.enumerate_images(d), ext, **kw) for d in (real, a, b)]
    want = S.select(feats[0], feats[1:], tau=0.0, k=3, target=17, device="cpu", ops=SelectEmuOps())
    assert [r["path"] for r in rows] == [str(cp[i]) for i in want["chosen"]]
    assert all(r["nearest_real_path"].startswith(str(real)) for r in rows)

    dry = tmp_path / "dry"
    assert S.main([*common, "--outdir", str(dry), "--no-copy"]) == 0
    assert not (dry / "images").exists() and json.load(open(dry / "selection_meta.json"))["selected"] == 17
    for n, f in zip(("real", "a", "b"), feats):
        np.save(tmp_path / f"{n}.npy", f.numpy())
    ff = tmp_path / "ff"
    assert S.main(["--cand_roots", str(a), str(b), "--real-features", str(tmp_path / "real.npy"), "--cand-features", str(tmp_path / "a.npy"),
                   str(tmp_path / "b.npy"), "--outdir", str(ff), "--tau", "0.0", "--k", "3", "--target", "17", "--device", "cpu"]) == 0
    assert [r["path"] for r in csv.DictReader(open(ff / "selection.csv"))] == [r["path"] for r in rows]
    with pytest.raises(SystemExit):
        S.main(["--cand_roots", str(a), str(b), "--real", str(real), "--cand-features", str(tmp_path / "a.npy"), "--outdir", str(ff), "--device", "cpu"])


def test_c_entries_validate_before_they_launch():
    """The ABI contract of the selection entries through ctypes: every bad argument comes back as a non-zero code with a gan_last_error
    text that names it, before anything is launched or dereferenced, so no GPU is needed and the pointers are plain aligned numbers."""
    import ctypes as C
    from gan_variant_research_amd import _lib
    lib = _lib.load()
    P, Q = 1 << 20, (1 << 20) + 4
    F32, F64 = _lib.FEAT_F32, _lib.FEAT_F64
    err = lambda: lib.gan_last_error().decode()
    need = C.c_int64(0)
    assert lib.gan_sqdist_rowmin_bounds(70, 321, C.byref(need)) == 0 and need.value == (70 + 321) * 8 + 8 + 6 * 70 * 8 + 6 * 70 * 4
    assert need.value == SelectEmuOps().sqdist_rowmin_bounds(70, 321)
    assert lib.gan_sqdist_rowmin_bounds(3, 1, C.byref(need)) == 0 and need.value == 32 + 32 + 12 == SelectEmuOps().sqdist_rowmin_bounds(3, 1)
    assert lib.gan_sqdist_rowmin_bounds(0, 5, C.byref(need)) != 0 and "extents must be positive" in err()
    assert lib.gan_sqdist_rowmin_bounds(5, 2 ** 31 - 1, C.byref(need)) != 0 and "are refused" in err()
    assert lib.gan_sqdist_rowmin_bounds(5, 5, None) != 0 and "null output" in err()

    def sq(A=P, da=F32, lda=8, B=P, ldb=8, M=4, N=4, K=8, ws=P, ws_bytes=1 << 16, dmin=P, imin=P):
        return lib.gan_sqdist_rowmin(A, da, lda, B, F32, ldb, M, N, K, None, None, None, None, ws, ws_bytes, dmin, imin, None)

    for kw, text in ((dict(A=None), "null feature matrix"), (dict(B=None), "null feature matrix"), (dict(lda=5), "row stride 5 below the 8 columns"),
                     (dict(ldb=7), "row stride 7 below the 8 columns"), (dict(da=9), "dtype 9"), (dict(A=Q, da=F64), "misaligned"),
                     (dict(M=0), "extents must be positive"), (dict(dmin=None), "null output"), (dict(imin=None), "null output"),
                     (dict(ws=None), "workspace"), (dict(ws=P + 8), "16-byte aligned"), (dict(ws_bytes=64 + 32 + 16 - 1), "gan_sqdist_rowmin_bounds asks 112"),
                     (dict(M=65535 * 64 + 1), "beyond 65535 row tiles")):
        assert sq(**kw) != 0 and text in err(), (kw, err())

    def ku(X=P, dt=F32, n=4, D=8, ld=8, labels=P, k=3, sums=P, lds=8, counts=P, e=P):
        return lib.gan_kmeans_update(X, dt, n, D, ld, None, None, labels, k, sums, lds, counts, e, None)

    for kw, text in ((dict(X=None), "null feature matrix"), (dict(ld=7), "row stride 7 below the 8 columns"), (dict(n=0), "extents must be positive"),
                     (dict(labels=None), "null labels or output"), (dict(sums=None), "null labels or output"), (dict(counts=None), "null labels or output"),
                     (dict(e=None), "null labels or output"), (dict(sums=Q), "misaligned"), (dict(k=0), "k = 0"), (dict(k=-2), "k = -2"),
                     (dict(lds=7), "sums row stride 7 below the 8 columns"), (dict(D=65535 * 256 + 1, ld=1 << 30, lds=1 << 30), "beyond 65535 column strips")):
        assert ku(**kw) != 0 and text in err(), (kw, err())
