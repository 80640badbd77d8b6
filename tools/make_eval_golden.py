"""Records what the reference's evaluation code (EVAL/eval/mifid.py, features.py's compute_statistics, utils.py, report.py) gives on
seeded features, for the golden bodies of tests/mifid_cases.py to hold gan_variant_research_amd.evaluate to:

    python tools/make_eval_golden.py --reference PATH        # PATH holds EVAL/

The reference's modules are imported from PATH with `torchmetrics` stubbed in sys.modules (the recorded functions never call it), and
`tqdm` too where it is absent.  Writes tests/golden/eval_metric.npz (features, minimum distances, mu, sigma), tests/golden/eval_metric.json
(statistics, worst cases, the hash of a generated tree and the tree, the validation and overlap results, a report) and copies the
reference's sample report to tests/golden/eval_sample_report.json.  Only results are recorded; none of the reference's program text is."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NR, NF, D, SEED = 33, 17, 40, 20251
TREE = [("a/img_002.jpg", 11), ("a/img_001.png", 7), ("b/c/deep.JPEG", 3), ("top.PNG", 5), ("z_last.jpeg", 13), ("notes.txt", 9), ("a/skip.Jpg", 4)]


def stub(name, **attrs):
    m = sys.modules.get(name) or types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def features():
    g = np.random.default_rng(SEED)
    base = g.standard_normal(D)
    real = np.maximum(g.standard_normal((NR, D)) * 0.8 + 0.3 * base, 0).astype(np.float32)
    fake = np.maximum(g.standard_normal((NF, D)) * 0.8 + 0.3 * base + 0.15, 0).astype(np.float32)
    fake[5] = real[20] * 1.5 + 0.01 * fake[5]            # one near copy: a clear worst case
    return real, fake


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    ev = os.path.join(args.reference, "EVAL")
    sys.dont_write_bytecode = True                       # the reference tree stays as it is
    stub("eval", __path__=[os.path.join(ev, "eval")])    # the package without its __init__, which imports the torchvision loaders
    for name in ("torchmetrics", "torchmetrics.image", "torchmetrics.image.mifid", "torchmetrics.image.fid"):
        stub(name)
    stub("torchmetrics.image.mifid", MemorizationInformedFrechetInceptionDistance=object)
    stub("torchmetrics.image.fid", FrechetInceptionDistance=object)
    try:
        import tqdm  # noqa: F401
    except ImportError:
        stub("tqdm", tqdm=lambda it, **kw: it)
    from eval import mifid as M, report as P, utils as U

    real, fake = features()
    fake_paths = [Path(f"/data/fake/img_{i:03d}.jpg") for i in range(NF)]
    real_paths = [Path(f"/data/monet/monet_{i:03d}.jpg") for i in range(NR)]
    dmin = M.compute_cosine_distances_batched(fake, real, batch_size=7)
    stats = M.compute_cosine_distance_statistics(dmin)
    worst = M.find_worst_memorization_cases(fake_paths, dmin, real_paths, real, fake, top_k=16)
    mu, sigma = np.mean(real, axis=0), np.cov(real, rowvar=False)          # compute_statistics' two lines (its class needs torchmetrics)

    with tempfile.TemporaryDirectory() as tmp:
        for rel, size in TREE:
            p = Path(tmp) / rel
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_bytes(b"x" * size)
        imgs = U.enumerate_images(tmp)
        flat = U.enumerate_images(tmp, recursive=False)
        sha = U.compute_image_list_hash(imgs, Path(tmp))
        sha_abs_free = U.compute_image_list_hash([Path(tmp) / "a" / "img_002.jpg"], Path(tmp) / "a")
        validation = U.validate_image_counts(imgs, flat)
        overlap = U.check_dataset_overlap(imgs, flat)
        listed = [p.relative_to(tmp).as_posix() for p in imgs]
        listed_flat = [p.relative_to(tmp).as_posix() for p in flat]

    scores = {"mifid": 41.23456789, "fid": 45.10987654, "cosine_min_distance": stats}
    run_config = {"name": "golden", "fake_dir": "/data/fake", "real_mode": "folder", "real_dir": "/data/monet", "img_size": 299, "batch_size": 32,
                  "num_workers": 4}
    hashes = {"fake_list_sha1": sha, "real_list_sha1": sha_abs_free, "real_cache_key": f"monet_jpg@sha1:{sha_abs_free[:16]}"}
    report = P.create_report(scores, run_config, hashes, validation, worst)

    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN, "eval_metric.npz"), real=real, fake=fake, min_distances=dmin, mu=mu, sigma=sigma)
    with open(os.path.join(GOLDEN, "eval_metric.json"), "w") as f:
        json.dump({"fake_paths": [str(p) for p in fake_paths], "real_paths": [str(p) for p in real_paths], "stats": stats, "worst": worst,
                   "tree": TREE, "enumerated": listed, "enumerated_flat": listed_flat, "sha1": sha, "sha1_single": sha_abs_free,
                   "validation": validation, "overlap": overlap, "report_inputs": {"scores": scores, "run_config": run_config, "hashes": hashes},
                   "report": report}, f, indent=1)
    shutil.copyfile(os.path.join(ev, "cache", "reports", "sample_report.json"), os.path.join(GOLDEN, "eval_sample_report.json"))
    os.chmod(os.path.join(GOLDEN, "eval_sample_report.json"), 0o644)
    print(f"wrote eval_metric.npz, eval_metric.json, eval_sample_report.json under {GOLDEN}")


if __name__ == "__main__":
    main()
