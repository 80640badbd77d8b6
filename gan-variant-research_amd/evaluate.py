"""Evaluation: FID, MiFID and the memorisation analysis of the reference's third stage (EVAL/), from image folders to the report.

    python -m gan_variant_research_amd.evaluate --fake F --real R --extractor pkg.module:factory --out report.json

What runs where.  Images are decoded by `dataio.DeviceDecoder` or a Pillow pool, resized on the device by
`dataio.InputPipeline(img_size, filter=BILINEAR).run_u8` (the bytes of the reference's loader, EVAL/eval/datasets.py:52-66), and handed
to a feature extractor: a callable from a uint8 (B, 3, S, S) device tensor to (B, D) features.  The extractor is a plug-in -- the
reference borrows torchmetrics' Inception module and so does this command when that package imports; `--extractor` names any other.
Everything after the features runs on the kernels of csrc/mifid.hip (`HipOps.feat_moments`, `gram_f64`, `cos_rowmin`), in float64:

  * the Frechet term through the identity   tr sqrt(Sr Sf) = sum of the singular values of  M = Rc Fc^T / sqrt((nr - 1)(nf - 1))
    (Rc, Fc the column-centred features; the non-zero eigenvalues of Sr Sf are the squared singular values of M).  `route="gram"`
    computes M (nr x nf) on the device and the host takes its singular values; `route="cov"` computes both D x D covariances on the
    device, the host factors each (eigh, negative eigenvalues clipped: L = V sqrt(L)), the device forms Lr^T Lf and the host takes its
    singular values.  The reference's metric (torchmetrics) takes eigvals of the non-symmetric D x D product instead, whose null
    eigenvalues are noise of order sqrt(u) lambda_max when a set has fewer rows than D; neither route here forms that product.
  * the memorisation distance and the reference's cosine analysis through the row-minimum kernel, which never writes the nr x nf matrix.

Host LAPACK (numpy, float64) on a matrix whose small side is at most min(nr, nf, D) is the boundary of the device path.  There is no
fallback: without the library every function here raises.
"""
from __future__ import annotations

import argparse
import csv
import hashlib
import importlib
import json
import math
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from datetime import datetime, timezone
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dataio

IMG_SUFFIXES = (".jpg", ".jpeg", ".png", ".JPG", ".JPEG", ".PNG")      # utils.py:32-42: each extension as written and upper-cased
NO_EXTRACTOR = ("no feature extractor: torchmetrics does not import here, so name one with --extractor pkg.module:factory, or give "
                "precomputed features with --real-features FILE and --fake-features FILE")


# ------------------------------------------------------------------------------------------------ features on the device
class Features:
    """A feature matrix on the device with its moments (one `feat_moments` launch, downloaded once)."""

    def __init__(self, x, device=None, ops=None, name: str = "features"):
        if isinstance(x, Features):
            self.__dict__.update(x.__dict__)
            return
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
        if x.dim() != 2:
            raise ValueError(f"{name}: a feature matrix is 2-D, got shape {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
        if ops is None:
            from . import autograd as AG
            device = dataio.normalize_device(device if device is not None else (x.device if x.device.type == "cuda" else "cuda"))
            ops = AG._OPS_FACTORY(device)
        elif device is None:
            device = x.device
        x = x.to(device)
        if x.shape[1] > 1 and x.stride(1) != 1:
            x = x.contiguous()
        self.x, self.ops, self.name = x, ops, name
        self.n, self.D = int(x.shape[0]), int(x.shape[1])
        if self.n < 2:
            raise ValueError(f"{name}: {self.n} row(s); a mean and a covariance need at least 2")
        if self.D < 1:
            raise ValueError(f"{name}: no feature columns")
        self.m = ops.feat_moments(x)
        if int(self.m["flag"].cpu()[0]) != 0:
            raise ValueError(f"{name}: a feature is NaN or Inf")
        self.mu = self.m["mean"].cpu().numpy()
        self.css = float(self.m["css"].cpu()[0])

    @property
    def trace(self) -> float:
        """tr cov (divisor n - 1), from the centred sums of squares."""
        return self.css / (self.n - 1)


def _pair(real, fake, device, ops) -> Tuple[Features, Features]:
    r = Features(real, device, ops, "real features")
    f = Features(fake, r.x.device if device is None else device, r.ops if ops is None else ops, "fake features")
    if r.D != f.D:
        raise ValueError(f"real features have D = {r.D}, fake features D = {f.D}: they must come from one extractor")
    return r, f


# ------------------------------------------------------------------------------------------------ statistics and their cache
def feature_statistics(features, device=None, ops=None) -> Tuple[np.ndarray, np.ndarray]:
    """InceptionFeatureExtractor.compute_statistics (features.py:79-94): (mu, sigma) in float64, sigma = np.cov(features, rowvar=False)
    (divisor n - 1), contracted over the rows on the device."""
    f = Features(features, device, ops)
    sigma = f.ops.gram_f64(f.x, f.x, 1, ca=f.m["mean"], cb=f.m["mean"], alpha=1.0 / (f.n - 1))
    return f.mu.copy(), sigma.cpu().numpy()


def save_cached_stats(cache_key: str, cache_dir, mu, sigma, features=None, n: Optional[int] = None) -> Path:
    """The reference's cache file (features.py:148-184): <cache_dir>/<cache_key>.npz with mu, sigma, n and, optionally, features."""
    cache_dir = Path(cache_dir)
    cache_dir.mkdir(parents=True, exist_ok=True)
    path = cache_dir / f"{cache_key}.npz"
    d = {"mu": np.asarray(mu), "sigma": np.asarray(sigma), "n": int(n) if n is not None else (len(features) if features is not None else 0)}
    if features is not None:
        d["features"] = np.asarray(features)
    np.savez_compressed(path, **d)
    return path


def load_cached_stats(cache_key: str, cache_dir) -> Optional[Dict]:
    """features.py:112-145: the cache file's mu, sigma, n (int) and features if it has them; None when there is no readable file."""
    path = Path(cache_dir) / f"{cache_key}.npz"
    if not path.exists():
        return None
    try:
        with np.load(path, allow_pickle=False) as z:
            out = {"mu": z["mu"], "sigma": z["sigma"], "n": int(z["n"])}
            if "features" in z.files:
                out["features"] = z["features"]
        return out
    except Exception as e:
        print(f"cache {path.name} is unreadable ({e}); recomputing", file=sys.stderr)
        return None


# ------------------------------------------------------------------------------------------------ the Frechet distance
def frechet_terms(real, fake, route: str = "auto", device=None, ops=None) -> Dict[str, float]:
    """The parts of the distance: dmu2 = |mu_r - mu_f|^2, tr_r, tr_f, c = tr sqrt(Sr Sf), and the route taken."""
    r, f = _pair(real, fake, device, ops)
    if route == "auto":
        route = "gram" if min(r.n, f.n) <= r.D else "cov"
    if route == "gram":
        M = r.ops.gram_f64(r.x, f.x, 0, ca=r.m["mean"], cb=f.m["mean"], alpha=1.0 / math.sqrt((r.n - 1.0) * (f.n - 1.0)))
        c = float(np.linalg.svd(M.cpu().numpy(), compute_uv=False).sum())
    elif route == "cov":
        factors = []
        for s in (r, f):
            sigma = s.ops.gram_f64(s.x, s.x, 1, ca=s.m["mean"], cb=s.m["mean"], alpha=1.0 / (s.n - 1))
            lam, V = np.linalg.eigh(sigma.cpu().numpy())
            factors.append(torch.from_numpy(np.ascontiguousarray(V * np.sqrt(np.clip(lam, 0.0, None)))).to(s.x.device))
        P = r.ops.gram_f64(factors[0], factors[1], 1)            # Lr^T Lf, contracted over the rows of both factors
        c = float(np.linalg.svd(P.cpu().numpy(), compute_uv=False).sum())
    else:
        raise ValueError(f"route = {route!r}: one of 'auto', 'gram', 'cov'")
    d = r.mu - f.mu
    return {"dmu2": float(d @ d), "tr_r": r.trace, "tr_f": f.trace, "c": c, "route": route}


def frechet_distance(real, fake, route: str = "auto", device=None, ops=None) -> float:
    """|mu_r - mu_f|^2 + tr Sr + tr Sf - 2 tr sqrt(Sr Sf); route "gram" | "cov" | "auto" (gram when min(nr, nf) <= D)."""
    t = frechet_terms(real, fake, route, device, ops)
    return t["dmu2"] + t["tr_r"] + t["tr_f"] - 2.0 * t["c"]


# ------------------------------------------------------------------------------------------------ cosine distances
def cosine_min_distances(fake, real, device=None, ops=None) -> Tuple[np.ndarray, np.ndarray]:
    """compute_cosine_distances_batched (mifid.py:109-147) in float64: rows divided by (norm + 1e-8), d = 1 - cos (signed), the minimum
    over the real rows for every fake row.  Also the index of the nearest real row (the lowest on a tie, as np.argmax of the
    similarities gives), which the reference finds with a second matrix product."""
    r, f = _pair(real, fake, device, ops)
    d, idx = f.ops.cos_rowmin(f.x, r.x, ra=1.0 / (f.m["norm"] + 1e-8), rb=1.0 / (r.m["norm"] + 1e-8), absolute=False)
    return d.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def cosine_distance_statistics(min_distances) -> Dict:
    """compute_cosine_distance_statistics (mifid.py:150-178): median, mean, std, 10th and 90th percentile, a 10-bin histogram."""
    d = np.asarray(min_distances, dtype=np.float64)
    counts, bins = np.histogram(d, bins=10)
    return {"median": float(np.median(d)), "mean": float(np.mean(d)), "std": float(np.std(d)), "p10": float(np.percentile(d, 10)),
            "p90": float(np.percentile(d, 90)), "hist_bins": bins.tolist(), "hist_counts": counts.tolist()}


def worst_memorization_cases(fake_paths: Sequence, min_distances, real_paths: Sequence, nearest, top_k: int = 16) -> List[Dict]:
    """find_worst_memorization_cases (mifid.py:181-228): the top_k fake images closest to the real set, ordered by (distance, index),
    each with its nearest real image -- taken from the row-minimum kernel's index instead of a second matrix product."""
    d = np.asarray(min_distances, dtype=np.float64)
    order = np.lexsort((np.arange(len(d)), d))[:top_k]
    return [{"fake_path": str(fake_paths[i]), "distance": float(d[i]), "nearest_real_path": str(real_paths[int(nearest[i])]),
             "cosine_similarity": float(1.0 - d[i])} for i in order]


def memorization_distance(real, fake, cosine_eps: float = 0.1, rows: str = "real", device=None, ops=None) -> float:
    """The memorisation term of MiFID as torchmetrics defines it (the definition the reference calls), restated: rows whose element sum
    is exactly 0 leave both sets; rows are divided by their norm (no epsilon); d = 1 - |cos|; the mean over the `rows` set of the
    minimum over the other set; that mean if it is below cosine_eps, else 1.
    rows="real" is torchmetrics' orientation (for every real image its nearest fake one); rows="fake" is the Kaggle competition's
    original one (for every generated image its nearest real one)."""
    if rows not in ("real", "fake"):
        raise ValueError(f"rows = {rows!r}: 'real' (torchmetrics) or 'fake' (Kaggle)")
    r, f = _pair(real, fake, device, ops)
    scale = {}
    for s in (r, f):
        keep = s.m["rowsum"] != 0
        if not bool(keep.any()):
            raise ValueError(f"{s.name}: every row sums to exactly 0, nothing is left after the zero-sum filter")
        scale[s] = torch.where(keep, 1.0 / s.m["norm"], torch.zeros_like(s.m["norm"]))        # 0 marks "left out" for the kernel
    a, b = (r, f) if rows == "real" else (f, r)
    d, _ = a.ops.cos_rowmin(a.x, b.x, ra=scale[a], rb=scale[b], absolute=True)
    d = d.cpu().numpy()[(scale[a] != 0).cpu().numpy()]
    mean = float(d.mean())
    return mean if mean < cosine_eps else 1.0


def mifid(real, fake, cosine_eps: float = 0.1, device=None, ops=None) -> Dict[str, float]:
    """{"fid", "distance", "mifid"}: mifid = fid / (distance + 1e-14) when fid > 1e-8, else 0 (torchmetrics' _mifid_compute)."""
    r, f = _pair(real, fake, device, ops)
    fid = frechet_distance(r, f)
    distance = memorization_distance(r, f, cosine_eps)
    return {"fid": fid, "distance": distance, "mifid": fid / (distance + 1e-14) if fid > 1e-8 else 0.0}


def full_evaluation(real_features, fake_features, fake_paths: Sequence, real_paths: Sequence, cosine_eps: float = 0.1, device=None, ops=None) -> Dict:
    """compute_full_evaluation (mifid.py:231-292) from features: mifid, fid, the statistics of the minimum cosine distances and the 16
    worst memorisation cases."""
    r, f = _pair(real_features, fake_features, device, ops)
    if len(fake_paths) != f.n or len(real_paths) != r.n:
        raise ValueError(f"{len(fake_paths)} fake paths for {f.n} rows, {len(real_paths)} real paths for {r.n} rows")
    m = mifid(r, f, cosine_eps)
    d, nearest = cosine_min_distances(f, r)
    return {"mifid": m["mifid"], "fid": m["fid"], "cosine_min_distance": cosine_distance_statistics(d),
            "worst_memorization_cases": worst_memorization_cases(fake_paths, d, real_paths, nearest, top_k=16)}


# ------------------------------------------------------------------------------------------------ folders (EVAL/eval/utils.py)
def enumerate_images(path, recursive: bool = True) -> List[Path]:
    """Every *.jpg / *.jpeg / *.png (as written or upper-cased) below `path`, sorted (utils.py:13-46)."""
    root = Path(path)
    if not root.exists():
        raise FileNotFoundError(f"Path does not exist: {path}")
    if not root.is_dir():
        raise NotADirectoryError(f"Path is not a directory: {path}")
    found = root.rglob("*") if recursive else root.glob("*")
    return sorted({p for p in found if p.name.endswith(IMG_SUFFIXES)})


def compute_image_list_hash(image_paths: Sequence[Path], base_path: Optional[Path] = None) -> str:
    """SHA-1 over "<posix path relative to base_path>:<file size>\\n" of the sorted paths (utils.py:49-86)."""
    h = hashlib.sha1()
    for p in sorted(image_paths):
        rel = p
        if base_path:
            try:
                rel = p.relative_to(base_path)
            except ValueError:
                pass
        try:
            size = p.stat().st_size
        except OSError:
            size = 0
        h.update(f"{rel.as_posix()}:{size}\n".encode("utf-8"))
    return h.hexdigest()


def validate_image_counts(fake_images: Sequence[Path], real_images: Sequence[Path]) -> Dict:
    """Counts, sizes and the reference's warnings about them (utils.py:89-132): 7000-10000 generated images, at least 300 real ones."""
    nf, nr = len(fake_images), len(real_images)
    warnings = []
    if nf < 7000:
        warnings.append(f"Fake image count ({nf}) is below expected range (7000-10000)")
    elif nf > 10000:
        warnings.append(f"Fake image count ({nf}) is above expected range (7000-10000)")
    if nr < 300:
        warnings.append(f"Real image count ({nr}) is below expected minimum (300)")
    if nf == 0:
        raise ValueError("No fake images found!")
    if nr == 0:
        raise ValueError("No real images found!")
    mb = lambda ps: sum(p.stat().st_size for p in ps) / (1024 * 1024)
    return {"num_fake": nf, "num_real": nr, "fake_total_mb": mb(fake_images), "real_total_mb": mb(real_images), "warnings": warnings,
            "valid": not warnings}


def check_dataset_overlap(fake_paths: Sequence[Path], real_paths: Sequence[Path]) -> Dict:
    """File names that occur in both sets (utils.py:135-156)."""
    both = {p.name for p in fake_paths} & {p.name for p in real_paths}
    return {"has_overlap": bool(both), "overlap_count": len(both), "overlap_examples": sorted(both)[:10]}


# ------------------------------------------------------------------------------------------------ images -> features
@torch.inference_mode()
def extract_features(paths: Sequence, extractor: Callable, device, batch: int = 64, img_size: int = 299, io_threads: int = 8,
                     device_decode: bool = False, device_png: bool = False, device_progressive: bool = False) -> torch.Tensor:
    """The reference's loader and feature loop (datasets.py:52-66, features.py:44-77) on the device: decode (DeviceDecoder for the formats
    asked, Pillow on a pool of io_threads otherwise), `Image.resize((S, S), BILINEAR)` as InputPipeline.run_u8, then
    extractor(uint8 (B, 3, S, S)) -> (B, D).  Returns the (N, D) features, on the device."""
    device = dataio.normalize_device(device)
    paths = list(paths)
    if not paths:
        raise ValueError("extract_features: no images")
    if batch < 1 or io_threads < 1:
        raise ValueError(f"extract_features: batch = {batch}, io_threads = {io_threads}: at least 1 each")
    pipe = dataio.InputPipeline(img_size, device, max_batch=batch, filter=dataio.BILINEAR)
    if device_progressive and not device_decode:
        raise ValueError("device_progressive needs device_decode")
    dec = dataio.DeviceDecoder(device, jpeg=device_decode, png=device_png, progressive=device_progressive) if device_decode or device_png else None
    feats = []
    with ThreadPoolExecutor(min(io_threads, 16)) as pool:
        for at in range(0, len(paths), batch):
            chunk = paths[at:at + batch]
            if dec is not None:
                images = dec.decode(chunk, each=pool.map)
            else:
                images = [torch.from_numpy(a).to(device) for a in pool.map(dataio._decode, chunk)]
            u8 = pipe.run_u8(images, [dataio.infer_job(int(im.shape[0]), int(im.shape[1]), img_size) for im in images])
            f = extractor(u8)
            if not isinstance(f, torch.Tensor) or f.dim() != 2 or f.shape[0] != len(chunk) or not f.is_floating_point():
                raise ValueError(f"the extractor must return a floating (B, D) tensor for a (B, 3, S, S) batch, got {getattr(f, 'shape', type(f))}")
            feats.append(f if f.dtype in (torch.float32, torch.float64) else f.float())
    return torch.cat(feats).to(device)


def load_extractor(spec: Optional[str], device) -> Callable:
    """`pkg.module:factory` -> factory(device); None: torchmetrics' Inception module, the reference's extractor, if that package imports."""
    if spec:
        mod, _, attr = spec.partition(":")
        if not attr:
            raise ValueError(f"--extractor {spec!r}: expected pkg.module:factory")
        return getattr(importlib.import_module(mod), attr)(device)
    try:
        from torchmetrics.image.fid import FrechetInceptionDistance
    except ImportError:
        raise SystemExit(NO_EXTRACTOR) from None
    inception = FrechetInceptionDistance(feature=2048, normalize=False).to(device).inception.eval()
    return lambda u8: inception(u8)


def load_features(path) -> np.ndarray:
    """A feature file: a .npy array, or the cache .npz with its `features`."""
    path = Path(path)
    if path.suffix == ".npz":
        with np.load(path, allow_pickle=False) as z:
            if "features" not in z.files:
                raise ValueError(f"{path}: a cache file without `features` (it holds {z.files})")
            return z["features"]
    return np.load(path, allow_pickle=False)


# ------------------------------------------------------------------------------------------------ reports (EVAL/eval/report.py)
NOTES = ("MiFID/FID over features of the named extractor (the reference's: InceptionV3 pool3, 2048 dims). uint8 input [0,255] resized to "
         "img_size x img_size, bilinear. FID through the singular values of the centred cross-Gram matrix, float64. "
         "MiFID = FID / M where M is the memorization penalty from the mean minimum cosine distance.")


def create_report(scores: Dict, run_config: Dict, hashes: Dict, validation: Dict, worst_cases: Optional[list] = None) -> Dict:
    """The report of report.py:12-66: run, scores (mifid and fid rounded to 4 places), hashes, notes, memorization_analysis."""
    report = {
        "run": {"name": run_config.get("name", "unnamed_run"),
                "timestamp_utc": datetime.now(timezone.utc).replace(tzinfo=None).isoformat() + "Z",
                "fake_dir": str(run_config.get("fake_dir", "")),
                "real_mode": run_config.get("real_mode", "folder"),
                "real_dir_or_tfds": str(run_config.get("real_dir", "")),
                "num_fake": validation.get("num_fake", 0),
                "num_real": validation.get("num_real", 0),
                "img_size": run_config.get("img_size", 299),
                "batch_size": run_config.get("batch_size", 64),
                "num_workers": run_config.get("num_workers", 8),
                "warnings": validation.get("warnings", [])},
        "scores": {"mifid": round(scores.get("mifid", 0.0), 4), "fid": round(scores.get("fid", 0.0), 4),
                   "cosine_min_distance": scores.get("cosine_min_distance", {})},
        "hashes": hashes,
        "notes": NOTES,
    }
    if worst_cases:
        report["memorization_analysis"] = {"worst_cases": worst_cases,
                                           "description": "Top-16 fake images with smallest cosine distance to real set (highest memorization risk)"}
    return report


def save_report(report: Dict, output_path, verbose: bool = True) -> None:
    path = Path(output_path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as f:
        json.dump(report, f, indent=2)
    if verbose:
        print(f"Report saved to: {path}")


def save_worst_cases_csv(worst_cases: Sequence[Dict], output_path) -> None:
    """report.py:192-218: rank, fake_path, distance, cosine_similarity, nearest_real_path."""
    path = Path(output_path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["rank", "fake_path", "distance", "cosine_similarity", "nearest_real_path"])
        for i, c in enumerate(worst_cases, 1):
            w.writerow([i, c["fake_path"], f"{c['distance']:.6f}", f"{c['cosine_similarity']:.6f}", c["nearest_real_path"]])


# ------------------------------------------------------------------------------------------------ the command line (EVAL/eval/cli.py)
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m gan_variant_research_amd.evaluate", description="Kaggle MiFID evaluator on the MI355X")
    p.add_argument("--config", type=str, default=None, help="Path to YAML config file")
    p.add_argument("--fake", type=str, default=None, help="Path to fake images folder")
    p.add_argument("--real", type=str, default=None, help="Path to real images folder (for folder mode)")
    p.add_argument("--out", type=str, default=None, help="Output JSON report path")
    p.add_argument("--batch", type=int, default=None, help="Batch size (overrides config)")
    p.add_argument("--workers", type=int, default=None, help="Number of workers (overrides config; recorded in the report)")
    p.add_argument("--img-size", type=int, default=None, help="Image size (overrides config)")
    p.add_argument("--device", type=str, default=None, help="Device: cuda or cuda:N")
    p.add_argument("--cosine-eps", type=float, default=None, help="Cosine distance epsilon for MiFID")
    p.add_argument("--no-cache", action="store_true", help="Disable caching of real features")
    p.add_argument("--extractor", type=str, default=None, help="pkg.module:factory; factory(device) returns the callable uint8 (B,3,S,S) -> (B,D)")
    p.add_argument("--real-features", type=str, default=None, help="Real features (.npy, or the cache .npz): skips extraction for that side")
    p.add_argument("--fake-features", type=str, default=None, help="Fake features (.npy, or the cache .npz): skips extraction for that side")
    p.add_argument("--device-decode", action="store_true", help="Decode baseline JPEGs on the device")
    p.add_argument("--device-progressive", action="store_true", help="With --device-decode: decode progressive JPEGs on the device too")
    p.add_argument("--device-png", action="store_true", help="Decode PNGs on the device")
    p.add_argument("--io-threads", type=int, default=8, help="Threads that read and (without the device decoders) decode files")
    return p


def _side(name: str, folder: Optional[str], feature_file: Optional[str], recursive: bool):
    """(paths, base, features or None) of one side: its folder's images, and / or the rows of its feature file."""
    feats = load_features(feature_file) if feature_file else None
    if folder:
        paths = enumerate_images(folder, recursive)
        if feats is not None and len(paths) != len(feats):
            raise ValueError(f"--{name}-features has {len(feats)} rows, --{name} holds {len(paths)} images")
        return paths, Path(folder), feats
    if feats is None:
        raise SystemExit(f"Error: --{name} path (or --{name}-features FILE) is required")
    return [Path(f"{feature_file}#{i}") for i in range(len(feats))], None, feats


def main(argv: Optional[Sequence[str]] = None) -> int:
    parser = build_parser()
    a = parser.parse_args(argv)
    if a.device_progressive and not a.device_decode:
        parser.error("--device-progressive needs --device-decode")
    cfg: Dict = {"name": "default_run", "real": {"mode": "folder"}}
    if a.config:
        import yaml
        with open(a.config) as f:
            cfg = yaml.safe_load(f) or {}
        cfg.setdefault("real", {})
    io, metric, cache, rep = (cfg.setdefault(k, {}) or {} for k in ("io", "metric", "cache", "report"))
    if a.fake:
        cfg["fake"] = {"path": a.fake, "recursive": True}
    if a.real:
        cfg["real"]["path"] = a.real
    batch = a.batch or io.get("batch_size", 64)
    workers = a.workers or io.get("num_workers", 8)
    img_size = a.img_size or metric.get("img_size", 299)
    cosine_eps = a.cosine_eps if a.cosine_eps is not None else metric.get("cosine_eps", 0.1)
    out_json = a.out or rep.get("out_json", "./cache/reports/report.json")
    cache_dir = Path(cache.get("dir", "./cache"))
    real_mode = cfg["real"].get("mode", "folder")
    if real_mode == "tfds":
        raise SystemExit("Error: TFDS mode is not implemented in this CLI (the reference's refuses it too)")
    device = dataio.normalize_device(a.device or "cuda")

    fake_dir = (cfg.get("fake") or {}).get("path")
    real_dir = cfg["real"].get("path")
    fake_paths, fake_base, fake_feats = _side("fake", fake_dir, a.fake_features, (cfg.get("fake") or {}).get("recursive", True))
    real_paths, real_base, real_feats = _side("real", real_dir, a.real_features, cfg["real"].get("recursive", True))
    hash_of = lambda paths, base, file: compute_image_list_hash(paths, base) if base is not None else compute_image_list_hash([Path(file)])
    fake_hash, real_hash = hash_of(fake_paths, fake_base, a.fake_features), hash_of(real_paths, real_base, a.real_features)
    if fake_base is not None and real_base is not None:
        validation = validate_image_counts(fake_paths, real_paths)
    else:
        validation = {"num_fake": len(fake_paths), "num_real": len(real_paths), "warnings": []}
    for w in validation["warnings"]:
        print(f"WARNING: {w}")
    overlap = check_dataset_overlap(fake_paths, real_paths)
    if overlap["has_overlap"]:
        print(f"WARNING: Found {overlap['overlap_count']} overlapping filenames! Examples: {overlap['overlap_examples'][:5]}")
    print(f"Fake dataset hash: {fake_hash}\nReal dataset hash: {real_hash}")

    extractor = None
    kw = dict(device=device, batch=batch, img_size=img_size, io_threads=a.io_threads, device_decode=a.device_decode, device_png=a.device_png,
              **(dict(device_progressive=True) if a.device_progressive else {}))
    real_cache = cache_dir / "real_feats"
    if real_feats is None and not a.no_cache:
        cached = load_cached_stats(real_hash, real_cache)
        if cached is not None and "features" in cached and len(cached["features"]) == len(real_paths):
            print(f"Loaded cached real features {real_hash[:8]} (n={cached['n']})")
            real_feats = cached["features"]
    if real_feats is None:
        extractor = load_extractor(a.extractor, device)
        real_feats = extract_features(real_paths, extractor, **kw)
        if not a.no_cache:
            mu, sigma = feature_statistics(real_feats, device)
            save_cached_stats(real_hash, real_cache, mu, sigma, real_feats.cpu().numpy(), len(real_paths))
    if fake_feats is None:
        extractor = extractor or load_extractor(a.extractor, device)
        fake_feats = extract_features(fake_paths, extractor, **kw)

    scores = full_evaluation(real_feats, fake_feats, fake_paths, real_paths, cosine_eps, device=device)
    run_config = {"name": cfg.get("name", "unnamed_run"), "fake_dir": fake_dir or a.fake_features, "real_mode": real_mode,
                  "real_dir": real_dir or a.real_features, "img_size": img_size, "batch_size": batch, "num_workers": workers}
    hashes = {"fake_list_sha1": fake_hash, "real_list_sha1": real_hash, "real_cache_key": f"monet_jpg@sha1:{real_hash[:16]}"}
    report = create_report(scores, run_config, hashes, validation, scores["worst_memorization_cases"])
    save_report(report, out_json)
    save_worst_cases_csv(scores["worst_memorization_cases"], Path(out_json).parent / f"{Path(out_json).stem}_worst_cases.csv")
    print(f"MiFID: {scores['mifid']:.4f}   FID: {scores['fid']:.4f}   median min cosine distance: {scores['cosine_min_distance']['median']:.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
