"""Selection: the reference's EVAL/scripts/select_7k.py, which chooses the 7000 generated images of the submission out of several
candidate folders.

    python -m gan_variant_research_amd.select_7k --real R --cand_roots A B --outdir OUT --extractor pkg.module:factory

The reference's script cannot run as it stands (it imports a function its package does not define, and its nearest-centre score
materialises a k x N x D array); its arithmetic is restated here step for step, in float64, on the kernels of csrc/mifid.hip:

  * the cosine floor is `evaluate.cosine_min_distances` (`HipOps.cos_rowmin`);
  * the standardisation (x - mean) / (std + 1e-8) is never applied to a stored matrix: mean and 1 / (std + 1e-8) go to the kernels as
    the column transform (x - c[k]) * s[k] of their operand load;
  * the nearest-centre score is one `HipOps.sqdist_rowmin` call, which never writes the N x k matrix;
  * k-means states scikit-learn's `KMeans(n_clusters=k, n_init=10, random_state=0)` (Lloyd, k-means++): assignment on
    `sqdist_rowmin`, update on `HipOps.kmeans_update`, seeding and the rare empty-cluster relocation on the host in numpy float64 --
    the same kind of boundary as LAPACK in evaluate.py.  scikit-learn is not imported; it is the yardstick of the tests, run on the
    float64 standardised matrix.  Parity with scikit-learn's run on a float32 matrix (what the reference's script would feed it) is
    not a target: on float32 input scikit-learn itself can choose another clustering than on the float64 one.

There is no fallback: without the library every function here raises.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import shutil
import sys
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dataio
from . import evaluate as E
from .evaluate import Features


def min_cos_dists(F_fake, F_real, device=None, ops=None) -> np.ndarray:
    """select_7k.py:14-20: for every fake row, 1 - the largest cosine similarity to a real row (norms + 1e-8)."""
    return E.cosine_min_distances(F_fake, F_real, device, ops)[0]


def _standardiser(f: Features) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean, 1 / (std + 1e-8)) of the columns, std the population one (numpy's F.std(0)): sqrt(colcss / n) from the moments launch."""
    return f.m["mean"], 1.0 / (torch.sqrt(f.m["colcss"] / f.n) + 1e-8)


# ------------------------------------------------------------------------------------------------ k-means
def _sqdist_expanded(Y: np.ndarray, X: np.ndarray, x2: np.ndarray) -> np.ndarray:
    """|y|^2 + |x|^2 - 2 y.x for every pair, clipped at 0: the expanded form scikit-learn's seeding uses."""
    d = -2.0 * (Y @ X.T)
    d += np.einsum("ij,ij->i", Y, Y)[:, None]
    d += x2[None, :]
    np.maximum(d, 0.0, out=d)
    return d


def _seed_plusplus(X: np.ndarray, x2: np.ndarray, k: int, rs: np.random.RandomState) -> np.ndarray:
    """k-means++ as scikit-learn draws it: the first centre from `choice`, every later one the best of 2 + int(log k) candidates drawn
    in proportion to the squared distance to the nearest centre so far."""
    n = X.shape[0]
    w = np.ones(n)
    trials = 2 + int(np.log(k))
    first = rs.choice(n, p=w / w.sum())
    centers = np.empty((k, X.shape[1]))
    centers[0] = X[first]
    closest = _sqdist_expanded(centers[0:1], X, x2)
    pot = closest @ w
    for c in range(1, k):
        draws = rs.uniform(size=trials) * pot
        cand = np.searchsorted(np.cumsum(w * closest.ravel()), draws)
        np.clip(cand, None, n - 1, out=cand)
        d = _sqdist_expanded(X[cand], X, x2)
        np.minimum(closest, d, out=d)
        pots = d @ w.reshape(-1, 1)
        best = int(np.argmin(pots))
        pot, closest = pots[best], d[best:best + 1]
        centers[c] = X[cand[best]]
    return centers


def _same_clustering(a: np.ndarray, b: np.ndarray, k: int) -> bool:
    """Two labellings that differ only by the names of the clusters."""
    to = np.full(k, -1, dtype=np.int64)
    for i, j in zip(a.tolist(), b.tolist()):
        if to[i] == -1:
            to[i] = j
        elif to[i] != j:
            return False
    return True


def _lloyd(f: Features, c, s, Xh: np.ndarray, centers0: np.ndarray, max_iter: int, tol: float):
    """One run from the seeded centres: (labels, inertia, centres, iterations)."""
    ops, dev = f.ops, f.x.device
    k = centers0.shape[0]
    centers = torch.from_numpy(np.ascontiguousarray(centers0)).to(dev)
    labels_old = None
    strict = False
    it = 0
    for it in range(1, max_iter + 1):
        _, labels = ops.sqdist_rowmin(f.x, centers, ca=c, sa=s)
        sums, counts, err = ops.kmeans_update(f.x, labels, k, c=c, s=s)
        if int(err.cpu()[0]) != 0:
            raise RuntimeError("kmeans_fit: an assignment outside [0, k): a feature or a centre is not finite")
        cnt = counts[:k].cpu().numpy().astype(np.int64)
        if (cnt == 0).any():                                  # rare: the farthest points move to the empty clusters, on the host
            lab = labels.cpu().numpy()
            S, old = sums.cpu().numpy().copy(), centers.cpu().numpy()
            far = ((Xh - old[lab]) ** 2).sum(1)
            empty = np.flatnonzero(cnt == 0)
            takers = np.argsort(-far, kind="stable")[:len(empty)]
            for e, i in zip(empty, takers):
                S[lab[i]] -= Xh[i]
                S[e] = Xh[i]
                cnt[e] = 1
                cnt[lab[i]] -= 1
            sums = torch.from_numpy(S).to(dev)
        new = sums / torch.from_numpy(cnt.astype(np.float64)).to(dev)[:, None]
        shift = float((torch.sqrt(((new - centers) ** 2).sum(1)) ** 2).sum().cpu())
        centers = new
        if labels_old is not None and bool(torch.equal(labels, labels_old)):
            strict = True
            break
        if shift <= tol:
            break
        labels_old = labels
    if not strict:
        _, labels = ops.sqdist_rowmin(f.x, centers, ca=c, sa=s)
    lab = labels.cpu().numpy().astype(np.int64)
    C = centers.cpu().numpy()
    inertia = float(((Xh - C[lab]) ** 2).sum())               # the direct form, not the expanded one
    return lab, inertia, C, it


def kmeans_fit(x, k: int, n_init: int = 10, seed: int = 0, max_iter: int = 300, tol: float = 1e-4, scale=None, device=None, ops=None,
               init=None) -> Dict:
    """scikit-learn's KMeans(n_clusters=k, n_init=n_init, random_state=seed, max_iter=max_iter, tol=tol).fit on the rows
    x' = (x - mean(x)) * scale (scale: None, or a float64 vector per column; the column mean is always subtracted, as KMeans.fit does),
    x' formed in the kernels' operand load.  init: None (k-means++), or k starting centres in the space of x (scikit-learn's
    init=array; one run).  Returns centers (float64 k x D, in the space of x'), labels, inertia, n_iter."""
    f = Features(x, device, ops, "k-means input")
    k = int(k)
    if k < 1 or k > f.n:
        raise ValueError(f"kmeans_fit: k = {k} clusters for {f.n} rows")
    if n_init < 1 or max_iter < 1:
        raise ValueError(f"kmeans_fit: n_init = {n_init}, max_iter = {max_iter}: at least 1 each")
    c = f.m["mean"]
    s = None
    if scale is not None:
        s = (scale if isinstance(scale, torch.Tensor) else torch.from_numpy(np.asarray(scale, dtype=np.float64))).to(f.x.device, torch.float64).contiguous()
        if s.numel() != f.D:
            raise ValueError(f"kmeans_fit: scale has {s.numel()} entries for {f.D} columns")
    Xh = f.x.cpu().numpy().astype(np.float64) - c.cpu().numpy()[None, :]          # the kernels' x', the same two rounded operations
    if s is not None:
        Xh = Xh * s.cpu().numpy()[None, :]
    x2 = np.einsum("ij,ij->i", Xh, Xh)
    tol_abs = float(np.mean(np.var(Xh, axis=0)) * tol)
    rs = np.random.RandomState(seed)
    best = None
    if init is not None:
        init = np.asarray(init, dtype=np.float64)
        if init.shape != (k, f.D):
            raise ValueError(f"kmeans_fit: init of shape {init.shape}, expected {(k, f.D)}")
        init = init - c.cpu().numpy()[None, :]
        if s is not None:
            init = init * s.cpu().numpy()[None, :]
        n_init = 1
    for _ in range(n_init):
        run = _lloyd(f, c, s, Xh, _seed_plusplus(Xh, x2, k, rs) if init is None else init, max_iter, tol_abs)
        if best is None or (run[1] < best[1] and not _same_clustering(run[0], best[0], k)):
            best = run
    return {"centers": best[2], "labels": best[0], "inertia": best[1], "n_iter": best[3], "mean": c.cpu().numpy(),
            "scale": None if s is None else s.cpu().numpy()}


def nearest_center_sqdist(features, centers, mean=None, scale=None, device=None, ops=None) -> Tuple[np.ndarray, np.ndarray]:
    """For every row of `features`, transformed on load as (x - mean) * scale, the squared distance to the nearest row of `centers`
    (taken as they are) and that row's index: one sqdist_rowmin call, no N x k matrix."""
    f = features if isinstance(features, Features) else Features(features, device, ops)
    dev = f.x.device
    vec = lambda v: None if v is None else (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v, dtype=np.float64))).to(dev, torch.float64).contiguous()
    cen = (centers if isinstance(centers, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(centers, dtype=np.float64))).to(dev, torch.float64).contiguous()
    if cen.dim() != 2 or cen.shape[1] != f.D:
        raise ValueError(f"centres of shape {tuple(cen.shape)} for features with D = {f.D}")
    d, idx = f.ops.sqdist_rowmin(f.x, cen, ca=vec(mean), sa=vec(scale))
    return d.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------------ the selection
def select(real, cands, tau: float = 0.22, k: int = 128, target: int = 7000, n_init: int = 10, seed: int = 0, device=None, ops=None,
           verbose: bool = True) -> Dict:
    """select_7k.py:36-59 on feature matrices.  `cands`: one matrix or a sequence of them (stacked in order).  Returns chosen (indices
    into the stacked candidates, best score first), score, dist, min_cos, nearest_real (each per stacked candidate), kept (the mask
    min_cos >= tau) and kmeans ({"inertia", "n_iter", "labels"})."""
    r = Features(real, device, ops, "real features")
    if isinstance(cands, (list, tuple)):
        parts = [c.x if isinstance(c, Features) else (c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(c)))) for c in cands]
        if not parts:
            raise ValueError("select: no candidates")
        dt = torch.float32 if all(p.dtype == torch.float32 for p in parts) else torch.float64
        cands = torch.cat([p.to(r.x.device, dt) for p in parts])
    f = Features(cands, r.x.device, r.ops, "candidate features")
    if f.D != r.D:
        raise ValueError(f"real features have D = {r.D}, candidates D = {f.D}: they must come from one extractor")
    mins, nearest = E.cosine_min_distances(f, r)
    mean_f, scale_f = _standardiser(f)                         # over all stacked candidates, before the filter
    keep = mins >= tau
    _, scale_r = _standardiser(r)
    km = kmeans_fit(r, k, n_init=n_init, seed=seed, scale=scale_r)
    dist, _ = nearest_center_sqdist(f, km["centers"], mean_f, scale_f)
    score = dist - 0.05 * mins
    kept_idx = np.flatnonzero(keep)
    chosen = kept_idx[np.argsort(score[kept_idx], kind="stable")][:target]
    if verbose and len(kept_idx) < target:
        print(f"only {len(kept_idx)} of {f.n} candidates pass tau = {tau}; all of them are selected, fewer than the target {target}")
    return {"chosen": chosen, "score": score, "dist": dist, "min_cos": mins, "nearest_real": nearest, "kept": keep,
            "kmeans": {"inertia": km["inertia"], "n_iter": km["n_iter"], "labels": km["labels"]}}


# ------------------------------------------------------------------------------------------------ the command line
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m gan_variant_research_amd.select_7k", description="Choose the submission's images on the MI355X")
    p.add_argument("--real", type=str, default=None, help="Real images folder")
    p.add_argument("--cand_roots", nargs="+", required=True, help="Candidate folders")
    p.add_argument("--outdir", required=True)
    p.add_argument("--tau", type=float, default=0.22, help="Floor on the minimum cosine distance to the real set")
    p.add_argument("--k", type=int, default=128, help="k-means clusters of the real set")
    p.add_argument("--target", type=int, default=7000)
    p.add_argument("--extractor", type=str, default=None, help="pkg.module:factory; factory(device) returns the callable uint8 (B,3,S,S) -> (B,D)")
    p.add_argument("--real-features", type=str, default=None, help="Real features (.npy, or the cache .npz): skips extraction for that side")
    p.add_argument("--cand-features", nargs="+", default=None, help="Candidate features, one file per root: skips their extraction")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--img-size", type=int, default=299)
    p.add_argument("--io-threads", type=int, default=8)
    p.add_argument("--device-decode", action="store_true", help="Decode baseline JPEGs on the device")
    p.add_argument("--device-progressive", action="store_true", help="With --device-decode: decode progressive JPEGs on the device too")
    p.add_argument("--device-png", action="store_true", help="Decode PNGs on the device")
    p.add_argument("--device", type=str, default=None, help="Device: cuda or cuda:N")
    p.add_argument("--no-copy", action="store_true", help="Write the meta file and the table, copy no image")
    p.add_argument("--zip", default=None, metavar="PATH", help="Write the selected images as stored entries of this archive (what images/ holds), also with --no-copy")
    return p


def main(argv: Optional[Sequence[str]] = None) -> int:
    parser = build_parser()
    a = parser.parse_args(argv)
    if a.device_progressive and not a.device_decode:
        parser.error("--device-progressive needs --device-decode")
    device = dataio.normalize_device(a.device or "cuda")
    if a.cand_features is not None and len(a.cand_features) != len(a.cand_roots):
        raise SystemExit(f"Error: {len(a.cand_features)} --cand-features files for {len(a.cand_roots)} --cand_roots")
    if not a.real and not a.real_features:
        raise SystemExit("Error: --real path (or --real-features FILE) is required")
    os.makedirs(a.outdir, exist_ok=True)
    kw = dict(device=device, batch=a.batch, img_size=a.img_size, io_threads=a.io_threads, device_decode=a.device_decode, device_png=a.device_png,
              **(dict(device_progressive=True) if a.device_progressive else {}))
    extractor = None

    def side(folder, feature_file, what):
        nonlocal extractor
        paths = E.enumerate_images(folder) if folder else None
        if feature_file:
            feats = E.load_features(feature_file)
            if paths is not None and len(paths) != len(feats):
                raise ValueError(f"{feature_file} has {len(feats)} rows, {folder} holds {len(paths)} images")
            if paths is None:
                paths = [Path(f"{feature_file}#{i}") for i in range(len(feats))]
            return feats, paths
        if not paths:
            raise ValueError(f"{what}: no images in {folder}")
        extractor = extractor or E.load_extractor(a.extractor, device)
        return E.extract_features(paths, extractor, **kw), paths

    real_feats, real_paths = side(a.real, a.real_features, "--real")
    cand_feats, cand_paths = [], []
    for i, root in enumerate(a.cand_roots):
        F, P = side(root, a.cand_features[i] if a.cand_features else None, "--cand_roots")
        cand_feats.append(F)
        cand_paths += P
    res = select(real_feats, cand_feats, tau=a.tau, k=a.k, target=a.target, device=device)
    sel_paths = [cand_paths[i] for i in res["chosen"]]

    outimgs = Path(a.outdir) / "images"
    names = [Path(p).name for p in sel_paths]
    collisions = len(names) - len(set(names))
    if not a.no_copy:
        outimgs.mkdir(parents=True, exist_ok=True)
        for p in sel_paths:
            shutil.copy2(p, outimgs / Path(p).name)               # as in the reference, a later file of the same name overwrites
    zipped = None
    if a.zip:
        from .inference import ZipWriter
        last = {Path(p).name: p for p in sel_paths}              # what images/ holds after the copy: the last file of a name
        with ZipWriter(a.zip) as zw:
            for name in sorted(last):
                zw.add(name, Path(last[name]).read_bytes())      # bytes from disk: the checksum is the host's
            zipped = len(zw)
    if collisions:
        print(f"{collisions} selected images share a file name with an earlier one; images/ holds {len(set(names))} files")
    with open(Path(a.outdir) / "selection_meta.json", "w") as f:
        json.dump({"real": a.real, "cand_roots": a.cand_roots, "tau": a.tau, "k": a.k, "selected": len(sel_paths),
                   "candidates": len(cand_paths), "kept": int(res["kept"].sum()), "collisions": collisions,
                   "kmeans_inertia": res["kmeans"]["inertia"], "kmeans_n_iter": res["kmeans"]["n_iter"],
                   **({"zip": a.zip, "zip_entries": zipped} if a.zip else {})}, f, indent=2)
    with open(Path(a.outdir) / "selection.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["path", "score", "dist", "min_cos", "nearest_real_path", "rank"])
        for rank, i in enumerate(res["chosen"], 1):
            w.writerow([str(cand_paths[i]), repr(float(res["score"][i])), repr(float(res["dist"][i])), repr(float(res["min_cos"][i])),
                        str(real_paths[int(res["nearest_real"][i])]), rank])
    print(f"Selected {len(sel_paths)} images into {outimgs if not a.no_copy or not a.zip else a.zip}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
