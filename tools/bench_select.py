"""Times the three float64 parts of the selection step (gan_variant_research_amd.select_7k) three ways, on seeded non-negative features:

    python tools/bench_select.py [--rounds 5] [--size 300x35000x2048] [--k 128] [--out FILE]

  host     the reference's arithmetic (EVAL/scripts/select_7k.py) in numpy on the CPU, in the float32 of its features: the cosine
           floor as one product; the standardisation and the nearest-centre score ((F - centers[:, None, :])**2).sum(-1).min(0), 256
           candidates at a time so that the k x N x D array fits in memory; scikit-learn's KMeans where it imports (else the numpy
           statement of tests/select_ref64.py)
  torch64  the same quantities with torch float64 on the device: the standardised copy, rocBLAS's DGEMM, the N x n_real and N x k
           matrices and their row minima; k-means as the same Lloyd loop in torch (matmul, argmin, index_add_) after the host seeding
  hip      this project's kernels: cos_rowmin, sqdist_rowmin with the transform fused into the operand load, and kmeans_fit
           (sqdist_rowmin + kmeans_update per iteration, seeding on the host)

One process; the modes run in rotation after a warm-up, `rounds` times; per mode and part one JSON line with the median and
[min .. max] of the rounds in milliseconds (wall time, device work synchronised) and the peak memory the part allocated on top of its
resident inputs (host: tracemalloc; device: the caching allocator's peak).  Size is n_real x n_candidates x D.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time
import tracemalloc

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_variant_research_amd import evaluate as E, select_7k as S  # noqa: E402
from gan_variant_research_amd.runtime import HipOps  # noqa: E402

DEV = torch.device("cuda:0")


def features(nr, nc, D):
    g = np.random.default_rng(nr + nc + D)
    base = g.standard_normal(D)
    mk = lambda n, s: np.maximum(g.standard_normal((n, D), dtype=np.float32) * 0.8 + (0.3 * base + s).astype(np.float32), 0)
    return mk(nr, 0.0), mk(nc, 0.15)


def host_run(fn):
    tracemalloc.start()
    t0 = time.perf_counter()
    out = fn()
    ms = (time.perf_counter() - t0) * 1e3
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    return ms, peak, out


def dev_run(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, torch.cuda.max_memory_allocated() - base, out


def torch_kmeans(X, Xh, k, n_init=10, seed=0, max_iter=300, tol=1e-4):
    """The Lloyd loop of select_7k.kmeans_fit with torch float64 in place of the kernels; X on the device, already transformed."""
    x2 = np.einsum("ij,ij->i", Xh, Xh)
    tol_abs = float(np.mean(np.var(Xh, axis=0)) * tol)
    rs = np.random.RandomState(seed)
    xn = (X * X).sum(1)
    best = None
    for _ in range(n_init):
        C = torch.from_numpy(S._seed_plusplus(Xh, x2, k, rs)).to(X.device)
        old, strict = None, False
        for it in range(1, max_iter + 1):
            lab = (xn[:, None] + (C * C).sum(1)[None, :] - 2.0 * (X @ C.t())).clamp_min(0).argmin(1)
            sums = torch.zeros_like(C).index_add_(0, lab, X)
            cnt = torch.bincount(lab, minlength=k).to(torch.float64)
            new = sums / cnt[:, None]                      # the benchmark's fixtures leave no cluster empty
            shift = float(((new - C) ** 2).sum())
            C = new
            if old is not None and bool(torch.equal(lab, old)):
                strict = True
                break
            if shift <= tol_abs:
                break
            old = lab
        if not strict:
            lab = (xn[:, None] + (C * C).sum(1)[None, :] - 2.0 * (X @ C.t())).clamp_min(0).argmin(1)
        inertia = float(((X - C[lab]) ** 2).sum())
        if best is None or inertia < best[1]:
            best = (lab, inertia, C)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", default="300x35000x2048")
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    nr, nc, D = (int(v) for v in args.size.split("x"))
    k = args.k
    ops = HipOps(DEV)
    real, cand = features(nr, nc, D)
    tr, tf = torch.from_numpy(real).to(DEV), torch.from_numpy(cand).to(DEV)
    R, F = E.Features(tr, ops=ops), E.Features(tf, ops=ops)
    mean_f, scale_f = S._standardiser(F)
    mean_r, scale_r = S._standardiser(R)
    km = S.kmeans_fit(R, k, scale=scale_r)
    centers64 = km["centers"]
    centers_dev = torch.from_numpy(centers64).to(DEV)
    centers32 = centers64.astype(np.float32)
    try:
        from sklearn.cluster import KMeans
        host_kmeans_name = "scikit-learn"
    except Exception:
        KMeans, host_kmeans_name = None, "numpy statement"
        from tests import select_ref64

    def host_cos():
        Ff = cand / (np.linalg.norm(cand, axis=1, keepdims=True) + 1e-8)
        Fr = real / (np.linalg.norm(real, axis=1, keepdims=True) + 1e-8)
        return 1.0 - (Ff @ Fr.T).max(axis=1)

    def host_score(chunk=256):
        Fs = (cand - cand.mean(0, keepdims=True)) / (cand.std(0, keepdims=True) + 1e-8)
        out = np.empty(len(Fs), dtype=Fs.dtype)
        for i in range(0, len(Fs), chunk):
            out[i:i + chunk] = ((Fs[i:i + chunk] - centers32[:, None, :]) ** 2).sum(-1).min(0)
        return out

    def host_km():
        Rs = (real - real.mean(0)) / (real.std(0) + 1e-8)
        if KMeans is not None:
            return KMeans(n_clusters=k, n_init=10, random_state=0).fit(Rs).inertia_
        return select_ref64.kmeans(Rs, k)["inertia"]

    def t64_cos():
        a, b = tf.double(), tr.double()
        a = a / (a.norm(dim=1, keepdim=True) + 1e-8)
        b = b / (b.norm(dim=1, keepdim=True) + 1e-8)
        return (1.0 - a @ b.t()).min(dim=1)

    def t64_score():
        a = tf.double()
        a = (a - a.mean(0, keepdim=True)) / (a.std(0, unbiased=False, keepdim=True) + 1e-8)
        d = (a * a).sum(1)[:, None] + (centers_dev * centers_dev).sum(1)[None, :] - 2.0 * (a @ centers_dev.t())
        return d.clamp_min(0).min(dim=1)

    def t64_km():
        a = tr.double()
        a = (a - a.mean(0, keepdim=True)) * scale_r[None, :]
        return torch_kmeans(a, a.cpu().numpy(), k)[1]

    modes = {
        "host": {"cosine": lambda: host_run(host_cos), "score": lambda: host_run(host_score), "kmeans": lambda: host_run(host_km)},
        "torch64": {"cosine": lambda: dev_run(t64_cos), "score": lambda: dev_run(t64_score), "kmeans": lambda: dev_run(t64_km)},
        "hip": {"cosine": lambda: dev_run(lambda: ops.cos_rowmin(tf, tr, ra=1.0 / (F.m["norm"] + 1e-8), rb=1.0 / (R.m["norm"] + 1e-8))),
                "score": lambda: dev_run(lambda: ops.sqdist_rowmin(tf, centers_dev, ca=mean_f, sa=scale_f)),
                "kmeans": lambda: dev_run(lambda: S.kmeans_fit(R, k, scale=scale_r)["inertia"])},
    }
    for m in ("torch64", "hip"):                          # warm-up: library handles, allocator, code objects
        for part in modes[m].values():
            part()
    times = {m: {p: [] for p in parts} for m, parts in modes.items()}
    peaks = {m: {p: 0 for p in parts} for m, parts in modes.items()}
    last = {m: {} for m in modes}
    for _ in range(args.rounds):
        for m, parts in modes.items():
            for p, run in parts.items():
                ms, peak, out = run()
                times[m][p].append(ms)
                peaks[m][p] = max(peaks[m][p], int(peak))
                last[m][p] = out
    for m, parts in times.items():
        for p, t in parts.items():
            say({"size": args.size, "k": k, "mode": m, "part": p, "median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3),
                 "max_ms": round(max(t), 3), "peak_bytes": peaks[m][p], "memory": "host" if m == "host" else "device", "rounds": args.rounds})
    d_hip, i_hip = last["hip"]["score"]
    t = last["torch64"]["score"]
    c_hip, c_t = last["hip"]["cosine"][0], last["torch64"]["cosine"].values
    say({"size": args.size, "check": {
        "score_max_abs_diff_vs_torch64": float((d_hip - t.values).abs().max()), "score_index_mismatches": int((i_hip.long() != t.indices).sum()),
        "score_max_rel_diff_host_float32_vs_hip": float(np.abs(last["host"]["score"].astype(np.float64) - d_hip.cpu().numpy()).max() / d_hip.max().item()),
        "cosine_max_abs_diff_vs_torch64": float((c_hip - c_t).abs().max()),
        "kmeans_inertia": {"host": float(last["host"]["kmeans"]), "torch64": float(last["torch64"]["kmeans"]), "hip": float(last["hip"]["kmeans"])},
        "host_kmeans": host_kmeans_name + " on the float32 standardised matrix", "kmeans_n_iter_hip": km["n_iter"]}})
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
