"""TEST INFRASTRUCTURE: the float64 statement of the selection step (the reference's EVAL/scripts/select_7k.py) in numpy, with the
direct-form distance sum (a' - b')^2 wherever the kernels use the expanded one: the transformed rows, the squared-distance row
minimum and its bound, the k-means update and its bound, a numpy k-means that states scikit-learn's KMeans (Lloyd, k-means++), and
the selection itself.  Never imported by the product package."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53


def xform(x, c=None, s=None):
    X = np.asarray(x, dtype=np.float64)
    if c is not None:
        X = X - np.asarray(c)[None, :]
    if s is not None:
        X = X * np.asarray(s)[None, :]
    return X


def sqdist(a, b, ca=None, sa=None, cb=None, sb=None):
    """(d, bound): d_ij = sum_k (a'_ik - b'_jk)^2 in long double, and the kernels' bound 4 (K + 8) u (na_i + nb_j)."""
    A, B = xform(a, ca, sa).astype(np.longdouble), xform(b, cb, sb).astype(np.longdouble)
    d = np.empty((A.shape[0], B.shape[0]), dtype=np.longdouble)
    for j in range(B.shape[0]):
        e = A - B[j][None, :]
        d[:, j] = (e * e).sum(1)
    na, nb = (A * A).sum(1), (B * B).sum(1)
    return d, 4.0 * (A.shape[1] + 8) * U * (na[:, None] + nb[None, :])


def kmeans_update(x, labels, k, c=None, s=None):
    """(sums, counts, bad, bound): long-double per-cluster sums of x', the counts, whether a label is outside [0, k), and the bound
    (n_c + 2) u sum |x'| per entry."""
    X = xform(x, c, s).astype(np.longdouble)
    labels = np.asarray(labels)
    sums = np.zeros((k, X.shape[1]), dtype=np.longdouble)
    mag = np.zeros((k, X.shape[1]), dtype=np.longdouble)
    counts = np.zeros(k, dtype=np.int64)
    bad = False
    for i, l in enumerate(labels.tolist()):
        if 0 <= l < k:
            sums[l] += X[i]
            mag[l] += np.abs(X[i])
            counts[l] += 1
        else:
            bad = True
    return sums, counts, bad, (counts[:, None] + 2) * U * mag


# ------------------------------------------------------------------------------------------------ k-means (scikit-learn's, restated)
def _expanded(Y, X, x2):
    d = -2.0 * (Y @ X.T)
    d += np.einsum("ij,ij->i", Y, Y)[:, None]
    d += x2[None, :]
    np.maximum(d, 0.0, out=d)
    return d


def _plusplus(X, x2, k, rs):
    n = X.shape[0]
    w = np.ones(n)
    trials = 2 + int(np.log(k))
    first = rs.choice(n, p=w / w.sum())
    centers = np.empty((k, X.shape[1]))
    centers[0] = X[first]
    closest = _expanded(centers[0:1], X, x2)
    pot = closest @ w
    for c in range(1, k):
        cand = np.searchsorted(np.cumsum(w * closest.ravel()), rs.uniform(size=trials) * pot)
        np.clip(cand, None, n - 1, out=cand)
        d = _expanded(X[cand], X, x2)
        np.minimum(closest, d, out=d)
        pots = d @ w.reshape(-1, 1)
        b = int(np.argmin(pots))
        pot, closest = pots[b], d[b:b + 1]
        centers[c] = X[cand[b]]
    return centers


def _direct(X, C):
    d = np.empty((X.shape[0], C.shape[0]))
    for j in range(C.shape[0]):
        e = X - C[j][None, :]
        d[:, j] = (e * e).sum(1)
    return d


def _same(a, b, k):
    to = {}
    return all(to.setdefault(i, j) == j for i, j in zip(a.tolist(), b.tolist()))


def _lloyd(X, C, max_iter, tol):
    k = C.shape[0]
    old = None
    strict = False
    for it in range(1, max_iter + 1):
        lab = np.argmin(_direct(X, C), axis=1)                       # np.argmin: the lowest index of a tie
        S = np.zeros_like(C)
        np.add.at(S, lab, X)
        cnt = np.bincount(lab, minlength=k).astype(np.int64)
        empty = np.flatnonzero(cnt == 0)
        if len(empty):
            far = ((X - C[lab]) ** 2).sum(1)
            for e, i in zip(empty, np.argsort(-far, kind="stable")[:len(empty)]):
                S[lab[i]] -= X[i]
                S[e] = X[i]
                cnt[e] = 1
                cnt[lab[i]] -= 1
        new = S / cnt[:, None]
        shift = ((new - C) ** 2).sum()
        C = new
        if old is not None and np.array_equal(lab, old):
            strict = True
            break
        if shift <= tol:
            break
        old = lab
    if not strict:
        lab = np.argmin(_direct(X, C), axis=1)
    return lab, float(((X - C[lab]) ** 2).sum()), C, it


def kmeans(x, k, n_init=10, seed=0, max_iter=300, tol=1e-4, scale=None, init=None):
    """KMeans(n_clusters=k, n_init=n_init, random_state=seed).fit on (x - mean(x)) * scale: centers (in that space), labels, inertia, n_iter."""
    X = np.asarray(x, dtype=np.float64)
    mean = X.mean(axis=0)
    X = xform(X, mean, scale)
    x2 = np.einsum("ij,ij->i", X, X)
    tol_abs = np.mean(np.var(X, axis=0)) * tol
    rs = np.random.RandomState(seed)
    best = None
    if init is not None:
        init, n_init = xform(init, mean, scale), 1
    for _ in range(n_init):
        run = _lloyd(X, _plusplus(X, x2, k, rs) if init is None else init, max_iter, tol_abs)
        if best is None or (run[1] < best[1] and not _same(run[0], best[0], k)):
            best = run
    return {"centers": best[2], "labels": best[0], "inertia": best[1], "n_iter": best[3], "mean": mean}


# ------------------------------------------------------------------------------------------------ the selection
def select(real, cands, tau=0.22, k=128, target=7000, n_init=10, seed=0):
    R = np.asarray(real, dtype=np.float64)
    F = np.vstack([np.asarray(c, dtype=np.float64) for c in cands]) if isinstance(cands, (list, tuple)) else np.asarray(cands, dtype=np.float64)
    Ff = F / (np.linalg.norm(F, axis=1, keepdims=True) + 1e-8)
    Fr = R / (np.linalg.norm(R, axis=1, keepdims=True) + 1e-8)
    sims = Ff @ Fr.T
    mins = 1.0 - sims.max(axis=1)
    nearest = sims.argmax(axis=1)
    Fs = xform(F, F.mean(0), 1.0 / (F.std(0) + 1e-8))
    keep = mins >= tau
    km = kmeans(R, k, n_init=n_init, seed=seed, scale=1.0 / (R.std(0) + 1e-8))
    dist = _direct(Fs, km["centers"]).min(1)
    score = dist - 0.05 * mins
    idx = np.flatnonzero(keep)
    chosen = idx[np.argsort(score[idx], kind="stable")][:target]
    return {"chosen": chosen, "score": score, "dist": dist, "min_cos": mins, "nearest_real": nearest, "kept": keep, "kmeans": km}
