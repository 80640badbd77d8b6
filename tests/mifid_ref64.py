"""TEST INFRASTRUCTURE: an independent numpy statement of every quantity of csrc/mifid.hip and gan_variant_research_amd.evaluate.

Products and sums that a kernel result is held to run in numpy's long double (a 64-bit mantissa on x86), so that the reference's own
rounding is far below the float64 bounds the tests derive; the linear algebra of the end-to-end quantities is float64 LAPACK on
factors of the two covariances (from the SVD of each centred set), not on the cross-Gram matrix the product computes.  Never imported by the product
package."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


# ---- kernels
def moments(X):
    """mean [D], colcss [D], norm [n], rowsum [n], css, and the magnitudes the bounds use."""
    x = ld(X)
    n = x.shape[0]
    mean = x.sum(0) / n
    c = x - mean
    colcss = (c * c).sum(0)
    return {"mean": mean, "colcss": colcss, "norm": np.sqrt((x * x).sum(1)), "rowsum": x.sum(1), "css": colcss.sum(),
            "abs_colsum": np.abs(x).sum(0), "abs_rowsum": np.abs(x).sum(1)}


def operands(A, B, trans, ca=None, cb=None):
    """The centred operands as (M, K) and (N, K) long doubles."""
    a, b = ld(A), ld(B)
    if trans:
        a, b = a.T, b.T
        if ca is not None:
            a = a - ld(ca)[:, None]
        if cb is not None:
            b = b - ld(cb)[:, None]
    else:
        if ca is not None:
            a = a - ld(ca)[None, :]
        if cb is not None:
            b = b - ld(cb)[None, :]
    return a, b


def gram(A, B, trans, ca=None, cb=None, ra=None, rb=None, alpha=1.0):
    """(C, bound): the contraction and (K + 8) 2^-53 |alpha| ra rb sum_k |a - ca| |b - cb| per element."""
    a, b = operands(A, B, trans, ca, cb)
    K = a.shape[1]
    sa = np.ones(a.shape[0], LD) if ra is None else ld(ra)
    sb = np.ones(b.shape[0], LD) if rb is None else ld(rb)
    scale = abs(LD(alpha)) * np.abs(sa)[:, None] * np.abs(sb)[None, :]
    C = LD(alpha) * sa[:, None] * sb[None, :] * (a @ b.T)
    bound = (K + 8) * U * scale * (np.abs(a) @ np.abs(b).T)
    return C, bound


def rowmin(A, B, ca=None, cb=None, ra=None, rb=None, alpha=1.0, absolute=False):
    """(d matrix with +inf where a row or a column is left out, bound matrix); d = 1 - s or 1 - |s|.  The bound adds 2 u for the
    subtraction from 1 (|d| <= 2)."""
    s, bound = gram(A, B, 0, ca, cb, ra, rb, alpha)
    d = 1 - (np.abs(s) if absolute else s)
    if ra is not None:
        d[np.asarray(ra) == 0, :] = np.inf
    if rb is not None:
        d[:, np.asarray(rb) == 0] = np.inf
    return d, bound + 2 * U


# ---- the metric, textbook form in float64
def statistics(X, ddof=1):
    X = np.asarray(X, np.float64)
    return X.mean(0), np.cov(X, rowvar=False, ddof=ddof).reshape(X.shape[1], X.shape[1])


def _factor(X, ddof=1):
    """L (D x rank) with L L^T = cov(X): from the singular value decomposition of the centred rows, whose small singular values carry
    noise of order u s_max -- the eigenvalues of a singular covariance carry u l_max, and their square roots sqrt(u) times as much."""
    X = np.asarray(X, np.float64)
    _, s, Vt = np.linalg.svd(X - X.mean(0), full_matrices=False)
    return Vt.T * (s / np.sqrt(len(X) - ddof))


def frechet_terms(real, fake, ddof=1):
    """dmu2, tr_r, tr_f and c = tr sqrt(Sr Sf) as the sum of the singular values of Lr^T Lf, S = L L^T."""
    mr, Sr = statistics(real, ddof)
    mf, Sf = statistics(fake, ddof)
    c = np.linalg.svd(_factor(real, ddof).T @ _factor(fake, ddof), compute_uv=False).sum()
    return {"dmu2": float(((mr - mf) ** 2).sum()), "tr_r": float(np.trace(Sr)), "tr_f": float(np.trace(Sf)), "c": float(c)}


def frechet_c_cov(real, fake):
    """c through eigh of the two covariances with negative eigenvalues clipped: the other float64 statement, less exact when a set has
    fewer rows than columns."""
    fac = []
    for X in (real, fake):
        lam, V = np.linalg.eigh(statistics(X)[1])
        fac.append(V * np.sqrt(np.clip(lam, 0, None)))
    return float(np.linalg.svd(fac[0].T @ fac[1], compute_uv=False).sum())


def frechet_c_gram(real, fake):
    """The same c from the centred cross-Gram matrix (the identity of evaluate.py), in float64 numpy."""
    r, f = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    M = (r - r.mean(0)) @ (f - f.mean(0)).T / np.sqrt((len(r) - 1.0) * (len(f) - 1.0))
    return float(np.linalg.svd(M, compute_uv=False).sum())


def frechet_distance(real, fake, ddof=1):
    t = frechet_terms(real, fake, ddof)
    return t["dmu2"] + t["tr_r"] + t["tr_f"] - 2 * t["c"]


def scale_of(real, fake):
    """tr Sr + tr Sf + |dmu|^2: what the end-to-end tolerances are relative to."""
    t = frechet_terms(real, fake)
    return t["tr_r"] + t["tr_f"] + t["dmu2"]


def memorization_mean(real, fake, rows="real", absolute=True):
    """The mean of the minimum distances before the threshold: zero-sum rows dropped from both sets, rows / norm, d = 1 - |cos|."""
    r, f = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    r, f = r[r.sum(1) != 0], f[f.sum(1) != 0]
    r, f = r / np.linalg.norm(r, axis=1, keepdims=True), f / np.linalg.norm(f, axis=1, keepdims=True)
    a, b = (r, f) if rows == "real" else (f, r)
    s = a @ b.T
    d = 1 - (np.abs(s) if absolute else s)
    return float(d.min(1).mean())


def memorization_distance(real, fake, cosine_eps=0.1, rows="real", absolute=True):
    m = memorization_mean(real, fake, rows, absolute)
    return m if m < cosine_eps else 1.0


def mifid(real, fake, cosine_eps=0.1):
    fid, dist = frechet_distance(real, fake), memorization_distance(real, fake, cosine_eps)
    return {"fid": fid, "distance": dist, "mifid": fid / (dist + 1e-14) if fid > 1e-8 else 0.0}


def cosine_min(fake, real):
    """Signed minimum distances with the reference's 1e-8 in the norms, in long double (so that the tests' float64 bound is the
    kernel's alone), and the nearest index; returned as float64."""
    f, r = ld(fake), ld(real)
    f = f / (np.sqrt((f * f).sum(1, keepdims=True)) + LD(1e-8))
    r = r / (np.sqrt((r * r).sum(1, keepdims=True)) + LD(1e-8))
    d = 1 - f @ r.T
    return d.min(1).astype(np.float64), d.argmin(1), d.astype(np.float64)
