"""TEST INFRASTRUCTURE: emulator statement of the evaluation entries of csrc/mifid.hip (HipOps.feat_moments, gram_f64,
cos_rowmin_bounds, cos_rowmin) in float64 torch on the CPU, so that gan_variant_research_amd.evaluate runs without a GPU.  The same
argument checks, the same extents written (nothing past an output's logical window), the same conventions for left-out rows and
columns.  Never imported by the product package."""
from __future__ import annotations

import torch

from gan_variant_research_amd._lib import GanError

TM = 64


def _feat(x):
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype in (torch.float32, torch.float64) and (x.shape[1] == 1 or x.stride(1) == 1)):
        raise GanError("feature matrix: 2-D fp32/fp64 with unit column stride")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise GanError("extents must be positive")
    return x.double()


def _vec(t, n):
    if t is None:
        return None
    assert t.dtype == torch.float64 and t.is_contiguous() and t.numel() == n
    return t


class MifidEmuOps:
    is_hip = False

    def feat_moments(self, x, out=None):
        X = _feat(x)
        n = X.shape[0]
        mean = X.sum(0) / n
        c = X - mean
        colcss = (c * c).sum(0)
        r = {"mean": mean, "colcss": colcss, "norm": (X * X).sum(1).sqrt(), "rowsum": X.sum(1), "css": colcss.sum().reshape(1),
             "flag": torch.tensor([0 if bool(torch.isfinite(X).all()) else 1], dtype=torch.int32)}
        if out is None:
            return r
        for k, v in r.items():
            assert out[k].dtype == v.dtype and out[k].is_contiguous() and out[k].numel() >= v.numel(), k
            out[k].reshape(-1)[:v.numel()] = v
        return {k: out[k].reshape(-1)[:v.numel()] for k, v in r.items()}

    def _product(self, a, b, trans, ca, cb, ra, rb, alpha):
        A, B = _feat(a), _feat(b)
        if trans not in (0, 1):
            raise GanError(f"trans must be 0 or 1 (got {trans})")
        if trans:
            if ra is not None or rb is not None:
                raise GanError("row scales belong to trans = 0")
            A, B = A.t(), B.t()
        M, N, K = A.shape[0], B.shape[0], A.shape[1]
        if B.shape[1] != K:
            raise GanError("contraction lengths differ")
        ca, cb = _vec(ca, M if trans else K), _vec(cb, N if trans else K)
        ra, rb = _vec(ra, M), _vec(rb, N)
        if ca is not None:
            A = A - (ca[:, None] if trans else ca[None, :])
        if cb is not None:
            B = B - (cb[:, None] if trans else cb[None, :])
        if ra is not None:
            A = A * ra[:, None]
        if rb is not None:
            B = B * rb[:, None]
        return alpha * (A @ B.t()), (M, N, K)

    def gram_f64(self, a, b, trans=0, ca=None, cb=None, ra=None, rb=None, alpha=1.0, out=None):
        C, (M, N, K) = self._product(a, b, int(trans), ca, cb, ra, rb, float(alpha))
        if out is None:
            return C.contiguous()
        assert out.dtype == torch.float64 and tuple(out.shape) == (M, N) and (N == 1 or out.stride(1) == 1)
        out.copy_(C)
        return out

    def cos_rowmin_bounds(self, M, N):
        if M <= 0 or N <= 0:
            raise GanError(f"cos_rowmin_bounds: extents must be positive (M={M} N={N})")
        nt = -(-N // TM)
        return -(-(nt * M * 8) // 16) * 16 + nt * M * 4

    def cos_rowmin(self, a, b, ca=None, cb=None, ra=None, rb=None, alpha=1.0, absolute=False, ws=None, dmin=None, imin=None):
        S, (M, N, K) = self._product(a, b, 0, ca, cb, ra, rb, float(alpha))
        if ws is not None and ws.numel() < self.cos_rowmin_bounds(M, N):
            raise GanError("cos_rowmin: workspace below gan_cos_rowmin_bounds")
        d = 1.0 - (S.abs() if absolute else S)
        inf = float("inf")
        if rb is not None:
            d[:, rb == 0] = inf
        if ra is not None:
            d[ra == 0, :] = inf
        best = d.min(1).values
        first = (d == best[:, None]).to(torch.int32).argmax(1).to(torch.int32)          # the lowest index that attains the minimum
        first[best == inf] = -1
        dmin = torch.empty(M, dtype=torch.float64) if dmin is None else dmin
        imin = torch.empty(M, dtype=torch.int32) if imin is None else imin
        dmin[:M] = best
        imin[:M] = first
        return dmin, imin
