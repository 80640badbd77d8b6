"""TEST INFRASTRUCTURE: emulator statement of the selection entries of csrc/mifid.hip (HipOps.sqdist_rowmin_bounds, sqdist_rowmin,
kmeans_update) in float64 torch on the CPU, on top of tests/emulator_mifid.py, so that gan_variant_research_amd.select_7k runs without
a GPU.  The same argument checks, the same extents written, the kernels' expanded-form distance clipped at 0 and lowest-index ties.
Never imported by the product package."""
from __future__ import annotations

import torch

from gan_variant_research_amd._lib import GanError
from tests.emulator_mifid import TM, MifidEmuOps, _feat, _vec


def _xform(x, c, s):
    X = _feat(x)
    K = X.shape[1]
    c, s = _vec(c, K), _vec(s, K)
    if c is not None:
        X = X - c[None, :]
    if s is not None:
        X = X * s[None, :]
    return X


class EmuU8Pipeline:
    """dataio.InputPipeline.run_u8 for inference jobs (whole image -> S x S) with Pillow's resize, for the folder path on the CPU."""

    def __init__(self, image_size, device, max_batch=64, max_rows=1024, filter=2):
        self.S, self.filter = image_size, filter

    def run_u8(self, images, jobs, out=None):
        import numpy as np
        from PIL import Image
        arr = np.stack([np.asarray(Image.fromarray(im.cpu().numpy()).resize((self.S, self.S), self.filter)) for im in images])
        return torch.from_numpy(arr).permute(0, 3, 1, 2).contiguous()


class SelectEmuOps(MifidEmuOps):
    def sqdist_rowmin_bounds(self, M, N):
        if M <= 0 or N <= 0:
            raise GanError(f"sqdist_rowmin_bounds: extents must be positive (M={M} N={N})")
        pairs = -(-N // TM) * M
        return -(-((M + N) * 8) // 16) * 16 + -(-(pairs * 8) // 16) * 16 + pairs * 4

    def sqdist_rowmin(self, a, b, ca=None, sa=None, cb=None, sb=None, ws=None, dmin=None, imin=None):
        A, B = _xform(a, ca, sa), _xform(b, cb, sb)
        M, N = A.shape[0], B.shape[0]
        if B.shape[1] != A.shape[1]:
            raise GanError("sqdist_rowmin: row lengths differ")
        if ws is not None and ws.numel() < self.sqdist_rowmin_bounds(M, N):
            raise GanError("sqdist_rowmin: workspace below gan_sqdist_rowmin_bounds")
        d = ((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :]) - 2.0 * (A @ B.t())
        d = torch.where(d < 0, torch.zeros_like(d), d)
        best = d.min(1).values
        first = (d == best[:, None]).to(torch.int32).argmax(1).to(torch.int32)          # the lowest index that attains the minimum
        dmin = torch.empty(M, dtype=torch.float64) if dmin is None else dmin
        imin = torch.empty(M, dtype=torch.int32) if imin is None else imin
        dmin[:M] = best
        imin[:M] = first
        return dmin, imin

    def kmeans_update(self, x, labels, k, c=None, s=None, sums=None, counts=None, err=None):
        X = _xform(x, c, s)
        n, D = X.shape
        k = int(k)
        if k < 1:
            raise GanError(f"kmeans_update: k = {k}")
        assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == n
        sums = torch.empty(k, D, dtype=torch.float64) if sums is None else sums
        counts = torch.empty(k, dtype=torch.int32) if counts is None else counts
        err = torch.empty(1, dtype=torch.int32) if err is None else err
        assert sums.dtype == torch.float64 and tuple(sums.shape) == (k, D) and counts.dtype == torch.int32 and counts.numel() >= k
        ok = (labels >= 0) & (labels < k)
        lab = labels[ok].long()
        S = torch.zeros(k, D, dtype=torch.float64)
        S.index_add_(0, lab, X[ok])                                # rows in ascending order
        sums.copy_(S)
        counts[:k] = torch.bincount(lab, minlength=k).to(torch.int32)
        err[0] = 0 if bool(ok.all()) else 1
        return sums, counts, err
